"""k_overlap on constructed slabs (tests/handover_cases.py: no common pixel, every pixel common, exactly 64 and 65 words with common
pixels in one wave's step, runs across every word boundary in t, in t-1 and in both, words first in their row, 32 pieces a word, more
distinct pairs than the LDS hash holds, past-the-end words) on the smallest shapes of every instance.  Flags and n_tracked must be
bit-identical to oracle/scipy_port.run_contrack -- the reference's own call sequence, computed once per slab -- on the fused pass
twice on one handle and on the synchronous path; CTK_S_OVERLAP_FORM must name the instance tests/label_forms.py predicts; no call may
leave the device path (CTK_S_HOST_PATH, CTK_S_HOST_REASON) or meet a decision on a rounding boundary."""
import numpy as np
import pytest

import handover_cases as hc
import label_forms as lf
import segment_util as su
from contrack_amd import _native
from oracle import scipy_port

pytestmark = pytest.mark.gpu

GORL, OVERLAP, PERSISTENCE, TWOSIDED = ">=", 0.5, 2, True
OP = _native.CMP_OPS[GORL]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")


def _inputs(mask, oracle):
    """a field of two values, +-1 around a threshold of 0; the row weights of a regular grid pole to pole"""
    T, ny, nx = mask.shape
    anom = np.where(mask.astype(bool), np.float32(1.0), np.float32(-1.0))
    lat = np.linspace(90, -90, ny).astype(np.float32)
    w = oracle.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    return anom, oracle.prepare_thresholds(0.0, T), w


def _check_stats(trk, shape, seg, fused):
    T, ny, nx = shape
    st = trk.stats()
    want = lf.overlap_form(T, ny, (nx + 63) // 64, seg)
    assert st["overlap_form"] == want, "%s, predicted %s" % (lf.overlap_name(st["overlap_form"]), lf.overlap_name(want))
    assert st["host_path"] == 0 and st["off_fused_path_reason"] == 0 and st["ambiguous_decisions"] == 0, st
    assert st["fused_pass"] == (1 if fused else 0)
    return st


def _dev_calls(trk, anom, thr, w, want, seg=False):
    """track_dev twice on the fused pass, then once on the synchronous path, each against `want`; the statistics of the three calls"""
    T, ny, nx = anom.shape
    d_in, d_out = trk.malloc(anom.nbytes), trk.malloc(anom.size * 4)
    stats = []
    try:
        trk.h2d(d_in, anom)
        out = np.empty(anom.shape, dtype=np.int32)
        for fused in (True, True, False):
            trk.set_fused(fused)
            trk.memset(d_out, 0xff, anom.size * 4)
            n = trk.track_dev(d_in, T, ny, nx, thr, OP, w, OVERLAP, PERSISTENCE, TWOSIDED, d_out)
            trk.d2h(out, d_out)
            assert np.array_equal(out, want[0]), "%s: flag differs at %d pixels" % ("fused" if fused else "synchronous", int((out != want[0]).sum()))
            assert n == want[1]
            stats.append(_check_stats(trk, anom.shape, seg, fused))
    finally:
        trk.set_fused(True)
        trk.free(d_in)
        trk.free(d_out)
    return stats


@pytest.mark.parametrize("name,case,shape", hc.all_slabs(), ids=lambda v: v if isinstance(v, str) else "")
def test_slab(name, case, shape, oracle_lib):
    mask = hc.build(case, shape)
    anom, thr, w = _inputs(mask, oracle_lib)
    del mask
    want = scipy_port.run_contrack(anom, 0.0, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
    with _native.Tracker(0) as trk:
        stats = _dev_calls(trk, anom, thr, w, want)
    ny, nx, _ = shape
    if case == "alt_both" and ny * nx >= 32 * 128:                   # more distinct pairs than hash slots: the ungrouped tail took some
        assert all(s["ungrouped_pairs"] > 0 for s in stats[:2])


def test_segment_break(oracle_lib):
    """the SEG build of <5,256>: 181 x 360 with a break at t = 2, each segment against scipy_port, the numbering of the whole against
    tests/segment_util.expected"""
    ny, nx, T = hc.SHAPES[0]
    starts = np.array([0, 2])
    for case in ("full", "cross", "alt_both"):
        anom, thr, w = _inputs(hc.slab(case, ny, nx, T), oracle_lib)
        want = su.expected(anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED, starts)
        for a, b in ((0, 2), (2, T)):
            f, _ = scipy_port.run_contrack(anom[a:b], 0.0, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
            assert np.array_equal(f > 0, want[0][a:b] > 0)
            first = int(want[0][a:b].max()) - int(f.max())               # labels of a segment: the port's, shifted by those before
            assert np.array_equal(np.where(f > 0, f + first, 0), want[0][a:b])
        with _native.Tracker(0) as trk:
            trk.set_segments(starts)
            try:
                _dev_calls(trk, anom, thr, w, want, seg=True)
            finally:
                trk.clear_segments()
