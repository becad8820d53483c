"""Segment breaks (ctk_set_segments, run_contrack(segments=...)): independent time segments tracked in one call.  Every segment must
be, bit for bit, the reference run on that segment alone (tests/segment_util.py builds it from the C oracle), its ids shifted by the
3-D components of the segments before it; n_tracked is len(np.unique(flag)) - 1 of the whole result."""
import numpy as np
import pytest

import golden_util
import segment_util as su
from contrack_amd import _native

pytestmark = pytest.mark.gpu

CASES = golden_util.case_names()


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def seg_track(trk, g, starts, f64=False):
    trk.set_segments(starts)
    try:
        a = g["anom"].astype(np.float64) if f64 else g["anom"]
        flag, n = trk.track(a, g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"], f64=f64)
        return flag.copy(), n
    finally:
        trk.clear_segments()


def check_case(trk, name, f64=False):
    g = golden_util.load(name)
    T = g["anom"].shape[0]
    for sname, starts in su.segmentations(T).items():
        want, nw = su.expected(g["anom"], g["thr"], g["gorl"], g["wrow"], g["overlap"], g["persistence"], g["twosided"], starts)
        got, ng = seg_track(trk, g, starts, f64=f64)
        assert np.array_equal(got, want), "{} / {}: flag differs at {} pixels".format(name, sname, int((got != want).sum()))
        assert ng == nw, "{} / {}: n_tracked {} != {}".format(name, sname, ng, nw)
        if sname == "one":
            assert np.array_equal(got, g["flag"])


@pytest.mark.parametrize("name", CASES)
def test_goldens_segmented(trk, name):
    check_case(trk, name)


@pytest.mark.parametrize("mode", ["sync", "host_resolver", "seam_caps", "pair_regrow", "f64"])
def test_goldens_segmented_paths(trk, mode):
    """the fall-backs give what the fused path gives: synchronous device resolve, the host resolver, the host seam driver, a
    pair table that has to be regrown, float64 input"""
    t = _native.Tracker(0)
    try:
        if mode == "sync":
            t.set_fused(False)
        elif mode == "host_resolver":
            t.set_device_resolve(False)
        elif mode == "seam_caps":
            t.debug_set_seam_caps(1, 1)
        elif mode == "pair_regrow":
            t.debug_set_pair_capacity(64)
        for name in CASES:
            check_case(t, name, f64=(mode == "f64"))
    finally:
        t.close()


def test_unsegmented_unchanged_and_sticky(trk):
    """segments apply to every call until cleared; after clearing, the handle gives the unsegmented golden again"""
    g = golden_util.load("syn2deg_s0")
    args = (g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    starts = np.array([0, 20, 21, 50])
    want, nw = su.expected(g["anom"], g["thr"], g["gorl"], g["wrow"], g["overlap"], g["persistence"], g["twosided"], starts)
    assert not np.array_equal(want, g["flag"])
    trk.set_segments(starts)
    try:
        for _ in range(2):
            got, ng = trk.track(g["anom"], *args)
            assert np.array_equal(got, want) and ng == nw
    finally:
        trk.clear_segments()
    got, ng = trk.track(g["anom"], *args)
    assert np.array_equal(got, g["flag"])
    trk.set_segments([0])
    try:
        got, ng = trk.track(g["anom"], *args)
        assert np.array_equal(got, g["flag"])
    finally:
        trk.clear_segments()


def test_threshold_field_with_segments(trk):
    """a threshold field composes with segments: a constant field at the golden's thresholds is the per-step path"""
    g = golden_util.load("syn2deg_s1")
    T, ny, nx = g["anom"].shape
    planes = np.broadcast_to(np.float32(g["thr"][0]), (1, ny, nx)).copy()
    assert np.all(g["thr"] == g["thr"][0])
    starts = np.array([0, 7, 30, 31, 60])
    want, nw = su.expected(g["anom"], g["thr"], g["gorl"], g["wrow"], g["overlap"], g["persistence"], g["twosided"], starts)
    trk.set_threshold_field(planes, np.zeros(T, dtype=np.int32))
    trk.set_segments(starts)
    try:
        got, ng = trk.track(g["anom"], None, _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"])
        got = got.copy()
    finally:
        trk.clear_segments()
        trk.clear_threshold_field()
    assert np.array_equal(got, want) and ng == nw


def test_dev_and_resident_entries(trk):
    g = golden_util.load("syn2deg_s2")
    a = g["anom"]
    T, ny, nx = a.shape
    starts = np.array([0, 1, 24, 48, 70])
    want, nw = su.expected(a, g["thr"], g["gorl"], g["wrow"], g["overlap"], g["persistence"], g["twosided"], starts)
    op = _native.CMP_OPS[g["gorl"]]
    d_in = trk.malloc(a.nbytes)
    d_out = trk.malloc(a.size * 4)
    try:
        trk.h2d(d_in, a)
        trk.set_segments(starts)
        try:
            n = trk.track_dev(d_in, T, ny, nx, g["thr"], op, g["wrow"], g["overlap"], g["persistence"], g["twosided"], d_out)
        finally:
            trk.clear_segments()
        got = np.empty(a.shape, dtype=np.int32)
        trk.d2h(got, d_out)
        assert np.array_equal(got, want) and n == nw
    finally:
        trk.free(d_in)
        trk.free(d_out)
    # resident slab: anomalies against a zero climatology (window 1, smooth 1) are the slab itself, left in HBM
    trk.anomalies(a, np.zeros(T, dtype=np.int32), 1, clim=np.zeros((1, ny, nx), dtype=np.float32), keep_resident=True, want_anom=False)
    trk.set_segments(starts)
    try:
        got, n = trk.track_resident(g["thr"], op, g["wrow"], g["overlap"], g["persistence"], g["twosided"])
        got = got.copy()
    finally:
        trk.clear_segments()
    assert np.array_equal(got, want) and n == nw


def test_refusals(trk):
    g = golden_util.load("T3")
    a = g["anom"]
    T, ny, nx = a.shape
    args = (g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    for bad in ([1, 2], [0, 2, 2], [0, 2, 1], [0, -1]):
        with pytest.raises(ValueError):
            trk.set_segments(bad)
    trk.set_segments([0, T])                           # legal to set; a call with T <= the last start is refused
    try:
        with pytest.raises(ValueError, match="segment"):
            trk.track(a, *args)
    finally:
        trk.clear_segments()
    trk.set_segments([0, 1])
    try:
        with pytest.raises(ValueError, match="segments"):
            trk.track_stream(a, *args)
        d_in = trk.malloc(a.nbytes)
        d_out = trk.malloc(a.size * 4)
        grp = _native.CommGroup(1)
        comm = _native.Comm.local(trk, grp, 0)
        try:
            trk.h2d(d_in, a)
            with pytest.raises(Exception, match="segments"):
                trk.track_sharded_dev(comm, d_in, T, 0, T, ny, nx, *args, d_out)
            with pytest.raises(ValueError, match="segments"):
                trk.shard_label2d(d_in, T, ny, nx, g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], 0)
        finally:
            comm.close()
            grp.close()
            trk.free(d_in)
            trk.free(d_out)
    finally:
        trk.clear_segments()
    flag, n = trk.track(a, *args)                        # the handle is fine afterwards
    assert np.array_equal(flag, g["flag"])
