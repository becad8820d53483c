"""Every k_rowcount, k_label2d_* and k_overlap form at both sides of its capacity edges, exactly against the C oracle: the staged
outputs (mask, 2-D labels before and after the seam merge, component / pair / seam tables: tests/staged_util.py), the one-call
flags of `track` and of `track_dev` twice on the same handle (the second call launches speculatively), and a call with a segment
break (the SEG builds of k_overlap, against tests/segment_util.expected).  The planes come from tests/label_forms.py, which
restates the selection; after every call the statistics CTK_S_LABEL_FORMS, CTK_S_OVERLAP_FORM, CTK_S_ROWCOUNT_THREADS and
CTK_S_ROWCOUNT_GROUPS must name the forms the restatement predicts, so a case that misses its form fails whatever its flags.
The rcu_* cases sit on the 4 | 5, 6 | 7 and 8 | 9 edges of the row groups a plane needs of k_rowcount<RCU>, with 256 and 512
threads, on the staged and the fused path.  Not covered: the 128-thread form with RCU 6 or 8 -- it needs more than 65536 planes
of at least 257 x 128, eight times the long shard below (tests/test_label_forms.py pins its rule on the host)."""
import numpy as np
import pytest

import label_forms as lf
import segment_util as su
import staged_util
from contrack_amd import _native

pytestmark = pytest.mark.gpu

GORL, OVERLAP, PERSISTENCE, TWOSIDED = ">=", 0.5, 2, True
OP = _native.CMP_OPS[GORL]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")


def _inputs(mask, oracle):
    """anomalies +-1 around a threshold of 0, the row weights of a regular grid pole to pole (pole rows: ~2^-20 of the equator's)"""
    T, ny, nx = mask.shape
    anom = np.where(mask.astype(bool), np.float32(1.0), np.float32(-1.0))
    thr = oracle.prepare_thresholds(0.0, T)
    lat = np.linspace(90, -90, ny).astype(np.float32)
    w = oracle.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    return anom, thr, w


def _expect_forms(trk, model, shape, runs, seg):
    T, ny, nx = shape
    W = (nx + 63) // 64
    st = trk.stats()
    want = model.label2d(T, ny, nx, runs)
    assert st["label_forms"] == want, "label forms %#x, predicted %#x" % (st["label_forms"], want)
    assert st["rowcount_threads"] == lf.rowcount_threads(T, ny, W)
    assert st["rowcount_groups"] == lf.rowcount_groups_stat(T, ny, W), \
        "k_rowcount<%d> ran, predicted %s" % (st["rowcount_groups"], lf.rowcount_name(T, ny, W))
    assert st["overlap_form"] == lf.overlap_form(T, ny, W, seg), \
        "%s, predicted %s" % (lf.overlap_name(st["overlap_form"]), lf.overlap_name(lf.overlap_form(T, ny, W, seg)))
    return st


def _one_call(trk, model, oracle, anom, thr, w, want=None):
    """track, then track_dev twice on the same handle; every result against the oracle and every call's forms"""
    T, ny, nx = anom.shape
    runs = lf.count_runs(anom > 0)
    if want is None:
        want = oracle.run_contrack(anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
    got, ng = trk.track(anom, thr, OP, w, OVERLAP, PERSISTENCE, TWOSIDED)
    assert np.array_equal(got, want[0]), "flag differs at %d pixels" % int((got != want[0]).sum())
    assert ng == want[1]
    del got
    st = [_expect_forms(trk, model, anom.shape, runs, False)]
    d_in, d_out = trk.malloc(anom.nbytes), trk.malloc(anom.size * 4)
    try:
        trk.h2d(d_in, anom)
        for _ in range(2):
            trk.memset(d_out, 0xff, anom.size * 4)
            n = trk.track_dev(d_in, T, ny, nx, thr, OP, w, OVERLAP, PERSISTENCE, TWOSIDED, d_out)
            out = np.empty(anom.shape, dtype=np.int32)
            trk.d2h(out, d_out)
            assert np.array_equal(out, want[0]) and n == want[1]
            del out
            st.append(_expect_forms(trk, model, anom.shape, runs, False))
    finally:
        trk.free(d_in)
        trk.free(d_out)
    return st


def _segmented(trk, model, oracle, anom, thr, w):
    T = anom.shape[0]
    starts = np.array([0, T // 2])
    want, nw = su.expected(anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED, starts)
    trk.set_segments(starts)
    try:
        got, ng = trk.track(anom, thr, OP, w, OVERLAP, PERSISTENCE, TWOSIDED)
        assert np.array_equal(got, want), "segmented flag differs at %d pixels" % int((got != want).sum())
        assert ng == nw
    finally:
        trk.clear_segments()
    return _expect_forms(trk, model, anom.shape, lf.count_runs(anom > 0), True)


def run_case(case, oracle):
    mask = lf.mask_of(case)
    anom, thr, w = _inputs(mask, oracle)
    del mask
    with _native.Tracker(0) as trk:
        model = lf.Handle()
        staged_util.check_staged(trk, oracle, anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
        stats = [_expect_forms(trk, model, anom.shape, lf.count_runs(anom > 0), False)]
        stats += _one_call(trk, model, oracle, anom, thr, w)
        if case["seg"] and anom.shape[0] >= 2:
            stats.append(_segmented(trk, model, oracle, anom, thr, w))
    return stats


FAST = [c for c in lf.CASES if not c["slow"]]


@pytest.mark.parametrize("case", FAST, ids=lambda c: c["name"])
def test_form_case(case, oracle_lib):
    stats = run_case(case, oracle_lib)
    if case["name"] == "pairs_600":                    # more distinct pairs in a timestep than the LDS hash holds (one-call stats)
        assert all(s["ungrouped_pairs"] > 0 for s in stats[1:])


def test_long_shard(oracle_lib):
    """T = 65537 planes of 32 x 128: <832,240,-1,256,256>, <1024,288,832,256>, k_overlap<4,128,5> (and its SEG build), the
    128-thread k_rowcount; the same handle first sees the shard without planes above 832 runs (no v1hi), then with them (v1hi
    missing from the speculative set), then without them again (v1hi in the speculative set)"""
    case = lf.CASE_BY_NAME["long_shard"]
    quiet = lf.mask_of(case, lf.long_schedule(lf.LONG_QUIET_KEYS)(lf.LONG_T))
    aq, thr, w = _inputs(quiet, oracle_lib)
    del quiet
    want_q = oracle_lib.run_contrack(aq, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
    with _native.Tracker(0) as trk:
        model = lf.Handle()
        st = _one_call(trk, model, oracle_lib, aq, thr, w, want_q)
        assert not st[0]["label_forms"] & lf.LABEL_BIT["v1hi_832"]
        mask = lf.mask_of(case)
        anom, _, _ = _inputs(mask, oracle_lib)
        del mask
        staged_util.check_staged(trk, oracle_lib, anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
        st = _expect_forms(trk, model, anom.shape, lf.count_runs(anom > 0), False)
        assert st["label_forms"] & lf.LABEL_BIT["v1hi_832"]
        _one_call(trk, model, oracle_lib, anom, thr, w)
        _segmented(trk, model, oracle_lib, anom, thr, w)
        del anom
        st = _one_call(trk, model, oracle_lib, aq, thr, w, want_q)
        assert st[0]["label_forms"] & lf.LABEL_BIT["v1hi_832"]          # speculatively, from the call before


def test_speculation_same_shape(oracle_lib):
    """one handle, one shape, calls whose launched sets differ (tests/label_forms.py SPEC_SEQUENCES[0]); each call against the
    oracle and its launched set against the restatement"""
    seq = lf.SPEC_SEQUENCES[0]
    seen = 0
    with _native.Tracker(0) as trk:
        model = lf.Handle()
        for T, sched in seq["calls"]:
            mask = lf.mask_of(dict(seq, schedule=sched, T=T), sched(T))
            anom, thr, w = _inputs(mask, oracle_lib)
            want = oracle_lib.run_contrack(anom, thr, GORL, w, OVERLAP, PERSISTENCE, TWOSIDED)
            got, ng = trk.track(anom, thr, OP, w, OVERLAP, PERSISTENCE, TWOSIDED)
            assert np.array_equal(got, want[0]) and ng == want[1]
            seen |= _expect_forms(trk, model, anom.shape, lf.count_runs(mask), False)["label_forms"]
    assert seen & lf.DISCARDED_BIT and seen & lf.LABEL_BIT["one"] and seen & lf.LABEL_BIT["glb"]


@pytest.mark.parametrize("shape", [(1, 1, 65536), (1, 65536, 1)])
def test_grid_beyond_65535_is_a_range_error(shape):
    a = np.zeros(shape, dtype=np.float32)
    w = np.ones(shape[1], dtype=np.float32)
    with _native.Tracker(0) as trk:
        with pytest.raises((_native.ContrackHipError, ValueError), match="exceeds 65535"):
            trk.track(a, np.zeros(1), OP, w, OVERLAP, PERSISTENCE, TWOSIDED)
