"""The host side of the time filter (no GPU): ctk_filter_layout against a brute-force enumeration, lanczos_weights against Duchon's closed
form, ctk_filter_plan at the capacity edges of every thread count, and the argument errors, which are named with a NULL handle too."""
import numpy as np
import pytest

import contrack_amd
from contrack_amd import _native

import filter_util as fu

SEGMENTS = ((20, None), (23, [0, 7, 15]), (5, [0, 1, 2, 3, 4]), (12, [0, 3, 10]), (9, [0, 1, 8]))      # (12, ...): a segment shorter than K = 4, 7
RING_BYTES = 32768


@pytest.mark.parametrize("K", (1, 2, 3, 4, 7))
@pytest.mark.parametrize("stride", (1, 2, 4, 7))
def test_layout_brute_force(K, stride):
    for offset in (None, -9, -K, -(K // 2), -1, 0, 1, K // 2, K, 11):
        for T, seg in SEGMENTS:
            first, label, out_starts = _native.filter_layout(T, K, stride, offset, seg)
            want = fu.layout(T, K, stride, offset, seg)
            case = (K, stride, offset, T, seg)
            assert np.array_equal(first, want[0]) and np.array_equal(label, want[1]) and np.array_equal(out_starts, want[2]), case
            # what the enumeration itself must satisfy: every label in its segment, labels strictly rising, at most one output per step
            assert len(label) <= T and np.all(np.diff(label) > 0), case
            for S, E in fu.segments_of(T, seg):
                inside = label[(label >= S) & (label < E)]
                assert np.all((inside - S - (fu.default_offset(K, stride) if offset is None else offset) - K // 2) % stride == 0), case


@pytest.mark.parametrize("K", (1, 2, 3, 4, 7))
def test_layout_stride_one_default_is_one_output_per_step(K):
    for T, seg in SEGMENTS:
        first, label, out_starts = _native.filter_layout(T, K, 1, None, seg)
        assert len(first) == T and np.array_equal(label, np.arange(T)) and np.array_equal(first, np.arange(T) - K // 2)
        assert np.array_equal(out_starts, [0] if seg is None else seg)
        label2, out_starts2, first2 = contrack_amd.filter_layout(T, K, segments=seg)
        assert np.array_equal(label2, label) and np.array_equal(out_starts2, out_starts) and np.array_equal(first2, first)


def test_lanczos_weights():
    for ntaps, fc in ((1, 0.2), (3, 0.25), (21, 0.1), (61, 1.0 / 10), (121, 1.0 / 30)):
        w = contrack_amd.lanczos_weights(ntaps, fc)
        assert w.dtype == np.float64 and w.shape == (ntaps,)
        assert np.array_equal(w, w[::-1]), "symmetry is exact: sin is odd and k enters as k and -k"
        # the sum of ntaps products each rounded to 2^-53 relative, of magnitude below 1: ntaps ulp of 1.0 bounds the error of the sum
        assert abs(w.sum() - 1.0) <= ntaps * np.finfo(np.float64).eps
        raw = fu.lanczos_closed_form(ntaps, fc)
        want = raw / raw.sum()
        # sin and pi * k are evaluated once vectorised, once per element: a few ulp of the largest weight
        assert np.max(np.abs(w - want)) <= 8 * np.finfo(np.float64).eps * np.max(np.abs(want))
        hp = contrack_amd.lanczos_weights(ntaps, fc, kind='highpass')
        delta = np.zeros(ntaps)
        delta[ntaps // 2] = 1.0
        assert np.max(np.abs(hp + w - delta)) <= np.finfo(np.float64).eps
    bp = contrack_amd.lanczos_weights(41, 1.0 / 6, 1.0 / 2.5, kind='bandpass')
    assert np.array_equal(bp, contrack_amd.lanczos_weights(41, 1.0 / 2.5) - contrack_amd.lanczos_weights(41, 1.0 / 6))
    assert np.array_equal(bp, contrack_amd.lanczos_weights(41, 1.0 / 2.5, 1.0 / 6, kind='bandpass'))
    assert abs(bp.sum()) <= 82 * np.finfo(np.float64).eps
    for bad in (0, 2, 20, 3.5, -3):
        with pytest.raises(ValueError):
            contrack_amd.lanczos_weights(bad, 0.1)
    with pytest.raises(ValueError):
        contrack_amd.lanczos_weights(21, 0.7)
    with pytest.raises(ValueError):
        contrack_amd.lanczos_weights(21, 0.1, kind='bandpass')
    with pytest.raises(ValueError):
        contrack_amd.lanczos_weights(21, 0.1, 0.2)


@pytest.mark.parametrize("elem", (4, 8))
def test_plan_capacity_edges(elem):
    nout, npix = 400, 469
    nxt = {256: 128, 128: 64, 64: None}
    for threads in (256, 128, 64):
        K = RING_BYTES // (threads * elem)                   # the largest K of this thread count
        p = _native.filter_plan(elem, K, 1, nout, npix)
        assert (p["form"], p["threads"], p["lds"]) == (1, threads, K * threads * elem), (elem, threads, p)
        assert p["lds"] == RING_BYTES and p["gx"] == -(-npix // threads)
        q = _native.filter_plan(elem, K + 1, 1, nout, npix)
        if nxt[threads] is None:
            assert (q["form"], q["threads"], q["lds"]) == (0, 256, 0), (elem, K + 1, q)
        else:
            assert (q["form"], q["threads"], q["lds"]) == (1, nxt[threads], (K + 1) * nxt[threads] * elem), (elem, K + 1, q)
            assert q["lds"] <= RING_BYTES
    assert RING_BYTES // (64 * elem) == (128 if elem == 4 else 64)
    for K in range(1, 140):
        for stride in (1, 2, K - 1, K, K + 1):
            if stride < 1:
                continue
            for forced in (-1, 0, 1):
                for ww, gm in ((0, 0), (1, 0), (1 << 40, 0), (0, 1), (0, 3), (0, 1 << 20)):
                    p = _native.filter_plan(elem, K, stride, nout, npix, ww, gm, forced)
                    case = (elem, K, stride, forced, ww, gm, p)
                    fits = K * 64 * elem <= RING_BYTES
                    ring = fits and forced != 0 and (stride < K or forced == 1)
                    assert p["form"] == int(ring), case
                    assert p["lds"] <= RING_BYTES and (p["lds"] == K * p["threads"] * elem if ring else p["lds"] == 0), case
                    assert p["threads"] in (64, 128, 256) and (ring or p["threads"] == 256), case
                    assert not ring or p["threads"] == 256 or K * 2 * p["threads"] * elem > RING_BYTES, case      # the most threads that fit
                    cap = min(gm, 65535) if gm > 0 else 65535
                    assert 1 <= p["gy"] <= cap and p["gy"] * p["tile"] >= nout > (p["gy"] - 1) * p["tile"], case
    assert _native.filter_plan(elem, 5, 1, 10 ** 9, 64)["gy"] <= 65535
    with pytest.raises(ValueError):
        _native.filter_plan(2, 5, 1, 10, 64)
    with pytest.raises(ValueError):
        _native.filter_plan(elem, 5, 1, 10, 64, forced=2)


def _call(K, stride, w, edges, skipna, starts, T=6, handle=None):
    L = _native.lib()
    x = np.zeros((T, 2, 3), dtype=np.float32)
    out = np.zeros_like(x)
    st = None if starts is None else np.asarray(starts, dtype=np.int64)
    wv = None if w is None else np.asarray(w, dtype=np.float64)
    rc = L.ctk_filter_f32(handle, x.ctypes.data, T, 2, 3, None if wv is None else wv.ctypes.data, K, stride, 0, edges, skipna,
                          None if st is None else st.ctypes.data, 0 if st is None else len(st), out.ctypes.data, T, 0, 0)
    return rc, L.ctk_last_error()


def test_argument_errors_with_a_null_handle():
    E = _native.CTK_E_INVALID
    rc, msg = _call(0, 1, None, 0, 0, None)
    assert rc == E and b"K = 0" in msg, msg
    rc, msg = _call(3, 0, None, 0, 0, None)
    assert rc == E and b"stride = 0" in msg, msg
    for edges, skipna in ((1, 0), (0, 1)):
        rc, msg = _call(3, 1, [0.5, -0.25, 0.75], edges, skipna, None)
        assert rc == E and b">= 0" in msg, msg
        rc, msg = _call(3, 1, [0.0, 0.0, 0.0], edges, skipna, None)
        assert rc == E and b"sum > 0" in msg, msg
    rc, msg = _call(3, 1, [0.5, -0.25, 0.75], 0, 0, None)                  # (a band-pass as it is: fine until the handle is looked at)
    assert rc == E and b"null handle" in msg, msg
    for bad in (np.nan, np.inf, -np.inf):
        rc, msg = _call(3, 1, [0.5, bad, 0.5], 0, 0, None)
        assert rc == E and b"finite" in msg, msg
    for starts in ([1, 3], [0, 3, 3], [0, 4, 2], [0, 6]):
        rc, msg = _call(3, 1, None, 0, 0, starts)
        assert rc == E and b"segment" in msg, (starts, msg)
    rc, msg = _call(3, 1, None, 2, 0, None)
    assert rc == E and b"edges" in msg, msg
    n = np.zeros(1, dtype=np.int64)
    L = _native.lib()
    assert L.ctk_filter_layout(6, 0, 1, 0, None, 0, None, None, n.ctypes.data) == E
    assert L.ctk_filter_layout(6, 3, 0, 0, None, 0, None, None, n.ctypes.data) == E
    assert L.ctk_filter_layout(0, 3, 1, 0, None, 0, None, None, n.ctypes.data) == E
    assert L.ctk_filter_layout(6, 3, 1, -1, None, 0, None, None, n.ctypes.data) == 0 and n[0] == 6
    with pytest.raises(ValueError):
        _native.filter_layout(6, 3, 1, None, [0, 7])
    with pytest.raises(ValueError):
        _native._filter_weights(2.5)
    with pytest.raises(ValueError):
        _native._filter_weights(np.zeros((2, 2)))


def test_numpy_statement_against_a_direct_dot():
    """the statement itself, where rounding cannot differ: small integers in float64, complete windows"""
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, size=(40, 2, 3)).astype(np.float64)
    w = np.array([1.0, -2.0, 4.0, 0.5, 3.0])
    got = fu.time_filter(x, w)
    for t in range(2, 38):
        assert np.array_equal(got[t], np.tensordot(w, x[t - 2:t + 3], axes=1))
    assert np.all(np.isnan(got[:2])) and np.all(np.isnan(got[38:]))
    daily = fu.time_filter(x, 4, stride=4)
    assert daily.shape[0] == 10 and np.array_equal(daily, x.reshape(10, 4, 2, 3).sum(axis=1) / 4.0)
    ren = fu.time_filter(x, np.ones(5), edges="renorm")
    assert np.array_equal(ren[0], x[:3].sum(axis=0) / 3.0) and np.array_equal(ren[39], x[37:].sum(axis=0) / 3.0)
