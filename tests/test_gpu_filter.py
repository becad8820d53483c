"""The time-filter kernels of contrack_amd/csrc/ctk_filter.hip (k_filter_ring, k_filter_plain) against the numpy statement of
tests/filter_util.py, bit for bit: every form at the K edges ctk_filter_plan reports, every tile edge, strides around K, segment breaks
inside a tile, NaN / inf / signed zeros / denormals, weights of either sign.  Forms and tiles other than the rule's are reached through
Tracker.debug_set_filter; what a launch took is read back through Tracker.debug_filter_launch.  Planes are 3 x 85 (255 pixels: less
than a workgroup, no multiple of 64) and 7 x 67 (469: two workgroups with a tail)."""
import ctypes as C

import numpy as np
import pytest

from contrack_amd import _native

import filter_util as fu
from filter_util import same_bits

pytestmark = pytest.mark.gpu

RING, PLAIN = 1, 0
SMALL, TWO = (3, 85), (7, 67)


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


@pytest.fixture
def steer(trk):
    """debug_set_filter for the length of one test"""
    yield trk.debug_set_filter
    trk.debug_set_filter(0, 0, -1)


def _weights(K, seed=0, positive=False):
    """K weights no two of which are equal, of either sign unless `positive`, that do not sum to 1"""
    rng = np.random.default_rng(100 + seed)
    w = rng.uniform(0.05, 1.0, size=K) if positive else rng.uniform(-1.0, 1.0, size=K)
    return w + np.arange(K) * 1e-3


def _dev(trk, x, weights, byte_off=0, **kw):
    """the _dev entry on device copies that start byte_off bytes past an allocation (0: 16-byte aligned)"""
    T, ny, nx = x.shape
    K = weights if np.ndim(weights) == 0 else len(weights)
    first, _, _ = _native.filter_layout(T, K, kw.get("stride", 1), kw.get("offset"), kw.get("segments"))
    out = np.empty((len(first), ny, nx), dtype=x.dtype)
    xin, xout = trk.malloc(x.nbytes + 64), trk.malloc(out.nbytes + 64)
    try:
        pin, pout = C.c_void_p(xin.value + byte_off), C.c_void_p(xout.value + byte_off)
        trk.h2d(pin, x)
        assert trk.time_filter_dev(pin, T, ny, nx, weights, pout, f64=x.dtype == np.float64, **kw) == len(first)
        if out.size:
            trk.d2h(out, pout)
    finally:
        trk.free(xin)
        trk.free(xout)
    return out


# ---- 1. every form at the K edges of the plan ---------------------------------------------------------------------------------------
FORM_EDGES = [(np.float32, K) for K in (32, 33, 64, 65, 128, 129)] + [(np.float64, K) for K in (16, 17, 32, 33, 64, 65)]


@pytest.mark.parametrize("dtype,K", FORM_EDGES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_every_form_at_its_edge(trk, steer, dtype, K):
    """the largest K of every thread count and the first of the next, weighted and box: the rule's form, then the plain form forced"""
    T, (ny, nx) = 2 * K + 37, SMALL
    x = fu.edge_field(T, ny, nx, dtype, seed=K)
    elem = np.dtype(dtype).itemsize
    plan = _native.filter_plan(elem, K, 1, T, ny * nx)
    fits = K * 64 * elem <= 32768
    assert plan["form"] == (RING if fits else PLAIN)
    for weights in (_weights(K, K), K):
        want = fu.time_filter(x, weights)
        assert np.isfinite(want[K:-K]).any()
        for forced in (-1, PLAIN):
            steer(0, 0, forced)
            got = trk.time_filter(x, weights)
            launch = trk.debug_filter_launch()
            want_form = PLAIN if forced == PLAIN else plan["form"]
            assert launch["form"] == want_form and launch["launches"] == 1 and (launch["o0"], launch["o1"]) == (0, T), (K, forced, launch)
            if want_form == RING:
                assert (launch["threads"], launch["lds"]) == (plan["threads"], K * plan["threads"] * elem), (K, launch)
            assert same_bits(got, want), (dtype.__name__, K, np.ndim(weights) == 0, forced)
    steer(0, 0, RING)                                         # (asked for where none fits: the plain form, and it says so)
    trk.time_filter(x[:K + 3], K)
    assert trk.debug_filter_launch()["form"] == (RING if fits else PLAIN)


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
@pytest.mark.parametrize("form", (RING, PLAIN))
def test_tile_edges(trk, steer, dtype, form):
    """a tile of 1, one longer than T_out, T_out one more than a multiple of the tile, and tiles grown by a cap on gridDim.y; with a
    segment break inside a tile"""
    K, (ny, nx) = 7, TWO
    waves = -(-ny * nx // 64)
    w = _weights(K, 7)
    for T, ww, gm, tile, segments in ((61, 1 << 40, 0, 1, None), (61, 1, 0, 61 * waves, None), (61, 61 * waves // 12, 0, 12, [0, 30]),
                                      (61, 1 << 40, 5, 13, [0, 14, 15, 33]), (400, 400 * waves // 57, 0, 57, None)):
        x = fu.edge_field(T, ny, nx, dtype, seed=T + tile)
        for edges, wts in (("nan", w), ("renorm", _weights(K, 8, positive=True))):
            want = fu.time_filter(x, wts, edges=edges, segments=segments)
            steer(ww, gm, form)
            got = trk.time_filter(x, wts, edges=edges, segments=segments)
            launch = trk.debug_filter_launch()
            assert launch["form"] == form and launch["tile"] == min(tile, 1024) and launch["gy"] == -(-T // launch["tile"]), (T, ww, gm, launch)
            assert same_bits(got, want), (dtype.__name__, form, T, ww, gm, edges)
    assert 400 % 57 == 1 and 61 % 12 == 1


# ---- 3. strides and offsets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
def test_strides_and_offsets(trk, steer, dtype):
    """strides 1, 2, 4, K - 1, K, K + 1, offsets that put the first and the last window partly outside, both edge rules, every form
    that can run (the ring is forced at stride >= K too, where the rule takes the plain form)"""
    K, T, (ny, nx) = 6, 83, SMALL
    x = fu.edge_field(T, ny, nx, dtype, seed=5)
    for stride in (1, 2, 4, K - 1, K, K + 1):
        for offset in (None, -(K - 1), -2, 3):
            for edges in ("nan", "renorm"):
                for weights in (_weights(K, stride, positive=True), K):
                    want = fu.time_filter(x, weights, stride=stride, offset=offset, edges=edges)
                    for forced in (-1, RING, PLAIN):
                        steer(1 << 40 if forced == RING else 0, 0, forced)
                        got = trk.time_filter(x, weights, stride=stride, offset=offset, edges=edges)
                        rule = RING if stride < K else PLAIN
                        assert trk.debug_filter_launch()["form"] == (rule if forced < 0 else forced)
                        assert same_bits(got, want), (dtype.__name__, stride, offset, edges, np.ndim(weights) == 0, forced)
    first, label, _ = _native.filter_layout(T, K, 4, -2)
    assert first[0] < 0 and first[-1] + K > T                # (the first and the last window do hang over the ends)


# ---- 4. segments ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
def test_segments(trk, steer, dtype):
    """breaks inside a tile, a segment of one step, a segment shorter than K: all NaN under 'nan', renormalised under 'renorm'"""
    K, T, (ny, nx) = 5, 70, TWO
    starts = [0, 1, 4, 30, 31, 47, 66]                        # segments of 1, 3 (< K), 26, 1, 16, 19 and 4 (< K) steps
    x = np.abs(fu.edge_field(T, ny, nx, dtype, seed=9)) + dtype(1)
    x[np.isinf(x)] = dtype(2)
    x[np.isnan(x)] = dtype(3)
    w = _weights(K, 3, positive=True)
    for weights in (w, K):
        for stride, offset in ((1, None), (2, 0), (3, -1)):
            for edges in ("nan", "renorm"):
                want = fu.time_filter(x, weights, stride=stride, offset=offset, edges=edges, segments=starts)
                for forced in (RING, PLAIN):
                    steer(0, 0, forced)
                    got = trk.time_filter(x, weights, stride=stride, offset=offset, edges=edges, segments=starts)
                    assert same_bits(got, want), (dtype.__name__, stride, offset, edges, forced)
                if stride == 1:
                    short = np.r_[0:4, 30, 66:70]
                    assert np.all(np.isnan(want[short])) if edges == "nan" else np.all(np.isfinite(want[short]))
                    assert np.all(np.isfinite(want[6:28]))


# ---- 5. data and weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
def test_special_values_and_skipna(trk, steer, dtype):
    """NaN, +-inf, +-0.0 and denormals propagate as in the statement; skipna with all taps NaN gives NaN, with one finite tap that tap
    renormalised; the sign of a zero result is kept"""
    K, T, (ny, nx) = 4, 64, SMALL
    x = fu.edge_field(T, ny, nx, dtype, seed=21)
    x[10:20, 0, :8] = np.nan                                  # ten NaN steps: windows with all taps NaN
    x[14, 0, :4] = dtype(7.5)                                 # ... and windows with one finite tap among them
    x[30:40, 1, :8] = dtype(-0.0)                             # windows of -0.0 alone: 0.0 + (w * -0.0)
    x[30:40, 2, :8] = np.finfo(dtype).tiny / 2
    pos = _weights(K, 4, positive=True)
    for weights, skipna, edges in ((_weights(K, 5), False, "nan"), (pos, True, "nan"), (pos, True, "renorm"), (pos, False, "renorm"), (K, True, "nan"),
                                   (K, False, "renorm"), (K, True, "renorm")):
        want = fu.time_filter(x, weights, skipna=skipna, edges=edges)
        for forced in (RING, PLAIN):
            steer(0, 0, forced)
            got = trk.time_filter(x, weights, skipna=skipna, edges=edges)
            assert same_bits(got, want), (dtype.__name__, np.ndim(weights) == 0, skipna, edges, forced)
        if skipna:
            assert np.all(np.isnan(want[15:18, 0, 4:8])) and np.all(np.isfinite(want[13:16, 0, :4]))
            if np.ndim(weights) == 0:
                assert np.all(want[13:16, 0, :4] == dtype(7.5))
    assert np.any(np.isinf(want)) and np.any(np.isnan(want))


def test_weights_and_single_tap(trk, steer):
    """weights that do not sum to 1, negative weights without renormalisation (a band-pass), K = 1 (weighted: w[0] * x; box: x itself)"""
    T, (ny, nx) = 50, SMALL
    x = fu.edge_field(T, ny, nx, np.float64, seed=2)
    import contrack_amd
    for weights in (np.array([3.0]), np.array([-0.25]), 1, np.array([2.0, 3.0, 4.0]), contrack_amd.lanczos_weights(21, 1 / 6.0, 1 / 2.5, kind="bandpass"),
                    contrack_amd.lanczos_weights(15, 0.1, kind="highpass")):
        want = fu.time_filter(x, weights)
        for forced in (-1, RING, PLAIN):
            steer(0, 0, forced)
            assert same_bits(trk.time_filter(x, weights), want), (weights, forced)
    assert np.array_equal(fu.time_filter(x, 1), x, equal_nan=True)      # (0.0 + -0.0 is +0.0: equal, not the same bits)
    with pytest.raises(ValueError):
        trk.time_filter(x, np.array([0.5, -0.5, 1.0]), edges="renorm")
    with pytest.raises(ValueError):
        trk.time_filter(x, np.array([0.5, -0.5, 1.0]), skipna=True)
    assert same_bits(trk.time_filter(x, 3), fu.time_filter(x, 3))       # (the handle is usable after a refusal)


# ---- 6. the device entry, aligned and not ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
def test_dev_entry_unaligned(trk, steer, dtype):
    """slabs that start one element past a 16-byte boundary, odd plane: the bits of the aligned call and of the host-array entry"""
    K, T, (ny, nx) = 9, 45, SMALL
    x = fu.edge_field(T, ny, nx, dtype, seed=11)
    w = _weights(K, 9)
    for kw in (dict(), dict(stride=3, offset=-4), dict(segments=np.array([0, 20, 21]), edges="renorm", stride=2)):
        weights = _weights(K, 9, positive=True) if "edges" in kw else w
        want = fu.time_filter(x, weights, **kw)
        for forced in (RING, PLAIN):
            steer(0, 0, forced)
            for off in (0, np.dtype(dtype).itemsize):
                assert same_bits(_dev(trk, x, weights, off, **kw), want), (dtype.__name__, kw, forced, off)
    with pytest.raises(ValueError):                           # (null slabs are refused)
        _native.check(_native.lib().ctk_filter_f32_dev(trk.handle, None, 10, 2, 2, None, 3, 1, -1, 0, 0, None, 0, None, 9))
