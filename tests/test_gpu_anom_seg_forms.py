"""The segmented and streamed anomaly kernels of contrack_amd/csrc/ctk_anom_seg.hip (k_anom_ring, k_anom_plain, k_clim_acc, k_clim_fin,
with k_clim_roll behind them) pinned bit for bit at the edges of the plan that launches them (ctk_anom_plan, csrc/ctk_forms.h; restated
in tests/anom_forms.py, which tests/test_anom_forms_host.py holds against the library without a GPU).

The yardstick is oracle/anom_port.py unchanged (anom_forms.expected).  Slabs are the wide recipe of tests/test_gpu_anom_exact.py with its
edges, and before a slab is used the test asserts on the CPU that it tells the port from the same computation with the raw anomaly left
unrounded, and (float64) with the window summed newest first or the group sums taken in falling t (anom_forms.assert_discriminates,
clim_reversed).  Every comparison is np.array_equal(..., equal_nan=True) with equal dtypes; no tolerance appears.  Tiles other than the
rule's are reached through Tracker.debug_set_anom; what a launch took is read back through Tracker.debug_anom_launch."""
import numpy as np
import pytest

from contrack_amd import _native

import anom_forms as af
from anom_forms import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


@pytest.fixture
def steer(trk):
    """debug_set_anom for the length of one test"""
    yield trk.debug_set_anom
    trk.debug_set_anom(0, 0)


def _elem(x):
    return x.dtype.itemsize


def _check_launch(trk, x, smooth, o0, o1, launches, ww=0, gm=0, case=None):
    """the last launch is what anom_forms.plan says for output steps [o0, o1)"""
    got = trk.debug_anom_launch()
    want = af.plan(_elem(x), smooth, o1 - o0, x.shape[1] * x.shape[2], ww, gm)
    want.update(o0=o0, o1=o1, launches=launches)
    assert got == want, (case, got, want)
    return got


def _resident_mean(trk, x):
    """x as the resident vertical mean: one level of weight 1 (0 + 1 * x, divided by 1: x's bits)"""
    out = trk.level_mean(x[:, None], [1.0], keep_resident=True)
    assert same(out, x)


# ---- 1. ring capacity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,smooth", af.RING_EDGE, ids=lambda v: getattr(v, "__name__", str(v)))
def test_ring_capacity_edge(trk, dtype, smooth):
    """the last two smoothings whose ring fits 32 KB and the first that does not, with segments of smooth - 1 steps (no output), of
    smooth steps (one output) and breaks at 1 and T - 1; the host-array entry, the resident mean and the stream give the port's bits"""
    x, group, G, starts = af.ring_edge_case(dtype, smooth)
    T = x.shape[0]
    want, want_c = af.assert_discriminates(x, group, G, 4, smooth, starts)
    form = af.RING if smooth <= af.ring_steps(_elem(x)) else af.PLAIN
    got, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=starts)
    assert _check_launch(trk, x, smooth, 0, T, 1, case=("host array", smooth))["form"] == form == trk.debug_anom_form()
    assert same(clim, want_c) and same(got, want), ("host array", dtype.__name__, smooth)
    _resident_mean(trk, x)
    got, clim = trk.anomalies_resident(group, G, window=4, smooth=smooth, want_clim=True, segments=starts)
    assert _check_launch(trk, x, smooth, 0, T, 1, case=("resident mean", smooth))["form"] == form
    assert same(clim, want_c) and same(got, want), ("resident mean", dtype.__name__, smooth)
    for chunk in (smooth - 1, smooth, T):
        got, clim = trk.anomalies_stream(x, group, G, window=4, smooth=smooth, chunk_steps=chunk, segments=starts, want_clim=True)
        ls = af.stream_launches(T, smooth, chunk)
        assert _check_launch(trk, x, smooth, ls[-1][0], ls[-1][1], len(ls), case=("stream", smooth, chunk))["form"] == form
        assert same(clim, want_c) and same(got, want), ("stream", dtype.__name__, smooth, chunk)


# ---- 2. tile edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", af.TILE_EDGE, ids=lambda c: "%s-smooth%d-tile%d" % (c[0].__name__, c[1], c[2]))
def test_tile_edges(trk, steer, case):
    """tiles of 33, of 157 (no multiple of 8) and of 256 reached by the clamp, nt = 2 tile - 1, 2 tile, 2 tile + 1, one break at
    tile - 1, tile or tile + 1: a valid window straddles the boundary of two workgroups' tiles, or ends on it"""
    dtype, smooth, tile = case
    for nt in (2 * tile - 1, 2 * tile, 2 * tile + 1):
        ww, gm = af.overrides_for_tile(np.dtype(dtype).itemsize, smooth, nt, 130, tile)
        steer(ww, gm)
        for brk in (tile - 1, tile, tile + 1):
            x, group, G, starts = af.tile_edge_case(dtype, smooth, tile, nt, brk)
            want, want_c = af.assert_discriminates(x, group, G, 4, smooth, starts)
            got, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=starts)
            l = _check_launch(trk, x, smooth, 0, nt, 1, ww, gm, case=(case, nt, brk))
            assert l["tile"] == tile and l["gy"] == (3 if nt > 2 * tile else 2) and l["form"] == af.RING, (case, nt, l)
            assert same(clim, want_c) and same(got, want), (case, nt, brk)


# ---- 3. the gridDim.y rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("form", [af.RING, af.PLAIN], ids=["ring", "plain"])
def test_grid_y_rule_through_the_override(trk, steer, form, dtype):
    """grid_y_max = 3 at T = 200: the tile is raised to ceil(200 / 3) = 67 in either form; breaks around the first boundary and on the
    second.  Streamed in chunks of 67 + smooth - 1 the launches are shorter and the rule raises their tiles less."""
    T, npix = 200, 130
    smooth = 5 if form == af.RING else af.ring_steps(np.dtype(dtype).itemsize) + 1
    x = af.slab(np.random.default_rng(200 + smooth), T, (2, 65), dtype)
    group, G, starts = af.run_groups(T), 12, [0, 66, 67, 68, 134]
    want, want_c = af.assert_discriminates(x, group, G, 4, smooth, starts)
    steer(0, 3)
    got, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=starts)
    l = _check_launch(trk, x, smooth, 0, T, 1, 0, 3, case=(form, dtype.__name__))
    assert l["tile"] == 67 and l["gy"] == 3 and l["form"] == form, l
    assert same(clim, want_c) and same(got, want), (form, dtype.__name__)
    chunk = 67 + smooth - 1
    got, _ = trk.anomalies_stream(x, group, G, window=4, smooth=smooth, chunk_steps=chunk, segments=starts)
    ls = af.stream_launches(T, smooth, chunk)
    l = _check_launch(trk, x, smooth, ls[-1][0], ls[-1][1], len(ls), 0, 3, case=(form, dtype.__name__, "stream"))
    assert l["gy"] <= 3 and same(got, want), (form, dtype.__name__, "stream", l)


@pytest.mark.parametrize("smooth", [2, 33], ids=["ring-smooth2", "plain-smooth33"])
def test_grid_y_rule_at_its_true_size(trk, smooth):
    """one float32 pixel, T = 65535 x 32 + 1: the plain form's tile of 32 would need 65 536 workgroups in y and is raised to 33; the
    ring form's waves term gives 127.  4099 cyclic groups keep the port's per-group loop at 512 rounds, a segment every 100 003 steps.
    The port takes 0.2 s for either smoothing at this size (measured on the host, with its conditions 0.6 s)."""
    T, G = 65535 * 32 + 1, 4099
    x = af.slab(np.random.default_rng(5), T, (1, 1), np.float32)
    group = (np.arange(T) % G).astype(np.int32)
    starts = list(range(0, T, 100003))
    want, want_c = af.assert_discriminates(x, group, G, 5, smooth, starts)
    got, clim = trk.anomalies(x, group, G, window=5, smooth=smooth, want_clim=True, segments=starts)
    l = _check_launch(trk, x, smooth, 0, T, 1, case=("true size", smooth))
    assert (l["form"], l["tile"], l["gy"]) == ((af.RING, 127, 16513) if smooth == 2 else (af.PLAIN, 33, 63550)), l
    assert same(clim, want_c) and same(got, want), smooth


# ---- 4. streamed pass 2 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("form", [af.RING, af.PLAIN], ids=["ring", "plain"])
def test_streamed_pass2_chunk_edges(trk, form, dtype):
    """chunks of 1, smooth - 1, smooth, tile - 1, tile, tile + 1, 2 tile + 3, T and T + 5 steps through the array entries and the
    callbacks: the resident call's bits, the port's bits, and the launches anom_forms predicts (their number, the last one's steps
    and plan)"""
    T, tile = 150, 32
    smooth = 5 if form == af.RING else af.ring_steps(np.dtype(dtype).itemsize) + 1
    x = af.slab(np.random.default_rng(150 + smooth), T, (2, 65), dtype)
    group, G, starts = af.run_groups(T), 12, [0, 11, 12, 37, 100]
    want, want_c = af.assert_discriminates(x, group, G, 4, smooth, starts)
    res, clim = trk.anomalies(x, group, G, window=4, smooth=smooth, want_clim=True, segments=starts)
    assert _check_launch(trk, x, smooth, 0, T, 1)["tile"] == tile
    assert same(res, want) and same(clim, want_c), (form, dtype.__name__, "resident")
    _resident_mean(trk, x)
    res2, _ = trk.anomalies_resident(group, G, window=4, smooth=smooth, segments=starts)
    assert same(res2, want), (form, dtype.__name__, "resident mean")
    for chunk in sorted({1, smooth - 1, smooth, tile - 1, tile, tile + 1, 2 * tile + 3, T, T + 5}):
        ls = af.stream_launches(T, smooth, chunk)
        a, c = trk.anomalies_stream(x, group, G, window=4, smooth=smooth, chunk_steps=chunk, segments=starts, want_clim=True)
        _check_launch(trk, x, smooth, ls[-1][0], ls[-1][1], len(ls), case=("array", chunk))
        assert same(a, res) and same(c, clim), (form, dtype.__name__, "array", chunk)
        out = np.full_like(x, -1.0)
        writes = []

        def reader(t0, nt, dst):
            dst[...] = x[t0:t0 + nt]

        def writer(t0, nt, src):
            writes.append((t0, t0 + nt))
            out[t0:t0 + nt] = src
        _, c = trk.anomalies_stream(reader, group, G, window=4, smooth=smooth, sink=writer, shape=x.shape, dtype=x.dtype, chunk_steps=chunk,
                                    segments=starts, want_clim=True)
        _check_launch(trk, x, smooth, ls[-1][0], ls[-1][1], len(ls), case=("callbacks", chunk))
        assert writes == ls, (form, dtype.__name__, "callbacks", chunk, writes[:4], ls[:4])      # every launch's steps leave as one piece
        assert same(out, res) and same(c, clim), (form, dtype.__name__, "callbacks", chunk)
        # with the climatology handed in: pass 2 alone
        a, _ = trk.anomalies_stream(x, group, G, window=4, smooth=smooth, clim=clim, chunk_steps=chunk, segments=starts)
        assert same(a, res) and trk.debug_anom_launch()["launches"] == len(ls), (form, dtype.__name__, "clim=", chunk)


# ---- 5. the streamed climatology ------------------------------------------------------------------------------------------------
CLIM_CASES = af.clim_cases()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CLIM_CASES, ids=["G%d-%s-chunk%d-window%d-%dpx" % (c[0], c[1], c[2], c[3], c[4][0] * c[4][1]) for c in CLIM_CASES])
def test_streamed_climatology(trk, case, dtype):
    """k_clim_acc with 31, 32 stripes and more groups than stripes, k_clim_fin with groups that own no step, k_clim_roll with up to 64
    rows behind them: the stream's climatology is the resident call's and the port's, with and without pass 2"""
    G, rule, chunk, window, shape, T = case
    x, group = af.clim_case(dtype, case)
    with np.errstate(invalid="ignore"):
        want = af.anom_port.calc_clim(x, group, G, window).astype(dtype)
    if dtype == np.float64:
        assert af.differ_finite(af.clim_reversed(x, group, G, window), want), "the order of a group's additions is invisible"
    if rule == "alternating" and G > af.ACC_STRIPES:
        a, b = af.alternating_pair(G)
        assert a % af.ACC_STRIPES == b % af.ACC_STRIPES and a != b and chunk >= 2           # one stripe, both inside every chunk
    if rule in ("gaps", "one", "alternating"):
        assert np.bincount(group, minlength=G).min() == 0                                    # groups that own no step
    _, res = trk.anomalies(x, group, G, window=window, smooth=1, want_anom=False, want_clim=True, segments=[0])
    assert same(res, want), (case, dtype.__name__, "resident")
    a, c = trk.anomalies_stream(x, group, G, window=window, smooth=1, chunk_steps=chunk, want_clim=True)
    assert same(c, want), (case, dtype.__name__, "stream")
    want_a, _ = af.expected(x, group, G, window, 1, [0])
    assert same(a, want_a), (case, dtype.__name__, "stream, anomalies")
    _, c = trk.anomalies_stream(x, group, G, window=window, sink=False, chunk_steps=chunk, want_clim=True)
    assert same(c, want), (case, dtype.__name__, "stream, sink=False")


# ---- 6. many groups -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [65535, 65536])
def test_groups_at_the_grid_y_limit(trk, G):
    """k_clim_raw takes one workgroup row per group: 65 535 rows and 65 536, the first count past what other launches grid-stride for
    (tests/test_gpu_anom_exact.py runs 70 000 through ctk_anom_*).  A 1 x 3 slab of 7 steps in the first, a middle and the last but
    one group: every other group is empty, and the climatology there is the fill -- NaN with window 1, whose fill is the empty last group.  Every entry gives the port's bits."""
    T = 7
    x = af.slab(np.random.default_rng(G), T, (1, 3), np.float32, edges=False)
    x[2, 0, 1] = np.nan
    group = np.array([0, G - 2, G // 2, 0, G - 2, G // 2, G - 2], dtype=np.int32)
    starts = [0, 4]
    for window in (1, 3):
        want, want_c = af.expected(x, group, G, window, 2, starts)
        assert np.isfinite(want).any() and np.isnan(want_c).any() == (window == 1)
        got, clim = trk.anomalies(x, group, G, window=window, smooth=2, want_clim=True, segments=starts)
        assert same(clim, want_c) and same(got, want), (G, window, "host array")
        _resident_mean(trk, x)
        got, clim = trk.anomalies_resident(group, G, window=window, smooth=2, want_clim=True, segments=starts)
        assert same(clim, want_c) and same(got, want), (G, window, "resident mean")
        got, clim = trk.anomalies_stream(x, group, G, window=window, smooth=2, chunk_steps=3, segments=starts, want_clim=True)
        assert same(clim, want_c) and same(got, want), (G, window, "stream")


def test_set_anom_refuses_negative_values(trk):
    for bad in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            trk.debug_set_anom(*bad)
    x = af.slab(np.random.default_rng(1), 40, (1, 5), np.float32)
    group = af.run_groups(40)
    want, _ = af.expected(x, group, 12, 1, 3, [0, 9])
    assert same(trk.anomalies(x, group, 12, smooth=3, segments=[0, 9])[0], want)
    assert trk.debug_anom_launch()["tile"] == 32                                              # the rule's values are still in place
