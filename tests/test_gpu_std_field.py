"""ctk_std_field_* (contrack_amd/csrc/ctk_std.hip) on the GPU against its statement tests/std_util.want_std -- the two-pass float64 loop
in time order that np.nanstd / np.std confirm on planes of two or more points (tests/test_std_field_host.py) -- bit for bit: every
comparison is np.array_equal(got, want, equal_nan=True), float32 and float64, no tolerance; std, mean and count are all compared.
Every assertion names its case."""
import importlib

import numpy as np
import pytest

import pctl_util
import std_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
STAGE = 64                                               # CTK_STD_STAGE: timesteps k_std_field stages per round


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def _same(got, ref, case):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = np.argwhere(~((got == ref) | ((got != got) & (ref != ref))))
    first = [tuple(b) for b in bad[:4].tolist()]
    assert np.array_equal(got, ref, equal_nan=got.dtype.kind == "f"), (case, len(bad), "at", first, "got", [got[b] for b in first], "want", [ref[b] for b in first])


def _check(trk, x, rows, group, G, W, case, ddofs=(0, 1), skipnas=(True, False), tile=None):
    """std, mean and count of every (ddof, skipna) against the statement; the plain call (no mean, no count) gives the same std"""
    got = None
    for skipna in skipnas:
        q, m, n = std_util.moments(x, rows, group, G, W, skipna)
        for ddof in ddofs:
            got = trk.std_field(x, rows[0], rows[1], group, G, window=W, ddof=ddof, skipna=skipna, want_mean=True, want_n=True)
            c = case + ("skipna", skipna, "ddof", ddof)
            _same(got[0], std_util.finish(q, n, ddof), c + ("std",))
            _same(got[1], m, c + ("mean",))
            _same(got[2], n, c + ("n",))
            if tile is not None:
                assert trk.debug_std_field_form()[0] == tile, (c, "tile", trk.debug_std_field_form())
        _same(trk.std_field(x, rows[0], rows[1], group, G, window=W, ddof=ddofs[-1], skipna=skipna), got[0], case + ("skipna", skipna, "std alone"))
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", pctl_util.KINDS)
def test_edge_kinds(trk, kind, dtype):
    """every kind x G x W x ddof x skipna; bands of 1, tile - 1, tile, tile + 1 and 67 pixels and of several rows, at row 0, inside the
    grid (y0 * nx odd: the band's base is no multiple of a vector) and ending at ny; the rows outside the band hold values that would
    change every answer; group ids cyclic, non-monotone (years concatenated), with groups that own no timestep, shuffled"""
    rng = np.random.default_rng(500 + pctl_util.KINDS.index(kind) * 2 + (dtype == np.float64))
    n = 0
    for G in pctl_util.GS:
        T = max(2 * G + 5, 40)
        for wi, W in enumerate(pctl_util.windows_for(G)):
            rule = ("cyclic", "years", "gaps", "shuffled")[(n + wi) % 4]
            group = pctl_util.groups_for(rule, T, G, rng)
            tile = _native.debug_std_field_plan(G, W, True)["tile"]              # 32 pixels; 16 for G = 366 under a window below it
            assert tile == _native.debug_std_field_plan(G, W, False)["tile"] == (16 if G == 366 and W < G else 32), (G, W, tile)
            shapes = [((3, 1), (1, 2)), ((3, tile - 1), (1, 2)), ((3, tile), (2, 3)), ((3, tile + 1), (0, 1)), ((3, 67), (1, 2)), ((5, 13), (1, 4)),
                      ((2, tile + 1), (1, 2))]
            (ny, nx), rows = shapes[(n + wi) % len(shapes)]
            x = pctl_util.poison_outside(pctl_util.edge_slab(kind, rng, T, ny, nx, dtype, group), rows, rng)
            _check(trk, x, rows, group, G, W, (kind, dtype.__name__, "G", G, "W", W, rule, (ny, nx), rows), tile=tile)
        n += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_time_order_decides_the_bits(trk, dtype):
    """per pixel one value of 1e16 among values of 1.0, at a different timestep for every pixel: every 1.0 added after it is rounded
    away, every one before it counts, so the sum (hence mean and std) tells in which order the pool was added -- a window of 3 groups
    interleaves the timesteps of three groups.  The slab reversed in time has its own, different, answer."""
    T, G, W, nx = 61, 6, 3, 45
    x = np.ones((T, 2, nx), dtype=dtype)
    for p in range(2 * nx):
        x[(7 * p) % T, p // nx, p % nx] = 1e16
    group = (np.arange(T) % G).astype(np.int32)
    fwd = _check(trk, x, (0, 2), group, G, W, ("order", dtype.__name__, "forward"))
    rev = _check(trk, np.ascontiguousarray(x[::-1]), (0, 2), np.ascontiguousarray(group[::-1]), G, W, ("order", dtype.__name__, "reversed"))
    assert not np.array_equal(fwd[1], rev[1]) and not np.array_equal(fwd[0], rev[0]), "the reversed slab must have another answer"
    # adding per member group and merging gives other bits than time order: the case can tell the two apart
    merged = np.stack([sum(x[group == m].astype(np.float64).sum(axis=0) for m in pctl_util.window_members(g, G, W)) for g in range(G)])
    assert not np.array_equal(merged / fwd[2], fwd[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_pool_edges(trk, dtype):
    rng = np.random.default_rng(7)
    for G, W in ((1, 1), (3, 2), (12, 31)):              # T = 1
        x = pctl_util.edge_slab("normal_nan", rng, 1, 5, 9, dtype, np.zeros(1, int))
        for gid in (0, G - 1):
            _check(trk, x, (1, 4), np.array([gid], dtype=np.int32), G, W, ("T=1", dtype.__name__, G, W, gid), ddofs=(0, 1, 2))
    # pools of n = ddof and n = ddof + 1 values side by side (groups of 1 and 2 steps, one that owns none), ddof 0, 1, 2
    x = (10.0 * rng.standard_normal((3, 2, 5))).astype(dtype)
    got = _check(trk, x, (0, 2), np.array([0, 1, 1], dtype=np.int32), 3, 1, ("n around ddof", dtype.__name__), ddofs=(0, 1, 2))
    assert np.isnan(got[0]).all() and not np.isnan(got[1][:2]).any() and np.isnan(got[1][2]).all() and got[2][:, 0, 0].tolist() == [1, 2, 0]
    # all-NaN pixels next to full ones; a pixel whose only values sit in one group
    x = (10.0 * rng.standard_normal((30, 3, 40))).astype(dtype)
    x[:, 1, ::3] = np.nan
    x[::2, 1, 1] = np.nan
    x[np.arange(30) % 5 != 2, 1, 4] = np.nan
    for W in (1, 3, 5):
        _check(trk, x, (1, 2), (np.arange(30) % 5).astype(np.int32), 5, W, ("nan pixels", dtype.__name__, W))
    # a group that owns no timestep: alone it is empty (NaN), under a window it takes its neighbours' steps
    group = np.array([0, 2, 3, 0, 2, 3, 0, 2], dtype=np.int32)
    x = (10.0 * rng.standard_normal((8, 2, 33))).astype(dtype)
    got = _check(trk, x, (0, 2), group, 4, 1, ("empty group", dtype.__name__, 1))
    assert np.isnan(got[0][1]).all() and np.isnan(got[1][1]).all() and not got[2][1].any()
    got = _check(trk, x, (0, 2), group, 4, 2, ("empty group", dtype.__name__, 2))
    assert not np.isnan(got[0][1]).any()
    # window >= G: one plane, replicated (std, mean and count alike)
    x = pctl_util.poison_outside(pctl_util.edge_slab("normal_nan", rng, 50, 4, 37, dtype, np.zeros(50, int)), (1, 3), rng)
    group = pctl_util.groups_for("shuffled", 50, 7, rng)
    for W in (7, 8, 30):
        got = _check(trk, x, (1, 3), group, 7, W, ("replicate", dtype.__name__, W), tile=32)
        for part in got:
            for g in (1, 3, 6):
                assert np.array_equal(part[g], part[0], equal_nan=part.dtype.kind == "f"), ("replicate: plane against plane 0", dtype.__name__, W, g)
    # a single 1 x 1 band: the statement, which numpy's pairwise sum of a one-point plane does not follow
    x = (1e3 + 50.0 * rng.standard_normal((400, 3, 3))).astype(dtype)
    _check(trk, x, (1, 2), np.zeros(400, np.int32), 1, 1, ("1 x 1 band of a 3 x 3 grid", dtype.__name__))
    _check(trk, np.ascontiguousarray(x[:, 1:2, 1:2]), (0, 1), np.zeros(400, np.int32), 1, 1, ("1 x 1 grid", dtype.__name__))


@pytest.mark.parametrize("skipna", [True, False], ids=["skipna", "plain"])
def test_capacity(trk, skipna):
    """the last group count of every pixel tile and the first of the next; the largest ngroups of the plan runs and matches, one more
    is refused before anything is launched; 366 calendar days with a window of 31"""
    rng = np.random.default_rng(19)
    last = {tile: std_util.planes_max(tile, skipna) for tile in (32, 16, 8)}
    assert _native.debug_std_field_plan(last[8], 3, skipna)["max_groups"] == last[8]
    for G, tile in ((last[32], 32), (last[32] + 1, 16), (last[16], 16), (last[16] + 1, 8), (last[8], 8), (366, 16)):
        assert _native.debug_std_field_plan(G, 3, skipna)["tile"] == tile, (G, skipna)
        T, W = 2 * G + 5, 31 if G == 366 else 3
        x = (30.0 * rng.standard_normal((T, 3, 2 * tile + 3))).astype(np.float32)
        x[rng.random(x.shape) < 0.02] = np.nan
        x = pctl_util.poison_outside(x, (1, 2), rng)
        group = pctl_util.groups_for("years", T, G, rng)
        _check(trk, x, (1, 2), group, G, W, ("capacity", G, skipna), ddofs=(1,), skipnas=(skipna,), tile=tile)
        steps = np.bincount(group, minlength=G)
        assert trk.debug_std_field_form() == (tile, max(int(steps[pctl_util.window_members(g, G, W)].sum()) for g in range(G))), (G, skipna)
    G = last[8] + 1
    T = 2 * G + 5
    before = trk.debug_std_field_form()
    x = np.zeros((T, 1, 9), np.float32)
    with pytest.raises(ValueError, match="at most %d groups" % last[8]):
        trk.std_field(x, 0, 1, (np.arange(T) % G).astype(np.int32), G, window=3, skipna=skipna)
    assert trk.debug_std_field_form() == before, "a refused call launches nothing"
    _check(trk, x + 1.5, (0, 1), (np.arange(T) % G).astype(np.int32), G, G, ("beyond the capacity, one plane", G, skipna), ddofs=(0,), skipnas=(skipna,), tile=32)


def test_window_against_owners(trk):
    """a pixel has 512 / tile owning threads: a window of at most that many groups gives a thread one own plane per step (and plane
    `owner` beyond the wrap), a wider one several -- two code paths; the last window of the first, the first of the second and the
    widest window below the group count, for every tile; years concatenated, so that windows wrap past the last group"""
    rng = np.random.default_rng(29)
    for G, tile in ((100, 32), (366, 16), (620, 8)):               # (the tile of either mode: skipna or not)
        owners = 512 // tile
        T = 2 * G + 5
        x = (30.0 * rng.standard_normal((T, 3, tile + 1))).astype(np.float32)
        x[rng.random(x.shape) < 0.02] = np.nan
        x = pctl_util.poison_outside(x, (1, 2), rng)
        for wi, W in enumerate((owners - 1, owners, owners + 1, 2 * owners + 1, G - 1)):
            rule = ("years", "shuffled")[wi % 2]
            group = pctl_util.groups_for(rule, T, G, rng)
            _check(trk, x, (1, 2), group, G, W, ("owners", G, W, rule), ddofs=(1,), tile=tile)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_staging_rounds(trk, dtype):
    """T one less than, equal to and one more than two staged rounds, and one round exactly: the round boundary falls inside every pool"""
    rng = np.random.default_rng(23)
    for T in (STAGE - 1, STAGE, STAGE + 1, 2 * STAGE - 1, 2 * STAGE, 2 * STAGE + 1):
        for G, W, nx in ((5, 3, 35), (1, 1, 9), (40, 31, 17)):
            x = pctl_util.poison_outside(pctl_util.edge_slab("normal_nan", rng, T, 3, nx, dtype, np.zeros(T, int)), (1, 2), rng)
            group = pctl_util.groups_for("cyclic", T, G, rng)
            _check(trk, x, (1, 2), group, G, W, ("staging", dtype.__name__, T, G, W), ddofs=(1,))
            assert trk.debug_std_field_form()[1] == max(int(np.bincount(group, minlength=G)[pctl_util.window_members(g, G, W)].sum()) for g in range(G))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_resident_slab(trk, dtype):
    rng = np.random.default_rng(3)
    T, ny, nx, G = 120, 9, 21, 12
    x = (5500.0 + 50.0 * rng.standard_normal((T, ny, nx))).astype(dtype)
    group = (np.arange(T) % G).astype(np.int32)
    anom, _ = trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=True)
    for W, ddof in ((1, 0), (5, 1), (G + 5, 0)):
        got = trk.std_field(None, 2, 7, group, G, window=W, ddof=ddof, want_mean=True, want_n=True)
        want = std_util.want_std(anom, (2, 7), group, G, W, ddof, True)
        host = trk.std_field(anom, 2, 7, group, G, window=W, ddof=ddof, want_mean=True, want_n=True)
        for part, a, b, c in zip(("std", "mean", "n"), got, want, host):
            _same(a, b, ("resident", dtype.__name__, W, ddof, part))
            _same(c, a, ("host array against resident", dtype.__name__, W, ddof, part))
    trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=False)
    with pytest.raises(_native.ContrackHipError):
        trk.std_field(None, 2, 7, group, G)


def test_library_refuses_bad_arguments(trk):
    x = np.zeros((6, 4, 5), np.float32)
    g = np.zeros(6, np.int32)
    for kw in (dict(y0=-1), dict(y1=5), dict(y0=3, y1=3), dict(window=0), dict(ddof=-1), dict(ngroups=0), dict(group=np.full(6, 2, np.int32)),
               dict(group=np.full(6, -1, np.int32))):
        a = dict(y0=0, y1=4, group=g, ngroups=2, ddof=0, window=1)
        a.update(kw)
        with pytest.raises(ValueError):                  # CTK_E_INVALID
            trk.std_field(x, a["y0"], a["y1"], a["group"], a["ngroups"], window=a["window"], ddof=a["ddof"])


def test_array_level_twin_and_timing_hook(trk):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((90, 8, 30))
    x[rng.random(x.shape) < 0.05] = np.nan
    group = np.arange(90) % 12
    _same(cm.std_field_numpy(x, (2, 6), group, window=3, ddof=1), std_util.want_std(x, (2, 6), group, 12, 3, 1, True)[0], "float64, groups")
    _same(cm.std_field_numpy(x, (2, 6), group, window=3, skipna=False), std_util.want_std(x, (2, 6), group, 12, 3, 0, False)[0], "float64, groups, plain")
    x32 = x.astype(np.float32)
    _same(cm.std_field_numpy(x32, (0, 8), None), std_util.want_std(x32, (0, 8), np.zeros(90, int), 1, 1, 0, True)[0], "float32, one group")
    for arr in (x, x32):
        d = trk.malloc(arr.nbytes)
        try:
            trk.h2d(d, arr)
            field, ms, tile = trk.time_std_field(d, 90, 8, 30, 2, 6, group, 12, window=3, ddof=1, reps=1, f64=arr.dtype == np.float64)
        finally:
            trk.free(d)
        assert ms > 0 and tile == 32, (ms, tile)
        _same(field, std_util.want_std(arr, (2, 6), group, 12, 3, 1, True)[0], ("timing hook", arr.dtype.name))
