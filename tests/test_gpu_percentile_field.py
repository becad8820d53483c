"""ctk_percentile_field_* (contrack_amd/csrc/ctk_pfield.hip) on the GPU against the numpy yardstick tests/pfield_util.want_field --
np.nanquantile of every (group, grid point) pool in float64 -- bit for bit: every comparison is np.array_equal(got, want,
equal_nan=True), float32 and float64, no tolerance.  Every assertion names its case."""
import importlib
import time

import numpy as np
import pytest

import minixr
import pctl_util
import pfield_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DIRECT, RING = 0, 1


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def _same(got, ref, case):
    assert got.dtype == np.float64 and got.shape == ref.shape, (case, got.dtype, got.shape, ref.shape)
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    first = [tuple(b) for b in bad[:4].tolist()]
    assert np.array_equal(got, ref, equal_nan=True), (case, len(bad), "at", first, "got", [got[b] for b in first], "want", [ref[b] for b in first])


def _check(trk, x, rows, group, G, W, qs, case, form=None):
    refs = pfield_util.want_field(x, rows, group, G, W, list(qs))
    got = None
    for q, ref in zip(qs, refs):
        got = trk.percentile_field(x, rows[0], rows[1], group, G, q, window=W)
        _same(got, ref, case + ("q", q))
        if form is not None:
            assert trk.debug_percentile_field_form()[0] == form, (case, "form", trk.debug_percentile_field_form())
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", pctl_util.KINDS)
def test_edge_kinds(trk, kind, dtype):
    """every kind x G x W x q; bands of 1, tile - 1, tile, tile + 1 and 67 pixels and one of several rows, at row 0, inside the grid
    (y0 * nx odd: the band's base is no multiple of a vector) and ending at ny; the rows outside the band hold values that would
    change every answer; group ids cyclic, non-monotone (years concatenated), with groups that own no timestep, shuffled"""
    rng = np.random.default_rng(100 + pctl_util.KINDS.index(kind) * 2 + (dtype == np.float64))
    kb = np.dtype(dtype).itemsize
    n = 0
    for G in pctl_util.GS:
        T = max(2 * G + 5, 40)
        for wi, W in enumerate(pctl_util.windows_for(G)):
            rule = ("cyclic", "years", "gaps", "shuffled")[(n + wi) % 4]
            group = pctl_util.groups_for(rule, T, G, rng)
            steps = np.bincount(group, minlength=G)
            longest = max(int(steps[pctl_util.window_members(g, G, W)].sum()) for g in range(G))
            tile = _native.debug_percentile_field_plan(kb, longest, G, W)["tile"]        # 32 pixels, 16 where float64 pools every step of G = 366
            shapes = [((3, 1), (1, 2)), ((3, tile - 1), (1, 2)), ((3, tile), (2, 3)), ((3, tile + 1), (0, 1)), ((3, 67), (1, 2)), ((5, 13), (1, 4)),
                      ((2, tile + 1), (1, 2))]
            (ny, nx), rows = shapes[(n + wi) % len(shapes)]
            x = pctl_util.poison_outside(pctl_util.edge_slab(kind, rng, T, ny, nx, dtype, group), rows, rng)
            _check(trk, x, rows, group, G, W, pctl_util.QS, (kind, dtype.__name__, "G", G, "W", W, rule, (ny, nx), rows), form=RING)
        n += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_pool_edges(trk, dtype):
    rng = np.random.default_rng(7)
    for G, W in ((1, 1), (3, 2), (12, 31)):              # T = 1
        x = pctl_util.edge_slab("normal_nan", rng, 1, 5, 9, dtype, np.zeros(1, int))
        for gid in (0, G - 1):
            _check(trk, x, (1, 4), np.array([gid], dtype=np.int32), G, W, pctl_util.QS, ("T=1", dtype.__name__, G, W, gid))
    _check(trk, np.array([[[3.5]]], dtype=dtype), (0, 1), np.zeros(1, np.int32), 1, 1, [0.5], ("one value", dtype.__name__))
    # all-NaN pixels next to full ones; a pixel whose only values sit in one group
    x = (10.0 * rng.standard_normal((30, 3, 40))).astype(dtype)
    x[:, 1, ::3] = np.nan
    x[::2, 1, 1] = np.nan
    x[np.arange(30) % 5 != 2, 1, 4] = np.nan
    for W in (1, 3, 5):
        _check(trk, x, (1, 2), (np.arange(30) % 5).astype(np.int32), 5, W, pctl_util.QS, ("nan pixels", dtype.__name__, W))
    # two-value pools side by side, one per pixel
    pools = [[1.0, np.inf], [np.inf, np.inf], [-np.inf, 1.0], [-np.inf, np.inf], [np.nan, np.nan], [0.0, -0.0], [-0.0, 0.0], [np.nan, 2.0]]
    x = np.array(pools, dtype=dtype).T.reshape(2, 1, len(pools))
    _check(trk, x, (0, 1), np.zeros(2, np.int32), 1, 1, pctl_util.QS, ("two-value pools", dtype.__name__))
    # keys that differ in their last digit(s) only: the last 8 bits (float32), the last 24 bits (float64)
    T, G = 90, 3
    if dtype == np.float32:
        x = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, (T, 2, 45)).astype(np.uint32)).view(np.float32)
    else:
        x = (np.float64(1.0).view(np.uint64) + rng.integers(0, 1 << 24, (T, 2, 45)).astype(np.uint64)).view(np.float64)
    for W in (1, 2):
        _check(trk, np.ascontiguousarray(x), (0, 2), (np.arange(T) % G).astype(np.int32), G, W, pctl_util.QS, ("low digits only", dtype.__name__, W))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_form_edges(trk, dtype):
    """G = 2, W = 1 on a band of 1 x 20 pixels: a group of exactly `cap` timesteps takes the ring form (8 pixels per workgroup), one
    more the direct form; pools between the tiles' rings take 16 pixels per workgroup"""
    rng = np.random.default_rng(11)
    kb = np.dtype(dtype).itemsize
    cap = _native.debug_percentile_field_plan(kb, 1, 2, 1)["cap"]
    ring32 = _native.debug_percentile_field_plan(kb, 1, 2, 1)["ring_bytes"] // (32 * kb)
    for steps, form, tile in ((cap, RING, 8), (cap + 1, DIRECT, 64), (ring32, RING, 32), (ring32 + 1, RING, 16)):
        plan = _native.debug_percentile_field_plan(kb, steps, 2, 1)
        assert (plan["form"], plan["tile"]) == (form, tile), (dtype.__name__, steps, plan)
        T = steps + 5
        group = np.zeros(T, np.int32)
        group[rng.choice(T, 5, replace=False)] = 1
        x = (40.0 * rng.standard_normal((T, 3, 20))).astype(dtype)
        x[rng.random(x.shape) < 0.01] = np.nan
        x = pctl_util.poison_outside(x, (1, 2), rng)
        _check(trk, x, (1, 2), group, 2, 1, [0.1, 0.5], ("form edge", dtype.__name__, steps), form=form)
        assert trk.debug_percentile_field_form() == (form, steps), (dtype.__name__, steps, trk.debug_percentile_field_form())
    # the direct form with a window that covers every group: one plane of cap + 1 steps, then k_pfield_replicate
    T = cap + 1
    group = (rng.integers(0, 3, T)).astype(np.int32)
    x = (40.0 * rng.standard_normal((T, 3, 20))).astype(dtype)
    x[rng.random(x.shape) < 0.01] = np.nan
    x = pctl_util.poison_outside(x, (1, 2), rng)
    for W in (3, 4):
        got = _check(trk, x, (1, 2), group, 3, W, [0.9], ("direct, replicated", dtype.__name__, W), form=DIRECT)
        assert trk.debug_percentile_field_form() == (DIRECT, T), (dtype.__name__, W, trk.debug_percentile_field_form())
        for g in (1, 2):
            assert np.array_equal(got[g], got[0], equal_nan=True), ("direct, replicated: plane against plane 0", dtype.__name__, W, g)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_ring_wraps_and_replicate(trk, dtype):
    rng = np.random.default_rng(13)
    G = 366
    T = 2 * G + 5
    x = pctl_util.poison_outside(pctl_util.edge_slab("normal_nan", rng, T, 4, 37, dtype, np.zeros(T, int)), (1, 3), rng)
    group = pctl_util.groups_for("years", T, G, rng)
    _check(trk, x, (1, 3), group, G, 31, [0.1, 0.9], ("G366 W31", dtype.__name__), form=RING)      # list positions T .. 2 T: the ring of 991 / 495 steps wraps once / twice
    for W in (G, G + 5, 3 * G):                          # every group has the same pool: one plane, replicated
        got = _check(trk, x, (1, 3), group, G, W, [0.5], ("replicate", dtype.__name__, W), form=RING)
        for g in (1, G // 2, G - 1):
            assert np.array_equal(got[g], got[0], equal_nan=True), ("replicate: plane against plane 0", dtype.__name__, W, g)
    _check(trk, x[:40], (1, 3), np.zeros(40, np.int32), 1, 1, [0.1], ("G1", dtype.__name__), form=RING)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_both_forms_give_the_same_field(trk, dtype):
    """the timing hook runs the form the plan chooses and the direct form forced on one slab in device memory"""
    rng = np.random.default_rng(17)
    T, ny, nx, G, W = 150, 5, 45, 12, 5
    x = pctl_util.edge_slab("mixed_inf", rng, T, ny, nx, dtype, np.zeros(T, int))
    group = pctl_util.groups_for("shuffled", T, G, rng)
    d = trk.malloc(x.nbytes)
    try:
        trk.h2d(d, x)
        ring, direct, ms_ring, ms_direct, ms_read, form = trk.time_percentile_field(d, T, ny, nx, 1, 4, group, G, 0.1, window=W, reps=1, f64=dtype == np.float64)
    finally:
        trk.free(d)
    assert form == RING and ms_ring > 0 and ms_direct > 0 and ms_read > 0, (form, ms_ring, ms_direct, ms_read)
    _same(ring, direct, ("ring against direct", dtype.__name__))
    _same(ring, pfield_util.want_field(x, (1, 4), group, G, W, 0.1), ("ring against numpy", dtype.__name__))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_resident_slab(trk, dtype):
    rng = np.random.default_rng(3)
    T, ny, nx, G = 120, 9, 21, 12
    x = (5500.0 + 50.0 * rng.standard_normal((T, ny, nx))).astype(dtype)
    group = (np.arange(T) % G).astype(np.int32)
    anom, _ = trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=True)
    for W, q in ((1, 0.1), (5, 0.9), (G + 5, 0.5)):
        got = trk.percentile_field(None, 2, 7, group, G, q, window=W)
        _same(got, pfield_util.want_field(anom, (2, 7), group, G, W, q), ("resident", dtype.__name__, W, q))
        _same(trk.percentile_field(anom, 2, 7, group, G, q, window=W), got, ("host array against resident", dtype.__name__, W, q))
    trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=False)
    with pytest.raises(_native.ContrackHipError):
        trk.percentile_field(None, 2, 7, group, G, 0.5)


def test_library_refuses_bad_arguments(trk):
    x = np.zeros((6, 4, 5), np.float32)
    g = np.zeros(6, np.int32)
    for kw in (dict(y0=-1), dict(y1=5), dict(y0=3, y1=3), dict(window=0), dict(q=1.5), dict(q=-0.1), dict(ngroups=0), dict(group=np.full(6, 2, np.int32)),
               dict(group=np.full(6, -1, np.int32))):
        a = dict(y0=0, y1=4, group=g, ngroups=2, q=0.5, window=1)
        a.update(kw)
        with pytest.raises(ValueError):                  # CTK_E_INVALID
            trk.percentile_field(x, a["y0"], a["y1"], a["group"], a["ngroups"], a["q"], window=a["window"])


def test_array_level_twin(trk):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((90, 8, 30))
    group = np.arange(90) % 12
    _same(cm.percentile_field_numpy(x, (2, 6), group, 0.1, window=3), pfield_util.want_field(x, (2, 6), group, 12, 3, 0.1), "float64, groups")
    x32 = x.astype(np.float32)
    _same(cm.percentile_field_numpy(x32, (0, 8), None, 0.9), pfield_util.want_field(x32, (0, 8), np.zeros(90, int), 1, 1, 0.9), "float32, one group")


@pytest.mark.parametrize("resident", [False, True], ids=["host_slab", "after_calc_anom"])
def test_class_dayofyear_field(resident):
    minixr.install_as_xarray()
    rng = np.random.default_rng(21)
    T, ny, nx = 830, 19, 36
    lat = np.linspace(90.0, 0.0, ny).astype(np.float32)
    lon = (np.arange(nx) * 10.0).astype(np.float32)
    stamps = (np.datetime64("2003-11-20") + np.arange(T)).astype("datetime64[ns]")
    import pandas as pd
    doy = np.asarray(pd.DatetimeIndex(stamps).dayofyear)
    season = 8.0 * np.cos(2 * np.pi * doy / 365.25)[:, None, None]
    blobs = np.cumsum(rng.standard_normal((T, ny, nx)), axis=2)
    a = (season + 6.0 * blobs).astype(np.float32)
    ds = minixr.make_dataset(a, lat, lon, time=stamps, var="z" if resident else "anom")
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    if resident:
        c.ds["z"].attrs.update({"units": "m", "long_name": "Z500"})
        c.calc_anom("z", window=5, smooth=2)
        a = np.asarray(c.ds["anom"].data)
    field = c.percentile_field(variable="anom", q=0.1, groupby="dayofyear", window=31, lat_bounds=(30, 90))
    days, ids = np.unique(doy, return_inverse=True)
    assert tuple(field.dims) == ("dayofyear", "latitude", "longitude") and np.array_equal(np.asarray(field["dayofyear"].data), days)
    assert np.array_equal(np.asarray(field["latitude"].data), lat) and np.array_equal(np.asarray(field["longitude"].data), lon)
    got = np.asarray(field.data)
    assert got.shape == (len(days), ny, nx) and len(days) == 366
    assert np.isnan(got[:, 13:]).all(), "rows outside 30-90N are NaN"
    ref = pfield_util.want_field(a, (0, 13), ids, len(days), 31, 0.1)
    _same(got[:, :13], ref, ("class", resident))
    if not resident:
        assert not np.isnan(ref).any()
    c.run_contrack(variable="anom", threshold=field, gorl="<=", overlap=0.5, persistence=3)
    flag = np.array(c.flag)
    whole = np.full((len(days), ny, nx), np.nan)
    whole[:, :13] = ref
    dim = lambda v, n: minixr.DataArray(v, (n,))
    same = minixr.DataArray(whole, ("dayofyear", "latitude", "longitude"),
                            coords={"dayofyear": dim(days, "dayofyear"), "latitude": dim(lat, "latitude"), "longitude": dim(lon, "longitude")})
    c.run_contrack(variable="anom", threshold=same, gorl="<=", overlap=0.5, persistence=3)
    assert np.array_equal(flag, np.asarray(c.flag)), ("flag", resident)
    assert flag.max() > 0, ("nothing was flagged", resident)


def test_larger_case(trk):
    """T = 1500, band 8 x 1440, G = 50, W = 5, float32: 360 workgroups of 32 pixels walk 50 groups with pools of 150 steps.  The yardstick
    must stay a matter of seconds on the CPU at this size (asserted: below 60 s)."""
    T, ny, nx, G, W, q = 1500, 10, 1440, 50, 5, 0.1
    rows = (1, 9)
    rng = np.random.default_rng(5)
    x = (30.0 * rng.standard_normal((T, ny, nx), dtype=np.float32))
    x[5::11, 3, ::7] = np.nan
    x = pctl_util.poison_outside(x, rows, rng)
    group = ((np.arange(T) // 3) % G).astype(np.int32)
    t0 = time.perf_counter()
    ref = pfield_util.want_field(x, rows, group, G, W, q)
    cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = trk.percentile_field(x, rows[0], rows[1], group, G, q, window=W)
    gpu = time.perf_counter() - t0
    print("larger case: yardstick %.1f s, percentile_field %.3f s (upload and download included), form %s" % (cpu, gpu, trk.debug_percentile_field_form()))
    assert cpu < 60, ("the numpy yardstick took %.1f s" % cpu)
    _same(got, ref, "larger case")
    assert trk.debug_percentile_field_form() == (RING, 150)
