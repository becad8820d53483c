"""ctk_percentile_groups_* (contrack_amd/csrc/ctk_pctl.hip) on the GPU against the numpy yardstick tests/pctl_util.want --
np.nanquantile of every group's pool in float64 -- bit for bit: every comparison is np.array_equal(got, want, equal_nan=True),
float32 and float64, no tolerance.  Every assertion names its case."""
import importlib
import time

import numpy as np
import pytest

import minixr
import pctl_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SWEEPS = {np.float32: 4, np.float64: 7}              # 11/11/10 (11/11/11/11/10/10) bits and the closing sweep


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def _check(trk, x, rows, group, G, W, q, case):
    got = trk.percentile_groups(x, rows[0], rows[1], group, G, q, window=W)
    ref = pctl_util.want(x, rows, group, G, W, q)
    assert got.dtype == np.float64 and got.shape == (G,), case
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0]
    assert np.array_equal(got, ref, equal_nan=True), (case, "groups", bad[:5].tolist(), "got", got[bad[:5]].tolist(), "want", ref[bad[:5]].tolist())
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", pctl_util.KINDS)
def test_edge_kinds(trk, kind, dtype):
    """every kind x G x W x q; bands whose width is no multiple of 64 or of the vector width, at row 0, inside and at ny; the rows
    outside the band hold values that would change every answer; group ids cyclic, non-monotone (years concatenated), with groups
    that own no timestep, shuffled"""
    rng = np.random.default_rng(pctl_util.KINDS.index(kind) * 2 + (dtype == np.float64))
    shapes = [((7, 37), (0, 3)), ((6, 19), (2, 5)), ((5, 67), (3, 5)), ((4, 13), (0, 4))]        # (ny, nx), rows: 111, 57, 134, 52 band values
    n = 0
    for G in pctl_util.GS:
        T = max(2 * G + 5, 40)
        for wi, W in enumerate(pctl_util.windows_for(G)):
            (ny, nx), rows = shapes[(n + wi) % len(shapes)]
            rule = ("cyclic", "years", "gaps", "shuffled")[(n + wi) % 4]
            group = pctl_util.groups_for(rule, T, G, rng)
            x = pctl_util.poison_outside(pctl_util.edge_slab(kind, rng, T, ny, nx, dtype, group), rows, rng)
            for q in pctl_util.QS:
                _check(trk, x, rows, group, G, W, q, (kind, dtype.__name__, "G", G, "W", W, "q", q, rule, (ny, nx), rows))
        n += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_single_timestep_and_tiny_pools(trk, dtype):
    rng = np.random.default_rng(7)
    for G, W in ((1, 1), (3, 2), (12, 31)):
        x = pctl_util.edge_slab("normal_nan", rng, 1, 5, 9, dtype, np.zeros(1, int))
        for gid in (0, G - 1):
            for q in pctl_util.QS:
                _check(trk, x, (1, 4), np.array([gid], dtype=np.int32), G, W, q, ("T=1", dtype.__name__, G, W, gid, q))
    one = np.array([[[3.5]]], dtype=dtype)
    _check(trk, one, (0, 1), np.zeros(1, np.int32), 1, 1, 0.5, "one value")
    for pool in ([1.0, np.inf], [np.inf, np.inf], [-np.inf, 1.0], [-np.inf, np.inf], [np.nan, np.nan], [0.0, -0.0]):
        x = np.array(pool, dtype=dtype).reshape(2, 1, 1)
        for q in pctl_util.QS:
            _check(trk, x, (0, 1), np.zeros(2, np.int32), 1, 1, q, ("pool", pool, dtype.__name__, q))


LARGE = [("normal", np.float32), ("16 values", np.float32), ("top 24 key bits shared", np.float32), ("normal", np.float64), ("16 values", np.float64),
         ("top 40 key bits shared", np.float64)]


@pytest.mark.parametrize("what, dtype", LARGE, ids=["%s-%s" % (w.replace(" ", "_"), d.__name__) for w, d in LARGE])
def test_large_pool(trk, what, dtype):
    """3.7e7 band values (T = 400, band 64 x 1440, G = 4): pools far beyond one workgroup's reach.  The float64 case whose keys share
    their top 40 bits has G = 12 and W = 7: only the last three digits tell its values apart, and the seven targets of a day select
    different prefixes there, more than a sweep workgroup keeps histograms for in LDS.  The yardstick must stay a matter of seconds
    on the CPU at this size (asserted: below 60 s per call)."""
    T, ny, nx, G = 400, 66, 1440, 4
    rows = (1, 65)
    rng = np.random.default_rng(len(what))
    if what == "normal":
        x = (30.0 * rng.standard_normal((T, ny, nx), dtype=np.float32)).astype(dtype)
        x[5, 3, ::7] = np.nan
    elif what == "16 values":                            # ties at every digit level
        vals = np.array([-1e9, -7.25, -7.249999, -1e-30, -0.0, 0.0, 1e-30, 0.5, 0.50000006, 1.0, 3.0, 3.0000002, 1e5, 1e5 + 0.0078125, 1e30, np.inf], dtype=dtype)
        x = vals[rng.integers(0, 16, (T, ny, nx))]
    elif dtype == np.float64:                            # float64 keys that differ in their last 24 bits only
        G = 12
        x = (np.float64(1.0).view(np.uint64) + rng.integers(0, 1 << 24, (T, ny, nx)).astype(np.uint64)).view(np.float64)
    else:                                                # float32 keys that differ in their last 8 bits only
        x = (np.float32(1.0).view(np.uint32) + rng.integers(0, 256, (T, ny, nx)).astype(np.uint32)).view(np.float32)
    x = pctl_util.poison_outside(np.ascontiguousarray(x, dtype=dtype), rows, rng)
    group = ((np.arange(T) // 3) % G).astype(np.int32)
    for W in (1, 3) if G == 4 else (7,):
        for q in (0.1, 0.5) if W == 1 else (0.1,):
            t0 = time.perf_counter()
            ref = pctl_util.want(x, rows, group, G, W, q)
            cpu = time.perf_counter() - t0
            got = trk.percentile_groups(x, rows[0], rows[1], group, G, q, window=W)
            print("large pool %s %s W=%d q=%g: yardstick %.1f s" % (what, dtype.__name__, W, q, cpu))
            assert cpu < 60, ("the numpy yardstick took %.1f s" % cpu, what, dtype.__name__, W, q)
            assert np.array_equal(got, ref, equal_nan=True), (what, dtype.__name__, W, q, got.tolist(), ref.tolist())
            assert trk.debug_percentile_groups_sweeps() == SWEEPS[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_resident_slab(trk, dtype):
    rng = np.random.default_rng(3)
    T, ny, nx, G = 120, 9, 21, 12
    x = (5500.0 + 50.0 * rng.standard_normal((T, ny, nx))).astype(dtype)
    group = (np.arange(T) % G).astype(np.int32)
    anom, _ = trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=True)
    for W, q in ((1, 0.1), (5, 0.9), (G + 5, 0.5)):
        got = trk.percentile_groups(None, 2, 7, group, G, q, window=W)
        host = pctl_util.want(anom, (2, 7), group, G, W, q)
        assert np.array_equal(got, host, equal_nan=True), ("resident", dtype.__name__, W, q)
        anom2, _ = trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=True)      # (the host-array call replaced io_in, not the slab)
        assert np.array_equal(trk.percentile_groups(anom, 2, 7, group, G, q, window=W), got, equal_nan=True)
        assert np.array_equal(anom2, anom, equal_nan=True)
    trk.anomalies(x, group, G, window=3, smooth=2, keep_resident=False)
    with pytest.raises(_native.ContrackHipError):
        trk.percentile_groups(None, 2, 7, group, G, 0.5)


def test_library_refuses_bad_arguments(trk):
    x = np.zeros((6, 4, 5), np.float32)
    g = np.zeros(6, np.int32)
    for kw in (dict(y0=-1), dict(y1=5), dict(y0=3, y1=3), dict(window=0), dict(q=1.5), dict(q=-0.1), dict(ngroups=0), dict(group=np.full(6, 2, np.int32)),
               dict(group=np.full(6, -1, np.int32))):
        a = dict(y0=0, y1=4, group=g, ngroups=2, q=0.5, window=1)
        a.update(kw)
        with pytest.raises(ValueError):                  # CTK_E_INVALID
            trk.percentile_groups(x, a["y0"], a["y1"], a["group"], a["ngroups"], a["q"], window=a["window"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_call_budget(trk, dtype):
    """the band is read once per digit and once to close, whatever G and W are"""
    rng = np.random.default_rng(9)
    for G in (1, 12, 366):
        T = 2 * G + 7
        x = rng.standard_normal((T, 6, 33)).astype(dtype)
        group = (np.arange(T) % G).astype(np.int32)
        for W in (1, 31, G + 5):
            trk.percentile_groups(x, 1, 5, group, G, 0.1, window=W)
            assert trk.debug_percentile_groups_sweeps() == SWEEPS[dtype], (dtype.__name__, G, W)


def test_array_level_twin(trk):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((90, 8, 30))
    group = np.arange(90) % 12
    got = cm.percentile_groups_numpy(x, (2, 6), group, 0.1, window=3)
    assert np.array_equal(got, pctl_util.want(x, (2, 6), group, 12, 3, 0.1), equal_nan=True)
    got = cm.percentile_groups_numpy(x.astype(np.float32), (0, 8), None, 0.9)
    assert np.array_equal(got, pctl_util.want(x.astype(np.float32), (0, 8), np.zeros(90, int), 1, 1, 0.9), equal_nan=True)


@pytest.mark.parametrize("resident", [False, True], ids=["host_slab", "after_calc_anom"])
def test_class_dayofyear_threshold(resident):
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
    thr = c.percentile_threshold(variable="anom", q=0.1, lat_bounds=(30, 90), groupby="dayofyear", window=31)
    days, ids = np.unique(doy, return_inverse=True)
    assert tuple(thr.dims) == ("dayofyear",) and np.array_equal(np.asarray(thr["dayofyear"].data), days)
    ref = pctl_util.want(a, (0, 13), ids, len(days), 31, 0.1)
    assert np.array_equal(np.asarray(thr.data), ref, equal_nan=True)
    assert len(days) == 366 and not np.isnan(ref).any()
    c.run_contrack(variable="anom", threshold=thr, gorl="<=", overlap=0.5, persistence=3)
    flag = np.array(c.flag)
    same = minixr.DataArray(ref, ("dayofyear",), coords={"dayofyear": minixr.DataArray(days, ("dayofyear",))})
    c.run_contrack(variable="anom", threshold=same, gorl="<=", overlap=0.5, persistence=3)
    assert np.array_equal(flag, np.asarray(c.flag)) and flag.max() > 0
