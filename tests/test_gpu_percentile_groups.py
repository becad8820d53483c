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


class _Sweeps:
    """band reads of one call, as the library's plan states them (ctk_debug_percentile_groups_plan): whatever the band, G and W are"""

    def __getitem__(self, dtype):
        return _native.debug_percentile_groups_plan(8 * np.dtype(dtype).itemsize, 1000, 12, 3)["sweeps"]


SWEEPS = _Sweeps()


def test_plan_sweeps():
    """11/11/10 (11/11/11/11/10/10) bits and the closing sweep"""
    assert SWEEPS[np.float32] == 4 and SWEEPS[np.float64] == 7
    for nband, G, W in ((1, 1, 1), (16385, 366, 31), (10 ** 6, 12, 17)):
        assert _native.debug_percentile_groups_plan(32, nband, G, W)["sweeps"] == 4
        assert _native.debug_percentile_groups_plan(64, nband, G, W)["sweeps"] == 7


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


def _check_state(trk, x, rows, group, G, W, q, case, model=None):
    """_check, then the device's intermediate values of that call (ctk_debug_percentile_groups_state) against the model's: the pool
    sizes, which groups the closing sweep serves, the distinct selected keys per day"""
    m = pctl_util.selection_model(x, rows, group, G, W, q) if model is None else model
    _check(trk, x, rows, group, G, W, q, case)
    nu, need, n = trk.debug_percentile_groups_state(G)
    assert np.array_equal(n, m["n"]), (case, "n_of", np.nonzero(n != m["n"])[0][:5].tolist())
    assert np.array_equal(need, m["need"]), (case, "need", np.nonzero(need != m["need"])[0][:5].tolist(), int(need.sum()), int(m["need"].sum()))
    assert np.array_equal(nu, m["nu"][-1]), (case, "nu_day", np.nonzero(nu != m["nu"][-1])[0][:5].tolist())
    return m


def _swept_nu(m):
    """the most distinct prefixes of a day at any level whose list a sweep searches (the list of level l serves the sweep of level
    l + 1: all but the last, which serves the closing sweep)"""
    return max(int(a.max()) for a in m["nu"][:-1])


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


# ---- the band stream (pctl_stream) off aligned bases ------------------------------------------------------------------------------
# A lane's unrolled trip takes vectors i, i + 256, i + 512, i + 768: 768 vectors is the last length without one, at 769 lane 0 alone
# takes one.  float32: 4 values a vector, float64: 2.  The band sits in a plane of an odd number of values (pctl_util.odd_plane_for),
# so its first element takes every residue of 16 bytes over consecutive timesteps (the slab is uploaded to an allocation of the
# device's own alignment): heads of 0 .. 3 (0 .. 1) values, tails of 0 .. 3 (0 .. 1), both with and without the unrolled trip.
STREAM_NBAND = {np.float32: [1, 3, 4, 5, 3071, 3072, 3073, 3076, 3077, 4096, 4099], np.float64: [1, 2, 3, 1535, 1536, 1537, 1538, 1539, 2048, 2049]}
STREAM = [(d, n) for d in DTYPES for n in STREAM_NBAND[d]]
UNROLLED = {np.float32: {3076, 3077, 4096, 4099}, np.float64: {1538, 1539, 2048, 2049}}            # some timestep takes the unrolled trip ...
UNROLLED_OFF_ALIGNED = {np.float32: {3077, 4096, 4099}, np.float64: {1539, 2048, 2049}}             # ... one with a misaligned head does


def _band_slab(rng, T, nband, dtype):
    (ny, nx), rows = pctl_util.odd_plane_for(nband)
    x = (50.0 * rng.standard_normal((T, ny, nx))).astype(dtype)
    x[rng.random(x.shape) < 0.03] = np.nan
    per16 = 16 // np.dtype(dtype).itemsize
    residues = {(t * ny * nx + rows[0] * nx) % per16 for t in range(T)}
    assert residues == set(range(per16)), ("the band does not take every alignment", nband, residues)
    return pctl_util.poison_outside(np.ascontiguousarray(x), rows, rng), rows, per16


@pytest.mark.parametrize("dtype, nband", STREAM, ids=["%s-%d" % (d.__name__, n) for d, n in STREAM])
def test_stream_edges_one_chunk(trk, dtype, nband):
    rng = np.random.default_rng(nband)
    T, G, W = 9, 3, 2
    x, rows, per16 = _band_slab(rng, T, nband, dtype)
    assert np.isnan(x[:, rows[0]:rows[1]]).any() or nband < 8
    group = pctl_util.groups_for("cyclic", T, G, rng)
    # vectors behind a head of h values: the unrolled trip is entered above 768 of them
    unrolled = {h for h in range(per16) if (nband - min(h, nband)) // per16 > 768}
    assert bool(unrolled) == (nband in UNROLLED[dtype]) and bool(unrolled - {0}) == (nband in UNROLLED_OFF_ALIGNED[dtype]), (nband, unrolled)
    for q in (0.1, 0.5):
        m = _check_state(trk, x, rows, group, G, W, q, ("stream", dtype.__name__, nband, q))
        assert int(m["n"].min()) > 0 or nband < 8


CHUNKED = [(d, n) for d in DTYPES for n in (16383, 16384, 16385, 32769, 16384 + 3077)]


@pytest.mark.parametrize("dtype, nband", CHUNKED, ids=["%s-%d" % (d.__name__, n) for d, n in CHUNKED])
def test_chunk_edges(trk, dtype, nband):
    """one chunk less a value, one chunk, one chunk and a value, two chunks and a value, a chunk and an unrolled trip with a head and
    a tail; at q = 0.5 every group takes its next key from the closing sweep, which so runs across the chunk boundary"""
    rng = np.random.default_rng(nband)
    T, G, W = 5, 3, 2
    x, rows, _ = _band_slab(rng, T, nband, dtype)
    group = pctl_util.groups_for("cyclic", T, G, rng)
    assert _native.debug_percentile_groups_plan(32, nband, G, W)["chunks"] == {16383: 1, 16384: 1, 16385: 2, 32769: 3, 19461: 2}[nband]
    for q in (0.1, 0.5):
        m = pctl_util.selection_model(x, rows, group, G, W, q)
        if q == 0.5:
            assert int(m["need"].sum()) == G, ("the closing sweep would not run for every group", m["need"].tolist())
        _check_state(trk, x, rows, group, G, W, q, ("chunks", dtype.__name__, nband, q), m)


# ---- the histograms a sweep workgroup keeps in LDS (CTK_PCTL_LDS_SLOTS = 4) and the fifth, in HBM ------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("W, most", [(4, 4), (5, 5)], ids=["W4_all_lds", "W5_fifth_hbm"])
def test_lds_slot_edge(trk, W, most, dtype):
    """every group a power of two of its own: the targets of a day select under as many distinct prefixes as the window has groups"""
    rng = np.random.default_rng(40 + W)
    T, G = 29, 12
    group = pctl_util.groups_for("cyclic", T, G, rng)
    x = np.empty((T, 3, 20), dtype)
    x[:] = (2.0 ** group * (1.0 + 0.01 * rng.random((20, 3, T)))).T.astype(dtype)
    x = pctl_util.poison_outside(np.ascontiguousarray(x), (1, 2), rng)
    m = pctl_util.selection_model(x, (1, 2), group, G, W, 0.5)
    assert _swept_nu(m) == most == pctl_util.PCTL_LDS_SLOTS + (W - 4), [int(a.max()) for a in m["nu"]]
    assert int(m["nu"][1].max()) == most                                           # (so the second digit's sweep already sees them)
    _check_state(trk, x, (1, 2), group, G, W, 0.5, ("lds slots", dtype.__name__, W), m)


@pytest.mark.parametrize("q", [0.1, 0.5, 0.9])
def test_hbm_slots_float32(trk, q):
    """the float32 twin of test_large_pool's float64 case of G = 12, W = 7: six scales, so the seven targets of a day select under
    more prefixes than LDS holds, and every group takes its next key from the closing sweep"""
    rng = np.random.default_rng(77)
    T, G, W = 65, 12, 7
    group = pctl_util.groups_for("cyclic", T, G, rng)
    x = (rng.standard_normal((T, 3, 67)) * (4.0 ** (group % 6))[:, None, None]).astype(np.float32)
    x = pctl_util.poison_outside(np.ascontiguousarray(x), (1, 2), rng)
    m = pctl_util.selection_model(x, (1, 2), group, G, W, q)
    assert _swept_nu(m) > pctl_util.PCTL_LDS_SLOTS and int(m["need"].sum()) == G, ([int(a.max()) for a in m["nu"]], m["need"].tolist())
    _check_state(trk, x, (1, 2), group, G, W, q, ("hbm slots f32", q), m)


# ---- windows above 256 groups: the second trip of the 256-lane loops over a day's targets and prefixes ---------------------------------
def _wide(G, W, dtype):
    rng = np.random.default_rng(G + W)
    T = 2 * G + 5
    group = pctl_util.groups_for("years", T, G, rng)
    x = (group[:, None, None] + 0.3 * rng.random((T, 3, 23))).astype(dtype)
    x = pctl_util.poison_outside(np.ascontiguousarray(x), (1, 2), rng)
    t0 = time.perf_counter()
    ref = pctl_util.want(x, (1, 2), group, G, W, 0.5)
    cpu = time.perf_counter() - t0
    assert cpu < 60, ("the numpy yardstick took %.1f s" % cpu, G, W)
    assert not np.isnan(ref).any()
    return x, group, pctl_util.selection_model(x, (1, 2), group, G, W, 0.5)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_window_257_of_300(trk, dtype):
    """257 targets a day: k_pctl_lists and k_pctl_close walk them in two trips of 256 lanes; tens of distinct prefixes a day"""
    G, W = 300, 257
    x, group, m = _wide(G, W, dtype)
    assert W > 256 and W < G and _swept_nu(m) > pctl_util.PCTL_LDS_SLOTS and int(m["need"].sum()) > 0, ([int(a.max()) for a in m["nu"]], int(m["need"].sum()))
    _check_state(trk, x, (1, 2), group, G, W, 0.5, ("window 257 of 300", dtype.__name__), m)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_window_257_of_1024(dtype):
    """257 targets a day that select 257 distinct prefixes: the lists the sweeps and the closing sweep load into LDS take a second
    trip, and their binary searches run over 257 entries.  1024 x 257 histograms of 8 KB (2.1 GB) in the handle's grow-only
    workspace: a handle of its own, closed afterwards"""
    G, W = 1024, 257
    x, group, m = _wide(G, W, dtype)
    assert _swept_nu(m) > 256 and int(m["nu"][-1].max()) > 256 and int(m["need"].sum()) > 0, ([int(a.max()) for a in m["nu"]], int(m["need"].sum()))
    assert _native.debug_percentile_groups_plan(8 * np.dtype(dtype).itemsize, 23, G, W)["refusal"] == "fine"
    with _native.Tracker(0) as own:
        _check_state(own, x, (1, 2), group, G, W, 0.5, ("window 257 of 1024", dtype.__name__), m)


def test_library_refuses_by_size_and_goes_on(trk):
    """the two size rules a small slab can meet, through the entry itself; nothing is allocated for a refused call"""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 4, 5)).astype(np.float32)
    g = np.zeros(6, np.int32)
    for G, W, why in ((1100, 1025, "window"), (1024, 513, "slots")):
        assert _native.debug_percentile_groups_plan(32, 20, G, W, 6)["refusal"] == why
        with pytest.raises(ValueError):
            trk.percentile_groups(x, 0, 4, g, G, 0.5, window=W)
        group = (np.arange(6) % 3).astype(np.int32)
        _check_state(trk, x, (1, 3), group, 3, 2, 0.5, ("after the refusal of", G, W))
    with pytest.raises(ValueError):
        trk.debug_percentile_groups_state(4)                                         # (the last call had 3 groups)
    with _native.Tracker(0) as fresh:
        with pytest.raises(_native.ContrackHipError):
            fresh.debug_percentile_groups_state(3)                                   # no call yet
