"""Threshold fields (ctk_set_threshold_field, k_threshold_field): a threshold that varies by grid point, as the reference accepts
it (contrack.py:648-671).  Exactness rests on this: only the threshold step sees the threshold, so for any field F

    run_contrack(anom, F, op) == run_contrack(ind, 0.5, '>=')   with   ind = (anom <op> F under numpy promotion, NaN -> 0)

and the right-hand side is the scalar path, pinned against every golden.  A constant field at a golden's own thresholds must
reproduce the golden's flag bit for bit."""
import importlib
import operator

import numpy as np
import pytest

import golden_util
import minixr
from contrack_amd import _native, synth

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

NP_OPS = {0: operator.ge, 1: operator.le, 2: operator.gt, 3: operator.lt}


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def indicator(anom, planes, pos, op):
    """numpy's compare of every step with its plane (promotion included; NaN compares false), as float32 0 / 1"""
    out = np.empty(anom.shape, dtype=np.float32)
    for t0 in range(0, anom.shape[0], 64):
        with np.errstate(invalid="ignore"):
            out[t0:t0 + 64] = NP_OPS[op](anom[t0:t0 + 64], planes[pos[t0:t0 + 64]])
    return out


def with_field(trk, planes, pos, fn):
    trk.set_threshold_field(planes, pos)
    try:
        return fn()
    finally:
        trk.clear_threshold_field()


def field_track(trk, anom, planes, pos, op, g, f64=False):
    flag, n = with_field(trk, planes, pos, lambda: trk.track(anom, None, op, g["wrow"], g["overlap"], g["persistence"], g["twosided"], f64=f64))
    return flag.copy(), n


def scalar_on_indicator(trk, ind, g):
    flag, n = trk.track(ind, np.full(ind.shape[0], 0.5), 0, g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    return flag.copy(), n


def smooth_planes(nplanes, ny, nx, center, amp, seed, dtype):
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, np.pi, ny)[None, :, None]
    x = np.linspace(0.0, 2 * np.pi, nx, endpoint=False)[None, None, :]
    ph = rng.uniform(0.0, 2 * np.pi, (nplanes, 3, 1, 1))
    f = center + amp * (np.sin(2 * y + ph[:, 0]) * np.cos(3 * x + ph[:, 1]) + 0.5 * np.cos(x + y + ph[:, 2]))
    return f.astype(dtype)


def djf_pos(T, nplanes):
    """plane of every step of a run of winters (Dec 1 ..): day of year - 1 for 366 planes, weekday-like for 7, 0 for 1"""
    d = np.datetime64("2000-12-01") + (np.arange(T) % 90)
    doy = (d - d.astype("datetime64[Y]")).astype(int)                  # day of year - 1
    return (doy % nplanes).astype(np.int32)


def _params(name):
    g = golden_util.load(name)
    return g, _native.CMP_OPS[g["gorl"]]


# ---- 1. constant fields reproduce every golden -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_util.case_names())
def test_constant_field_reproduces_golden(trk, name):
    g, op = _params(name)
    T, ny, nx = g["anom"].shape
    _, n_scalar = trk.track(g["anom"], g["thr"], op, g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    planes = np.ascontiguousarray(np.broadcast_to(g["thr"][:, None, None], (T, ny, nx)), dtype=np.float64)
    flag, n = field_track(trk, g["anom"], planes, np.arange(T, dtype=np.int32), op, g)
    assert np.array_equal(flag, g["flag"]) and n == n_scalar
    if np.all(g["thr"] == g["thr"][0]):
        flag1, n1 = field_track(trk, g["anom"], planes[:1], np.zeros(T, dtype=np.int32), op, g)
        assert np.array_equal(flag1, g["flag"]) and n1 == n_scalar


# ---- 2. varying fields: the C oracle and the GPU scalar path on the indicator slab --------------------------------------------
@pytest.mark.parametrize("nplanes", [1, 7, 366])
@pytest.mark.parametrize("name, dtype", [("busy_s1", np.float64), ("odd_65x130", np.float32), ("odd_9x65", np.float64), ("nan_speckle", np.float32),
                                         ("syn2deg_le", np.float64), ("refslab_two", np.float32), ("f64pole_syn", np.float64), ("chain_a", np.float32)])
def test_varying_field_equals_oracle_and_scalar_path_on_indicator(trk, oracle_lib, name, dtype, nplanes):
    g, op = _params(name)
    T, ny, nx = g["anom"].shape
    amp = 0.3 * float(np.nanstd(g["anom"]))
    planes = smooth_planes(nplanes, ny, nx, float(g["thr"][0]), amp, seed=nplanes, dtype=dtype)
    pos = djf_pos(T, nplanes)
    flag, n = field_track(trk, g["anom"], planes, pos, op, g)
    ind = indicator(g["anom"], planes, pos, op)
    want, nw = oracle_lib.run_contrack(ind, np.full(T, 0.5), ">=", g["wrow"], g["overlap"], g["persistence"], g["twosided"])
    assert np.array_equal(flag, want) and n == nw
    got_s, ns = scalar_on_indicator(trk, ind, g)
    assert np.array_equal(flag, got_s) and n == ns


# ---- 3. compare semantics, bit by bit -------------------------------------------------------------------------------------
def _edge_values(rng, shape, data_dtype):
    """data and a float64 field around it: equal values, float32 midpoints and +-1 ulp of float64 around them, NaN, +-inf, values
    beyond the float32 range, signed zeros"""
    base = rng.choice(np.array([1.0, -1.0, 0.1, -2.5, 3.0e-39, 0.0, -0.0, 1.0e30, 160.0], dtype=np.float32), size=shape)
    step = rng.integers(-2, 3, size=shape).astype(np.int32)
    a32 = base.copy()
    for k in (1, 2):
        a32 = np.where(step >= k, np.nextafter(a32, np.float32(np.inf)), np.where(step <= -k, np.nextafter(a32, np.float32(-np.inf)), a32))
    b32 = base.astype(np.float64)
    up = np.nextafter(base, np.float32(np.inf)).astype(np.float64)
    mid = (b32 + up) / 2                                                # exactly between two float32 values
    kind = rng.integers(0, 10, size=shape)
    f = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7, kind == 8],
                  [b32, mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf), np.nan, np.inf, -np.inf, 1e300, -1e300], default=b32)
    a = a32.astype(data_dtype)
    if data_dtype == np.float64:                                       # float64 data between float32 values too
        a = np.where(rng.random(shape) < 0.3, mid + rng.integers(-1, 2, size=shape) * np.spacing(mid), a)
    nanm = rng.random(shape) < 0.03
    a[nanm] = np.nan
    a[rng.random(shape) < 0.02] = np.inf
    a[rng.random(shape) < 0.02] = -np.inf
    return a, f


@pytest.mark.parametrize("nx", [64, 65])
@pytest.mark.parametrize("data_dtype, field_dtype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)])
@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_mask_equals_numpy_compare(trk, nx, data_dtype, field_dtype, op):
    rng = np.random.default_rng(100 * op + nx)
    T, ny = 5, 7
    a, f64field = _edge_values(rng, (T, ny, nx), data_dtype)
    planes = f64field.astype(field_dtype) if field_dtype == np.float64 else np.where(np.abs(f64field) > 3e38, np.copysign(np.inf, f64field), f64field).astype(np.float32)
    pos = np.arange(T, dtype=np.int32)
    w = np.ones(ny, dtype=np.float32)
    with_field(trk, planes, pos, lambda: trk.track(a, None, op, w, 0.5, 1, True, f64=data_dtype == np.float64))
    mask = trk.debug_mask(T, ny, nx)
    want = indicator(a, planes, pos, op).astype(np.uint8)
    assert np.array_equal(mask, want)


# ---- 4. shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [9, 65, 360, 1440])
@pytest.mark.parametrize("T", [1, 2, 17])
@pytest.mark.parametrize("full", [True, False])
def test_shapes(trk, nx, T, full):
    ny = 13
    a = synth.smooth_field(T, ny, nx, seed=nx + T)
    lat, _ = synth.grid(ny, nx)
    g = dict(wrow=cm.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx)), overlap=0.5, persistence=1, twosided=True)
    fld = smooth_planes(T if full else 1, ny, nx, 120.0, 60.0, seed=T, dtype=np.float32)
    thr = fld if full else fld[0]                                     # (T, ny, nx) or (ny, nx)
    flag, n = cm.track_numpy(a, g["wrow"], thr, ">=", 0.5, 1)
    ind = indicator(a, np.broadcast_to(thr, a.shape), np.arange(T), 0)
    want, nw = scalar_on_indicator(trk, ind, g)
    assert np.array_equal(flag, want) and n == nw


# ---- 5. every entry gives the same -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field_dtype", [np.float32, np.float64])
def test_entries_agree(field_dtype):
    t = _native.Tracker(0)
    try:
        T, ny, nx = 40, 91, 180
        x = synth.smooth_field(T, ny, nx, seed=7, offset=0.0)
        group = (np.arange(T) % 10).astype(np.int32)
        a, _ = t.anomalies(x, group, 10, keep_resident=True)        # the slab the class's calc_anom leaves in HBM
        lat, _ = synth.grid(ny, nx)
        g = dict(wrow=cm.row_weights(lat, np.float32(2.0), np.float32(2.0)), overlap=0.5, persistence=3, twosided=True)
        planes = smooth_planes(366, ny, nx, 60.0, 40.0, seed=9, dtype=field_dtype)
        pos = djf_pos(T, 366)
        op = 0
        want, nw = scalar_on_indicator(t, indicator(a, planes, pos, op), g)
        args = (op, g["wrow"], g["overlap"], g["persistence"], g["twosided"])
        t.set_threshold_field(planes, pos)
        results = {}
        f, n = t.track(a, None, *args)
        results["host_f32"] = (f.copy(), n)
        f, n = t.track(a.astype(np.float64), None, *args, f64=True)
        results["host_f64"] = (f.copy(), n)
        f, n = t.track_resident(None, *args)
        results["resident"] = (f.copy(), n)
        d_in, d_out = t.malloc(a.nbytes), t.malloc(a.size * 4)
        try:
            t.h2d(d_in, a)
            n = t.track_dev(d_in, T, ny, nx, None, *args, d_out)
            out = np.empty(a.shape, dtype=np.int32)
            t.d2h(out, d_out)
            results["dev"] = (out, n)
        finally:
            t.free(d_in)
            t.free(d_out)
        for chunk in (7, 13):                                          # chunks that cut across plane groups
            f, n = t.track_stream(a, None, *args, chunk_steps=chunk)
            results["stream_%d" % chunk] = (f, n)
        sink = np.zeros(a.shape, dtype=np.int32)

        def writer(t0, nt, flags):
            sink[t0:t0 + nt] = flags

        _, n = t.track_stream(lambda t0, nt, out: out.__setitem__(Ellipsis, a[t0:t0 + nt]), None, *args, sink=writer, shape=a.shape,
                              dtype=np.float32, chunk_steps=11)
        results["stream_cb"] = (sink, n)
        t.clear_threshold_field()
        for k, (f, n) in results.items():
            assert np.array_equal(f, want) and n == nw, k
    finally:
        t.close()


# ---- 6. one handle: scalar -> field A -> scalar -> field B -> field A ----------------------------------------------------------
def test_handle_reuse_and_refusals(trk):
    g, op = _params("syn2deg_s1")
    T, ny, nx = g["anom"].shape
    A = (smooth_planes(366, ny, nx, 160.0, 50.0, seed=1, dtype=np.float64), djf_pos(T, 366))
    B = (smooth_planes(7, ny, nx, 150.0, 30.0, seed=2, dtype=np.float32), djf_pos(T, 7))
    args = (op, g["wrow"], g["overlap"], g["persistence"], g["twosided"])

    def fresh(field):
        t = _native.Tracker(0)
        try:
            if field is None:
                f, n = t.track(g["anom"], g["thr"], *args)
            else:
                t.set_threshold_field(*field)
                f, n = t.track(g["anom"], None, *args)
            return f.copy(), n
        finally:
            t.close()

    want = {k: fresh(v) for k, v in (("s", None), ("A", A), ("B", B))}
    assert np.array_equal(want["s"][0], g["flag"])
    for k in ("s", "A", "s", "B", "A", "s"):
        if k == "s":
            f, n = trk.track(g["anom"], g["thr"], *args)
        else:
            trk.set_threshold_field(*(A if k == "A" else B))
            f, n = trk.track(g["anom"], None, *args)
        assert np.array_equal(f, want[k][0]) and n == want[k][1], k
    trk.clear_threshold_field()
    with pytest.raises(ValueError, match="no threshold field"):
        trk.track(g["anom"], None, *args)
    trk.set_threshold_field(A[0], A[1][:-1])                           # one step short: another shape
    with pytest.raises(ValueError, match="another shape"):
        trk.track(g["anom"], None, *args)
    with pytest.raises(ValueError):
        trk.set_threshold_field(A[0], np.full(T, 366))               # a plane the field does not have
    trk.clear_threshold_field()
    f, n = trk.track(g["anom"], g["thr"], *args)                       # and the scalar path is still fine
    assert np.array_equal(f, g["flag"])


def test_time_shard_entries_refuse_a_field(trk):
    g, op = _params("T3")
    T, ny, nx = g["anom"].shape
    grp = _native.CommGroup(1)
    comm = _native.Comm.local(trk, grp, 0)
    d_in, d_out = trk.malloc(g["anom"].nbytes), trk.malloc(g["anom"].size * 4)
    try:
        trk.h2d(d_in, g["anom"])
        trk.set_threshold_field(np.broadcast_to(g["thr"][:, None, None], (T, ny, nx)), np.arange(T))
        with pytest.raises(ValueError, match="threshold field"):
            trk.track_sharded_dev(comm, d_in, T, 0, T, ny, nx, None, op, g["wrow"], g["overlap"], g["persistence"], g["twosided"], d_out)
        with pytest.raises(ValueError, match="threshold field"):
            trk.shard_label2d(d_in, T, ny, nx, None, op, g["wrow"], False)
    finally:
        trk.clear_threshold_field()
        trk.free(d_in)
        trk.free(d_out)
        comm.close()
        grp.close()


# ---- 7. the class on tests/minixr.py -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 9])
def test_class_dayofyear_field(chunk):
    minixr.install_as_xarray()
    g, _ = _params("syn2deg_s0")
    a = g["anom"]
    T, ny, nx = a.shape
    time = (np.datetime64("2003-12-05") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(a, g["lat"], g["lon"], time=time)
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    tll = smooth_planes(366, ny, nx, 160.0, 40.0, seed=11, dtype=np.float64)            # (dayofyear, lat, lon), the dataset's lat order
    lat = np.asarray(g["lat"])
    thr = minixr.DataArray(np.ascontiguousarray(tll[:, ::-1].transpose(2, 0, 1)), ("longitude", "dayofyear", "latitude"),
                           coords={"dayofyear": minixr.DataArray(np.arange(1, 367), ("dayofyear",)),
                                   "latitude": minixr.DataArray(lat[::-1], ("latitude",)),
                                   "longitude": minixr.DataArray(np.asarray(g["lon"]), ("longitude",))})
    c.run_contrack(variable="anom", threshold=thr, gorl=">=", overlap=g["overlap"], persistence=g["persistence"], twosided=g["twosided"],
                   chunk_steps=chunk)
    import pandas as pd
    doy = np.asarray(pd.DatetimeIndex(time).dayofyear)
    want, nw = cm.track_numpy(a, g["wrow"], tll[doy - 1], ">=", g["overlap"], g["persistence"], g["twosided"])
    assert np.array_equal(np.asarray(c.flag), want)
    short = minixr.DataArray(tll[:300], ("dayofyear", "latitude", "longitude"),
                             coords={"dayofyear": minixr.DataArray(np.arange(1, 301), ("dayofyear",))})
    with pytest.raises(KeyError):
        c.run_contrack(variable="anom", threshold=short, gorl=">=", overlap=0.5, persistence=1)
    with pytest.raises(ValueError):
        c.run_contrack(variable="anom", threshold=minixr.DataArray(tll[0], ("latitude", "longitude")), gorl=">=", overlap=0.5, persistence=1)


# ---- 8. full size -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, ny, nx, field_dtype, pers", [(2707, 181, 360, np.float32, 5), (480, 721, 1440, np.float64, 20)])
def test_full_size(T, ny, nx, field_dtype, pers):
    t = _native.Tracker(0)
    d_in = d_ind = d_f = d_s = None
    try:
        nb = T * ny * nx * 4
        d_in, d_ind, d_f, d_s = t.malloc(nb), t.malloc(nb), t.malloc(nb), t.malloc(nb)
        t.synth_fill(d_in, T, ny, nx, seed=0)
        a = np.empty((T, ny, nx), dtype=np.float32)
        t.d2h(a, d_in)
        lat, _ = synth.grid(ny, nx)
        w = cm.row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
        planes = smooth_planes(366, ny, nx, 160.0, 40.0, seed=3, dtype=field_dtype)
        pos = djf_pos(T, 366)
        ind = indicator(a, planes, pos, 0)
        t.h2d(d_ind, ind)
        del ind
        n_s = t.track_dev(d_ind, T, ny, nx, np.full(T, 0.5), 0, w, 0.5, pers, True, d_s)
        t.set_threshold_field(planes, pos)
        n_f = t.track_dev(d_in, T, ny, nx, None, 0, w, 0.5, pers, True, d_f)
        t.clear_threshold_field()
        out_f = np.empty((T, ny, nx), dtype=np.int32)
        t.d2h(out_f, d_f)
        out_s = a.view(np.int32)                                       # (the slab's host copy is not needed any more)
        t.d2h(out_s, d_s)
        assert n_f == n_s and n_s > 0
        assert np.array_equal(out_f, out_s)
    finally:
        for d in (d_in, d_ind, d_f, d_s):
            if d is not None:
                t.free(d)
        t.close()
