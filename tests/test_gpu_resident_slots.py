"""The two slabs that stay in HBM between calls -- the field to track (anomalies / reversal / lwa with keep_resident) and the resident
vertical mean (level_mean / time_filter with keep_resident) -- as every entry family leaves them: one handle walks a table of calls,
and after EVERY call both slots are asked for their shape (or None) and whether their generation changed.  Then the refusals: what
reads a slot raises once it is dropped or holds another shape or type.  Results of a keep / no-keep pair are the same bits."""
import ctypes as C

import numpy as np
import pytest

from contrack_amd import _native
from contrack_amd._native import ContrackHipError, check, lib

import lwa_util
import reversal_util
import subset_util
from level_util import same_bits

pytestmark = pytest.mark.gpu

T, NY, NX, NLEV = 8, 5, 16, 3
LAT = np.linspace(90.0, -90.0, NY)                       # rows at 90, 45, 0, -45, -90: the rows at 45 degrees are active below
GROUP, G, WINDOW, SMOOTH = (np.arange(T) % 2).astype(np.int32), 2, 1, 2
SEGMENTS = [0, 4]
LEVEL_W = [1.0, 0.0, 2.0]
WROW = np.linspace(1.0, 2.0, NY).astype(np.float32)
REV = reversal_util.table(LAT, delta=45.0, lat_bounds=(40, 50))
LWA = lwa_util.rows(LAT, lat_bounds=(40, 50))
STAMPS = dict(t=np.array([0, 3, 7]), row=np.array([2, 2, 1]), col=np.array([3, 8, 15]), bin=None, nbins=1, hy=1, hx=1)
SAME, NONE, BUMP = "same", "none", "same shape, new generation"


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


class Inputs:
    def __init__(self, dtype):
        rng = np.random.default_rng(11)
        self.dtype, self.f64 = dtype, dtype == np.float64
        self.x = (50.0 * rng.standard_normal((T, NY, NX)) + 5500.0).astype(dtype)
        self.lev = (50.0 * rng.standard_normal((T, NLEV, NY, NX)) + 5500.0).astype(dtype)
        self.z = reversal_util.field(LAT, NX, steps=T, seed=3, dtype=dtype)
        self.flag = rng.integers(0, 4, size=(T, NY, NX)).astype(np.int32)
        self.rows = subset_util.table_by_row([[1, 2]] * T)
        self.slab = (T, NY, NX, self.f64)


def slots(trk):
    return (trk.resident_anom(), trk.resident_generation()), (trk.resident_level_mean(), trk.resident_level_mean_generation())


def step(trk, what, call, anom, mean):
    """runs `call`; each slot then is SAME (shape and generation as before), NONE (no slab, a new generation), BUMP (the shape as
    before, a new generation) or a shape (that slab, a new generation)"""
    before = slots(trk)
    got = call()
    for name, (s0, g0), (s1, g1), want in zip(("anomaly slot", "mean slot"), before, slots(trk), (anom, mean)):
        print(what, "|", name, s0, g0, "->", s1, g1, "| wanted:", want)
        if want is SAME:
            assert (s1, g1) == (s0, g0), (what, name)
        elif want is BUMP:
            assert s1 == s0 and g1 != g0, (what, name)
        else:
            assert s1 == (None if want is NONE else want) and g1 != g0, (what, name)
    return got


def same_pair(a, b):
    return all((p is None and q is None) or same_bits(p, q) for p, q in zip(a, b))


def keep_mean(trk, inp):
    return trk.level_mean(inp.lev, LEVEL_W, keep_resident=True)


def anomaly_forms(trk, inp):
    """the three producers of anomalies as functions of the keywords they share; the third reads the resident vertical mean"""
    kw = dict(window=WINDOW, smooth=SMOOTH)
    return (("anomalies", lambda **k: trk.anomalies(inp.x, GROUP, G, **kw, **k)),
            ("anomalies segments", lambda **k: trk.anomalies(inp.x, GROUP, G, segments=SEGMENTS, **kw, **k)),
            ("anomalies_resident", lambda **k: trk.anomalies_resident(GROUP, G, segments=SEGMENTS, **kw, **k)))


def consumers(trk, inp, f64=None, gen=None):
    """what reads the anomaly slot through the binding's own arguments: the slab of the flag's shape, of type f64"""
    f64 = inp.f64 if f64 is None else f64
    return (("composite", lambda: trk.composite(inp.flag, None, resident_f64=f64)),
            ("band", lambda: trk.band(inp.flag, (1, 4), np.ones(NY), resident_gen=trk.resident_generation() if gen is None else gen, resident_f64=f64)),
            ("centred", lambda: trk.centred(None, **STAMPS, resident_f64=f64, shape=(T, NY, NX))),
            ("blockstat", lambda: trk.blockstat(inp.flag, inp.rows, None, resident_f64=f64)),
            ("lifecycle", lambda: trk.lifecycle(inp.flag, None, WROW, resident_f64=f64)))


def c_percentile(trk, f64, shape=(T, NY, NX)):
    out = C.c_double(0.0)
    check((lib().ctk_percentile_f64 if f64 else lib().ctk_percentile_f32)(trk.handle, None, *shape, 1, 4, 0.9, C.byref(out)))


def c_track_resident(trk):
    thr, flag, n = np.full(T, 10.0), np.empty((T, NY, NX), np.int32), C.c_int64(0)
    check(lib().ctk_track_resident(trk.handle, thr.ctypes.data, 0, WROW.ctypes.data, 0.5, 2, 1, flag.ctypes.data, C.byref(n)))


def c_anom_resident(trk, dtype):
    out = np.empty((T, NY, NX), dtype)
    check(lib().ctk_anom_seg_resident(trk.handle, GROUP.ctypes.data, G, WINDOW, SMOOTH, None, out.ctypes.data, None, 0, None, 0))


def c_filter_resident(trk, dtype):
    out = np.empty((T, NY, NX), dtype)
    check(lib().ctk_filter_resident(trk.handle, None, 3, 1, -1, 0, 0, None, 0, out.ctypes.data, T, 0))


def refused(what, call, exc, match):
    with pytest.raises(exc, match=match) as e:
        call()
    print("refused:", what, "|", type(e.value).__name__, "|", e.value)
    assert exc is ValueError or not isinstance(e.value, ValueError), what             # (a state error is no bad argument)


def anomaly_readers_refuse(trk, inp, f64=None):
    for name, call in consumers(trk, inp, f64):
        if name == "blockstat":
            refused(name, call, ValueError, "resident")
        else:
            refused(name, call, ContrackHipError, "resident")
    refused("percentile of this shape", lambda: c_percentile(trk, inp.f64 if f64 is None else f64), ContrackHipError, "no matching anomaly slab")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_call_leaves_the_slots_as_stated(trk, dtype):
    inp = Inputs(dtype)
    other = np.float32 if inp.f64 else np.float64
    step(trk, "release_io", trk.release_io, NONE, NONE)

    # ---- the mean slot: level_mean ------------------------------------------------------------------------------------------------
    mean = step(trk, "level_mean keep", lambda: keep_mean(trk, inp), SAME, inp.slab)
    d_x, d_o = trk.malloc(inp.lev.nbytes), trk.malloc(mean.nbytes)
    try:
        trk.h2d(d_x, inp.lev)
        step(trk, "level_mean_dev", lambda: trk.level_mean_dev(d_x, T, NLEV, NY, NX, LEVEL_W, d_o, f64=inp.f64), SAME, BUMP)
        got = np.empty_like(mean)
        trk.d2h(got, d_o)
        assert same_bits(got, mean)
    finally:
        trk.free(d_x)
        trk.free(d_o)
    assert same_bits(step(trk, "level_mean", lambda: trk.level_mean(inp.lev, LEVEL_W), SAME, NONE), mean)
    assert same_bits(step(trk, "level_mean on an empty slot", lambda: trk.level_mean(inp.lev, LEVEL_W), SAME, NONE), mean)
    step(trk, "level_mean keep, nothing downloaded", lambda: trk.level_mean(inp.lev, LEVEL_W, keep_resident=True, want_out=False), SAME, inp.slab)

    # ---- the anomaly slot: the three anomaly producers -----------------------------------------------------------------------------
    for name, form in anomaly_forms(trk, inp):
        kept = step(trk, name + " keep", lambda: form(keep_resident=True, want_clim=True), inp.slab, SAME)
        clim = step(trk, name + " climatology only", lambda: form(want_anom=False, want_clim=True), SAME, SAME)
        assert same_pair(clim, (None, kept[1]))
        plain = step(trk, name, lambda: form(want_clim=True), NONE, SAME)
        assert same_pair(plain, kept)
        step(trk, name + " climatology only, empty slot", lambda: form(want_anom=False, want_clim=True), SAME, SAME)
        step(trk, name + " on an empty slot", lambda: form(), NONE, SAME)
        step(trk, name + " keep, nothing downloaded", lambda: form(keep_resident=True, want_anom=False), inp.slab, SAME)
    streamed = step(trk, "anomalies_stream", lambda: trk.anomalies_stream(inp.x, GROUP, G, WINDOW, SMOOTH, segments=SEGMENTS, chunk_steps=3), SAME, SAME)
    assert same_bits(streamed[0], trk.anomalies(inp.x, GROUP, G, WINDOW, SMOOTH, segments=SEGMENTS)[0])
    anom = step(trk, "anomalies keep", lambda: trk.anomalies(inp.x, GROUP, G, WINDOW, SMOOTH, keep_resident=True), inp.slab, SAME)[0]

    # ---- what reads the anomaly slot leaves both alone -----------------------------------------------------------------------------
    for name, call in consumers(trk, inp):
        step(trk, name, call, SAME, SAME)
    step(trk, "subset", lambda: trk.subset(inp.flag, subset_util.table_by_id([1, 2])), SAME, SAME)
    step(trk, "percentile", lambda: trk.percentile(None, 1, 4, 0.9), SAME, SAME)
    flag, _ = step(trk, "track_resident", lambda: trk.track_resident(np.full(T, 10.0), 0, WROW, 0.5, 2), SAME, SAME)
    flag = flag.copy()                                                                                     # (the result pool hands its arrays out again)
    assert np.array_equal(flag, trk.track(anom, np.full(T, 10.0), 0, WROW, 0.5, 2, f64=inp.f64)[0])

    # ---- reversal and lwa ------------------------------------------------------------------------------------------------------------
    for name, call in (("reversal", lambda **k: trk.reversal(inp.z, REV, **k)), ("lwa", lambda **k: trk.lwa(inp.z, LWA, **k))):
        plain = step(trk, name, call, SAME, SAME)
        assert same_bits(step(trk, name + " keep", lambda: call(keep_resident=True), inp.slab, SAME), plain)
        step(trk, name + " again", call, SAME, SAME)
        step(trk, name + " keep, nothing downloaded", lambda: call(keep_resident=True, want_out=False), inp.slab, SAME)
        step(trk, "composite of it", consumers(trk, inp)[0][1], SAME, SAME)

    # ---- the anomaly slot refuses: a stale generation, another shape, another type, dropped ---------------------------------------
    stale = trk.resident_generation()
    step(trk, "anomalies keep", lambda: trk.anomalies(inp.x, GROUP, G, WINDOW, SMOOTH, keep_resident=True), inp.slab, SAME)
    refused("band, stale generation", consumers(trk, inp, gen=stale)[1][1], ContrackHipError, "stale")
    anomaly_readers_refuse(trk, inp, f64=not inp.f64)                                                      # the other type is asked for
    step(trk, "anomalies keep, shorter", lambda: trk.anomalies(inp.x[:6], GROUP[:6], G, WINDOW, SMOOTH, keep_resident=True), (6, NY, NX, inp.f64), SAME)
    anomaly_readers_refuse(trk, inp)
    step(trk, "anomalies keep, other type", lambda: trk.anomalies(inp.x.astype(other), GROUP, G, WINDOW, SMOOTH, keep_resident=True), (T, NY, NX, not inp.f64), SAME)
    anomaly_readers_refuse(trk, inp)
    step(trk, "anomalies", lambda: trk.anomalies(inp.x, GROUP, G, WINDOW, SMOOTH), NONE, SAME)
    anomaly_readers_refuse(trk, inp)
    refused("track_resident", lambda: trk.track_resident(np.full(T, 10.0), 0, WROW, 0.5, 2), ContrackHipError, "no anomaly slab is resident")
    refused("ctk_track_resident", lambda: c_track_resident(trk), ContrackHipError, "no anomaly slab is resident")
    refused("percentile", lambda: trk.percentile(None, 1, 4, 0.9), ContrackHipError, "no anomaly slab is resident")

    # ---- the mean slot: the time filter --------------------------------------------------------------------------------------------
    assert trk.resident_level_mean() == inp.slab
    fkw = dict(stride=2, edges="renorm")
    t_out = 4                                                                          # labels at the steps 1, 3, 5, 7
    assert len(trk.time_filter(inp.x, 3, **fkw)) == t_out
    reader = lambda t0, nt, out: out.__setitem__(Ellipsis, inp.x[t0:t0 + nt])          # noqa: E731
    plain = step(trk, "time_filter", lambda: trk.time_filter(inp.x, 3, chunk_steps=3, **fkw), SAME, SAME)
    assert same_bits(step(trk, "time_filter_cb", lambda: trk.time_filter_cb(reader, inp.x.shape, dtype, 3, chunk_steps=3, **fkw), SAME, SAME), plain)
    assert same_bits(step(trk, "time_filter keep", lambda: trk.time_filter(inp.x, 3, chunk_steps=3, keep_resident=True, **fkw), SAME, (t_out, NY, NX, inp.f64)), plain)
    step(trk, "level_mean keep", lambda: keep_mean(trk, inp), SAME, inp.slab)
    assert same_bits(step(trk, "time_filter_cb keep", lambda: trk.time_filter_cb(reader, inp.x.shape, dtype, 3, chunk_steps=3, keep_resident=True, **fkw), SAME,
                          (t_out, NY, NX, inp.f64)), plain)
    step(trk, "time_filter_cb keep, nothing downloaded", lambda: trk.time_filter_cb(reader, inp.x.shape, dtype, 3, sink=False, keep_resident=True), SAME, inp.slab)
    plain = step(trk, "time_filter_resident", lambda: trk.time_filter_resident(3, **fkw), SAME, SAME)
    assert same_bits(plain, trk.time_filter(trk.time_filter(inp.x, 3), 3, **fkw))
    assert same_bits(step(trk, "time_filter_resident keep", lambda: trk.time_filter_resident(3, keep_resident=True, **fkw), SAME, (t_out, NY, NX, inp.f64)), plain)
    step(trk, "time_filter_resident keep, nothing downloaded", lambda: trk.time_filter_resident(2, stride=2, keep_resident=True, want_out=False), SAME,
         (t_out // 2, NY, NX, inp.f64))
    kept = step(trk, "anomalies_resident of the filtered mean", lambda: trk.anomalies_resident(GROUP[:t_out // 2], G, keep_resident=True), (t_out // 2, NY, NX, inp.f64), SAME)
    assert kept[0].shape == (t_out // 2, NY, NX)

    # ---- the mean slot refuses once it is dropped ----------------------------------------------------------------------------------
    step(trk, "level_mean", lambda: trk.level_mean(inp.lev, LEVEL_W), SAME, NONE)
    refused("anomalies_resident", lambda: trk.anomalies_resident(GROUP, G), ContrackHipError, "no vertical mean is resident")
    refused("ctk_anom_seg_resident", lambda: c_anom_resident(trk, dtype), ValueError, "no vertical mean is resident")
    refused("time_filter_resident", lambda: trk.time_filter_resident(3), ContrackHipError, "no vertical mean is resident")
    refused("ctk_filter_resident", lambda: c_filter_resident(trk, dtype), ValueError, "no vertical mean is resident")

    # ---- release_io drops both -----------------------------------------------------------------------------------------------------
    step(trk, "level_mean keep", lambda: keep_mean(trk, inp), SAME, inp.slab)
    step(trk, "release_io", trk.release_io, NONE, NONE)
    anomaly_readers_refuse(trk, inp)
    refused("ctk_track_resident", lambda: c_track_resident(trk), ContrackHipError, "no anomaly slab is resident")
    refused("ctk_anom_seg_resident", lambda: c_anom_resident(trk, dtype), ValueError, "no vertical mean is resident")
    refused("ctk_filter_resident", lambda: c_filter_resident(trk, dtype), ValueError, "no vertical mean is resident")
    step(trk, "release_io again", trk.release_io, NONE, NONE)
