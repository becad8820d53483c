"""The host plumbing the map consumers share, without a GPU: the binding's callback trampolines (_native._Trampolines) called
directly on a ctypes buffer, and the class's plan for grouped maps over members (contrack._group_plan, contrack._map_layout) against
the expressions calc_frequency, calc_spells and calc_composite each carried before, written out here."""
import ctypes as C
import itertools

import numpy as np
import pytest

import minixr
from contrack_amd import _native
from contrack_amd.contrack import contrack

minixr.install_as_xarray()          # only when the real package is absent

NT, NY, NX = 2, 3, 4


# ---- trampolines ---------------------------------------------------------------------------------------------------------------
def _buffer(values=None):
    buf = (C.c_float * (NT * NY * NX))()
    view = np.ctypeslib.as_array(buf).reshape(NT, NY, NX)
    if values is not None:
        view[...] = values
    return buf, view


def _slab():
    return np.arange(5 * NY * NX, dtype=np.float32).reshape(5, NY, NX) + 0.5


def test_reader_from_an_array_and_from_a_callable():
    slab = _slab()
    tr = _native._Trampolines()
    buf, view = _buffer()
    cb = tr.reader(slab, C.c_float, (NY, NX))
    assert isinstance(cb, _native.READ_CHUNK_FN)
    assert cb(None, 1, NT, C.addressof(buf)) == 0
    assert np.array_equal(view, slab[1:3])
    seen = []

    def source(t0, nt, out):
        seen.append((t0, nt, out.shape, out.dtype))
        out[...] = slab[t0:t0 + nt] * 2
    buf, view = _buffer()
    cb = tr.reader(source, C.c_float, (NY, NX))
    assert cb(None, 3, NT, C.addressof(buf)) == 0
    assert seen == [(3, NT, (NT, NY, NX), np.dtype(np.float32))] and type(seen[0][0]) is int
    assert np.array_equal(view, slab[3:5] * 2)
    tr.finish(0)                                                    # nothing was raised: the return code decides
    assert not tr.reader(None, C.c_float, (NY, NX))                 # the NULL reader


def test_writer_to_an_array_and_to_a_callable():
    chunk = _slab()[:NT] - 7
    tr = _native._Trampolines()
    buf, _ = _buffer(chunk)
    sink = np.zeros((5, NY, NX), dtype=np.float32)
    cb = tr.writer(sink, C.c_float, (NY, NX))
    assert isinstance(cb, _native.WRITE_CHUNK_FN)
    assert cb(None, 3, NT, C.addressof(buf)) == 0
    assert np.array_equal(sink[3:5], chunk) and not sink[:3].any()
    got = []
    cb = tr.writer(lambda t0, nt, values: got.append((t0, nt, values.copy())), C.c_float, (NY, NX))
    assert cb(None, 1, NT, C.addressof(buf)) == 0
    assert got[0][:2] == (1, NT) and np.array_equal(got[0][2], chunk)
    assert not tr.writer(None, C.c_float, (NY, NX))                 # the NULL writer


def test_an_exception_stays_behind_the_callback_and_finish_raises_it():
    boom = OSError("no such chunk")

    def source(t0, nt, out):
        raise boom
    tr = _native._Trampolines()
    buf, _ = _buffer()
    assert tr.reader(source, C.c_float, (NY, NX))(None, 0, NT, C.addressof(buf)) != 0
    checked = []
    with pytest.raises(OSError) as e:
        tr.finish(-1, check=checked.append)                         # in preference to the library's return code
    assert e.value is boom and checked == []
    with pytest.raises(OSError) as e:
        tr.finish(0)
    assert e.value is boom
    # a second failure does not displace the first; another callback type goes through wrap()
    other = tr.wrap(C.CFUNCTYPE(C.c_int, C.c_int), lambda v: 1 // v)
    assert other(1) == 0 and other(0) != 0 and len(tr.errors) == 2
    with pytest.raises(OSError):
        tr.finish(0)
    ok = _native._Trampolines()
    ok.finish(5, check=checked.append)
    assert checked == [5]


def test_flag_i32_keeps_its_messages():
    assert _native._flag_i32(np.zeros((2, 3, 4), np.int16), "x_cb").dtype == np.int32
    with pytest.raises(ValueError, match=r"\(time, lat, lon\)"):
        _native._flag_i32(np.zeros((3, 4), np.int32), "x_cb")
    for wide in (np.int64, np.uint32, np.float32):
        with pytest.raises(ValueError, match=r"int32 here \(wider ids: x_cb, or contrack.x_numpy\)"):
            _native._flag_i32(np.zeros((2, 3, 4), wide), "x_cb, or contrack.x_numpy")


# ---- the plan of a grouped map over members ---------------------------------------------------------------------------------------
T, M, G = 5, 2, 3
NAMES = ("time", "latitude", "longitude")
IDS = np.array([2, 0, 1, 1, 2], dtype=np.int64)
UNIQ = np.array([10, 20, 30])
ORDERS = [("member", "time", "latitude", "longitude"), ("time", "member", "latitude", "longitude"),
          ("latitude", "longitude", "time", "member"), ("longitude", "member", "latitude", "time")]


def _before(dims, ids, uniq, groupby, member, pool):
    """what calc_frequency / calc_spells / calc_composite each computed in place: (group, G, out_dims, coord keys, shaped)"""
    m = 1 if member is None else M
    g = 1 if ids is None else len(uniq)
    per_member = member is not None and not pool
    gids = np.zeros(T, dtype=np.int32) if ids is None else ids
    if per_member:
        gids = (np.arange(m, dtype=np.int32)[:, None] * g + gids[None, :]).reshape(-1)
    else:
        gids = np.tile(gids, m)
    group = gids if (per_member or ids is not None) else None
    lead = ((member,) if per_member else ()) + ((groupby,) if groupby is not None else ())
    have = lead + NAMES[1:]
    gone = (("time",) if groupby is None else ()) + ((member,) if member is not None and pool else ())
    out_dims = tuple(groupby if d == "time" else d for d in dims if d not in gone)

    def shaped(a):
        if per_member:
            a = a.reshape((m, g) + a.shape[1:])
        if ids is None:
            a = a[:, 0] if per_member else a[0]
        return np.ascontiguousarray(a.transpose([have.index(d) for d in out_dims]))
    keys = set(() if groupby is None else (groupby,)) | set((member,) if member in lead else ()) | set(NAMES[1:])
    return group, g, out_dims, keys, shaped


@pytest.fixture(scope="module")
def klass():
    ds = minixr.make_dataset(np.zeros((T, NY, NX), np.float32), 60.0 - np.arange(NY), np.arange(NX, dtype=np.float64))
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("grouped,member,pool", list(itertools.product([False, True], [None, "member"], [False, True])))
def test_group_plan_and_layout_are_what_the_three_methods_computed(klass, order, grouped, member, pool):
    dims = tuple(d for d in order if member is not None or d != "member")
    ids, uniq, groupby = (IDS, UNIQ, "month") if grouped else (None, None, None)
    want_group, want_g, want_dims, want_keys, want_shaped = _before(dims, ids, uniq, groupby, member, pool)
    size = None if member is None else M
    group, g, per_member = klass._group_plan(ids, uniq, T, size, pool)
    assert g == want_g and per_member == (member is not None and not pool)
    if want_group is None:
        assert group is None
    else:
        assert group.dtype == want_group.dtype and np.array_equal(group, want_group)
    out_dims, coords, shaped = klass._map_layout(dims, member, pool, groupby, uniq, size, g)
    assert out_dims == want_dims and set(coords) == want_keys
    if grouped:
        assert np.array_equal(coords[groupby], UNIQ)
    if member in coords:
        assert np.array_equal(coords[member], np.arange(M))         # (the dataset has no such coordinate: its indices)
    a = np.arange((M if per_member else 1) * g * NY * NX, dtype=np.int64).reshape(-1, NY, NX)
    got, want = shaped(a), want_shaped(a)
    assert got.shape == want.shape and got.flags.c_contiguous and np.array_equal(got, want)
