"""ctk_subset_* on the GPU against its statement tests/subset_util.py: the device, host-array and callback paths, both kinds, invert,
by-id and row tables, chunking, in place, count only, background values, the largest id, a consumer fed in HBM, the resident slot and
every error case.  All integers: equality everywhere.  Every slab asserts that the selection is neither empty nor everything."""
import ctypes as C

import numpy as np
import pytest

import reversal_util as ru
import subset_util as su
from contrack_amd import _native
from contrack_amd.contrack import subset_numpy, subset_table

pytestmark = pytest.mark.gpu

IMIN, IMAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
KIND = {su.ID: 'id', su.MASK: 'mask'}


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def slab(T, ny, nx, seed=0, top=9):
    """ids 1 .. top on about four pixels in ten; the background holds 0, -1 and INT32_MIN"""
    rng = np.random.default_rng(seed)
    f = rng.integers(1, top + 1, size=(T, ny, nx)).astype(np.int32)
    f[rng.random(f.shape) < 0.6] = 0
    bg = np.flatnonzero(f.reshape(-1) == 0)
    f.reshape(-1)[bg[::3]] = -1
    f.reshape(-1)[bg[1::3]] = IMIN
    return f


def tables(T, top=9, seed=0):
    """a by-id table and a row table with empty, short and full slices"""
    rng = np.random.default_rng(100 + seed)
    slices = [sorted(rng.choice(np.arange(1, top + 3), size=int(rng.integers(0, top)), replace=False).tolist()) for _ in range(T)]
    slices[0] = []
    return {"id": su.table_by_id([2, 3, 5, 8, top + 2]), "row": su.table_by_row(slices)}


def on_device(trk, f, table, invert=False, kind='id', off=0, in_place=False, count_only=False, want_hits=True):
    """ctk_subset_dev on a copy of f that starts `off` bytes past a 16-byte boundary (the output too): (out or None, hits, n, flag after)"""
    d_f, d_o = trk.malloc(f.nbytes + 16), trk.malloc(f.nbytes + 16)
    try:
        pf, po = C.c_void_p(d_f.value + off), C.c_void_p(d_o.value + off)
        trk.h2d(pf, f)
        trk.memset(d_o, 0x5a, f.nbytes + 16)
        hits, n = trk.subset_dev(pf, f.shape[0], f.shape[1], f.shape[2], table, None if count_only else pf if in_place else po, invert, kind, want_hits)
        got, after = np.empty_like(f), np.empty_like(f)
        trk.d2h(got, po)
        trk.d2h(after, pf)
        return (None if count_only else after if in_place else got), hits, n, after, got
    finally:
        trk.free(d_f)
        trk.free(d_o)


def same(got, want, case):
    out, hits, n = got[:3]
    assert out.dtype == np.int32 and np.array_equal(out, want[0]), (case, np.argwhere(out != want[0])[:4].tolist())
    assert hits.dtype == np.uint64 and np.array_equal(hits, want[1]), (case, hits.tolist(), want[1].tolist())
    assert n == want[2], (case, n, want[2])


# ---- paths and options ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 6, 8), (5, 5, 7)], ids=["vector", "scalar"])
@pytest.mark.parametrize("which", ["id", "row"])
def test_every_path_equals_the_statement(trk, shape, which):
    f = slab(*shape, seed=1)
    table = tables(shape[0])[which]
    for kind in (su.ID, su.MASK):
        for invert in (False, True):
            want = su.subset(f, *table, invert, kind)
            assert 0 < want[2] < np.count_nonzero(f > 0) and want[1].any() and not want[1].all()
            case = (shape, which, kind, invert)
            same(on_device(trk, f, table, invert, KIND[kind]), want, case + ("dev",))
            assert trk.debug_subset_launch()[1] == (shape[1] * shape[2] % 4 == 0)
            same(trk.subset(f, table, invert, KIND[kind]), want, case + ("host",))
            same(trk.subset_cb(f, f.shape, table, invert, KIND[kind]), want, case + ("cb",))
            same(trk.subset_cb(lambda t0, nt, out: out.__setitem__(Ellipsis, f[t0:t0 + nt]), f.shape, table, invert, KIND[kind]), want, case + ("reader",))
            out, n, hits = subset_numpy(f, table, invert, KIND[kind], return_hits=True)
            same((out, hits, n), want, case + ("numpy",))
            out, n = subset_numpy(f.astype(np.int64), table, invert, KIND[kind])
            assert np.array_equal(out, want[0]) and n == want[2]
    # without hits a by-id table takes the bitmap: the same output
    want = su.subset(f, *tables(shape[0])["id"])
    out, hits, n = trk.subset(f, tables(shape[0])["id"], want_hits=False)
    assert hits is None and np.array_equal(out, want[0]) and n == want[2] and trk.debug_subset_launch()[0] == _native.SUBSET_FORMS.index("bitmap")


def test_sinks_of_the_callback_path(trk):
    f = slab(6, 4, 8, seed=2)
    table = tables(6)["row"]
    want = su.subset(f, *table)
    arr = np.full(f.shape, 77, dtype=np.int32)
    out, hits, n = trk.subset_cb(f, f.shape, table, sink=arr, chunk_steps=4)
    assert out is arr
    same((arr, hits, n), want, "array sink")
    seen, got = [], np.full(f.shape, 77, dtype=np.int32)

    def writer(t0, nt, values):
        seen.append((t0, nt))
        got[t0:t0 + nt] = values
    out, hits, n = trk.subset_cb(f, f.shape, table, sink=writer, chunk_steps=4)
    assert out is None and seen == [(0, 4), (4, 2)]
    same((got, hits, n), want, "writer")

    def bad(t0, nt, values):
        raise KeyError("sink")
    with pytest.raises(KeyError):
        trk.subset_cb(f, f.shape, table, sink=bad)
    same(trk.subset(f, table), want, "after a failing writer")


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["id", "row"])
def test_same_bytes_for_every_chunk_length(trk, which):
    T = 7
    f = slab(T, 5, 8, seed=3)
    table = tables(T, seed=1)[which]
    for invert in (False, True):
        want = su.subset(f, *table, invert)
        assert 0 < want[2] < np.count_nonzero(f > 0)
        for chunk in (1, 2, T - 1, T, T + 5):
            same(trk.subset(f, table, invert, chunk_steps=chunk), want, (which, invert, chunk, "host"))
            same(trk.subset_cb(f, f.shape, table, invert, chunk_steps=chunk), want, (which, invert, chunk, "cb"))
            out, n, hits = subset_numpy(f, table, invert, chunk_steps=chunk, return_hits=True)
            same((out, hits, n), want, (which, invert, chunk, "numpy"))


# ---- in place, count only -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["id", "row"])
def test_in_place_and_count_only(trk, which):
    f = slab(5, 6, 8, seed=4)
    table = tables(5, seed=2)[which]
    for kind in (su.ID, su.MASK):
        want = su.subset(f, *table, True, kind)
        got = on_device(trk, f, table, True, KIND[kind], in_place=True)
        same(got, want, (which, kind, "in place"))
        assert (got[4].view(np.uint8) == 0x5a).all()                                # the other buffer was not touched
    want = su.subset(f, *table)
    out, hits, n, after, other = on_device(trk, f, table, count_only=True)
    assert out is None and np.array_equal(hits, want[1]) and n == want[2]
    assert np.array_equal(after, f) and (other.view(np.uint8) == 0x5a).all()       # nothing written anywhere
    out, hits, n = trk.subset(f, table, want_out=False)
    assert out is None and np.array_equal(hits, want[1]) and n == want[2]
    out, hits, n = trk.subset(f, table, want_out=False, want_hits=False)
    assert out is None and hits is None and n == want[2]
    calls = []
    out, hits, n = trk.subset_cb(lambda t0, nt, o: (calls.append(t0), o.__setitem__(Ellipsis, f[t0:t0 + nt])), f.shape, table, sink=False, chunk_steps=2)
    assert out is None and calls == [0, 2, 4] and np.array_equal(hits, want[1]) and n == want[2]
    # the host entry in place: out is the flag array itself
    g = f.copy()
    rc = _native.lib().ctk_subset(trk.handle, g.ctypes.data, 5, 6, 8, table[0].ctypes.data, len(table[0]), table[1].ctypes.data, len(table[1]), 0, 0,
                                  g.ctypes.data, None, None, 2)
    assert rc == 0 and np.array_equal(g, want[0])


# ---- values -----------------------------------------------------------------------------------------------------------------------------
def test_background_values_are_never_selected(trk):
    f = slab(3, 4, 8, seed=5)
    assert (f == 0).any() and (f == -1).any() and (f == IMIN).any()
    for table in (su.table_by_id([]), su.table_by_id([1, 2, 3, 4, 5, 6, 7, 8, 9]), su.table_by_row([[], [4], []])):
        for invert in (False, True):
            for hits in (True, False):
                want = su.subset(f, *table, invert)
                assert not want[0][f <= 0].any()
                out, h, n = trk.subset(f, table, invert, want_hits=hits)
                assert np.array_equal(out, want[0]) and n == want[2] and (h is None or np.array_equal(h, want[1])), (table, invert, hits)
    out, h, n = trk.subset(f, su.table_by_id([]), True)
    assert np.array_equal(out, np.where(f > 0, f, 0)) and n == np.count_nonzero(f > 0) > 0
    allbg = np.where(f > 0, -f, f)                                                 # no lane has anything to look up
    out, h, n = trk.subset(allbg, su.table_by_id([1, 2, 3]), True)
    assert not out.any() and n == 0 and not h.any()


def test_largest_id(trk):
    f = slab(4, 3, 8, seed=6)
    f[1, 1, :5] = IMAX
    f[2, 0, 0] = IMAX - 1
    for table in (su.table_by_id([5, IMAX]), su.table_by_id([IMAX]), su.table_by_row([[IMAX], [3, IMAX], [IMAX - 1], []])):
        for invert in (False, True):
            for hits in (True, False):
                want = su.subset(f, *table, invert)
                out, h, n = trk.subset(f, table, invert, want_hits=hits)
                assert np.array_equal(out, want[0]) and n == want[2] and (h is None or np.array_equal(h, want[1])), (table, invert, hits)
                assert (out[1, 1, :5] == IMAX).all() != invert
    assert su.subset(f, *su.table_by_id([5, IMAX]))[1].tolist() == [int(np.count_nonzero(f == 5)), 5]


# ---- beside the other entries -----------------------------------------------------------------------------------------------------------
def test_selection_in_hbm_feeds_frequency(trk):
    f = slab(9, 6, 8, seed=7)
    table = tables(9, seed=3)["row"]
    want = su.subset(f, *table)[0]
    counts = (want > 0).sum(axis=0).astype(np.uint32)[None]
    assert counts.any()
    d_f, d_o = trk.malloc(f.nbytes), trk.malloc(f.nbytes)
    try:
        trk.h2d(d_f, f)
        trk.subset_dev(d_f, 9, 6, 8, table, d_o)
        assert np.array_equal(trk.frequency_dev(d_o, 9, 6, 8), counts)
        assert np.array_equal(trk.frequency(want), counts)
        above1 = trk.frequency_dev(d_o, 9, 6, 8, above=1)
        assert np.array_equal(above1, (want > 1).sum(axis=0).astype(np.uint32)[None])
    finally:
        trk.free(d_f)
        trk.free(d_o)


def test_resident_slot_is_not_touched(trk):
    lat = ru.grid(7.5)
    z = ru.field(lat, 8, steps=4, seed=1)
    trk.reversal(z, ru.table(lat), keep_resident=True)
    gen, res = trk.resident_generation(), trk.resident_anom()
    assert res[:3] == z.shape
    f = slab(4, 5, 8, seed=8)
    for table in tables(4).values():
        trk.subset(f, table, chunk_steps=2)
        trk.subset_cb(f, f.shape, table)
        on_device(trk, f, table)
        with pytest.raises(ValueError):
            trk.subset(f, (table[0], -table[1]))
        assert trk.resident_generation() == gen and trk.resident_anom() == res


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_every_error_case_leaves_the_handle_working(trk):
    L = _native.lib()
    T, ny, nx = 3, 4, 8
    f = slab(T, ny, nx, seed=9)
    out = np.full(f.shape, 77, dtype=np.int32)
    hits = np.full(8, 77, dtype=np.uint64)
    nsel = C.c_int64(77)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    good_off, good_ids = i64(0, 1, 1, 3), i32(4, 2, 6)
    want = su.subset(f, good_off, good_ids)

    def host(off=good_off, ids=good_ids, n_off=None, n_ids=None, T=T, ny=ny, nx=nx, flag=f, kind=0, chunk=0, o=out, h=hits, n=nsel):
        return L.ctk_subset(trk.handle, None if flag is None else flag.ctypes.data, T, ny, nx, None if off is None else off.ctypes.data,
                            len(off) if n_off is None else n_off, None if ids is None else ids.ctypes.data, len(ids) if n_ids is None else n_ids, 0, kind,
                            None if o is None else o.ctypes.data, None if h is None else h.ctypes.data, None if n is None else C.byref(n), chunk)

    cases = {
        "null flag": dict(flag=None),
        "null off": dict(off=None, n_off=T + 1),
        "null ids": dict(ids=None, n_ids=3),
        "T < 1": dict(T=0, n_off=1),
        "ny < 1": dict(ny=0),
        "nx < 1": dict(nx=-1),
        "plane of 2^31": dict(ny=65536, nx=32768),
        "n_off": dict(off=i64(0, 1, 3)),
        "off[0]": dict(off=i64(1, 1, 1, 3)),
        "off decreasing": dict(off=i64(0, 2, 1, 3)),
        "off beyond": dict(off=i64(0, 4, 4, 3)),
        "off[T]": dict(off=i64(0, 1, 1, 2)),
        "id 0": dict(ids=i32(4, 0, 6)),
        "id negative": dict(ids=i32(-4, 2, 6)),
        "equal ids": dict(ids=i32(4, 2, 2)),
        "falling ids": dict(ids=i32(4, 6, 2)),
        "by id, falling": dict(off=i64(0, 3), ids=i32(4, 2, 6)),
        "kind": dict(kind=2),
        "kind negative": dict(kind=-1),
        "chunk_steps": dict(chunk=-1),
        "nothing to produce": dict(o=None, h=None, n=None),
    }
    for name, kw in cases.items():
        assert host(**kw) == _native.CTK_E_INVALID, name
        msg = L.ctk_last_error().decode()
        assert "ctk_subset" in msg, (name, msg)
        assert (out == 77).all() and (hits == 77).all() and nsel.value == 77, name
        same(trk.subset(f, (good_off, good_ids)), want, ("after", name))
    # the same checks guard the device and the callback entries
    d = trk.malloc(f.nbytes)
    try:
        trk.h2d(d, f)
        dev = lambda off, ids, flag=d, o=d, kind=0, n=nsel: L.ctk_subset_dev(trk.handle, flag, T, ny, nx, off.ctypes.data, len(off), ids.ctypes.data, len(ids), 0, kind,
                                                                          o, None, None if n is None else C.byref(n))
        assert dev(good_off, good_ids, flag=None) == _native.CTK_E_INVALID
        assert dev(good_off, good_ids, o=None, n=None) == _native.CTK_E_INVALID
        assert dev(i64(0, 1, 3), good_ids) == _native.CTK_E_INVALID
        assert dev(good_off, i32(4, 2, 2)) == _native.CTK_E_INVALID
        assert dev(good_off, good_ids, kind=5) == _native.CTK_E_INVALID
        back = np.empty_like(f)
        trk.d2h(back, d)
        assert np.array_equal(back, f) and nsel.value == 77
        assert dev(good_off, good_ids) == 0 and nsel.value == want[2]
        trk.d2h(back, d)
        assert np.array_equal(back, want[0])
    finally:
        trk.free(d)
    null_reader = C.cast(None, _native.READ_CHUNK_FN)
    null_writer = C.cast(None, _native.WRITE_CHUNK_FN)
    assert L.ctk_subset_cb(trk.handle, T, ny, nx, null_reader, None, good_off.ctypes.data, 4, good_ids.ctypes.data, 3, 0, 0, null_writer, None, None, C.byref(nsel),
                           0) == _native.CTK_E_INVALID
    with pytest.raises(ValueError):
        trk.subset_cb(f, f.shape, (good_off, good_ids), chunk_steps=-1)
    with pytest.raises(ValueError):
        trk.subset(f, (good_off, good_ids), kind='both')
    with pytest.raises(ValueError):
        subset_numpy(f, subset_table([1]), chunk_steps=-2)
    same(trk.subset_cb(f, f.shape, (good_off, good_ids)), want, "at the end")
