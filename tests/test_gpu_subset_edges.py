"""k_subset at its edges: the scalar and the vector form on the smallest planes and an offset pointer, the stride loop under both XCD
mappings, the bitmap's word boundaries, every form of ctk_subset_plan below, at and above the capacity that separates it from the next
(the capacities come from the plan hook), empty and neighbouring slices, a slice across a chunk cut, and the LDS hit counters with one
id on every pixel.  Against tests/subset_util.py, equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import subset_util as su
from contrack_amd import _native

pytestmark = pytest.mark.gpu

FORMS = {name: i for i, name in enumerate(_native.SUBSET_FORMS)}
CAPS = None


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def caps():
    global CAPS
    if CAPS is None:
        CAPS = _native.subset_plan(False, 1, 1, 4, 8)
    return CAPS


def slab_of(ids, T, ny, nx, seed=0, cover=0.5):
    """values drawn from `ids` on about half the pixels, 0 / -1 elsewhere"""
    rng = np.random.default_rng(seed)
    f = np.asarray(ids, dtype=np.int32)[rng.integers(0, len(ids), size=(T, ny, nx))]
    f[rng.random(f.shape) >= cover] = 0
    f[0].reshape(-1)[-1:] = -1
    return f


def dev(trk, f, table, invert=False, kind='id', off=0, want_hits=True):
    d_f, d_o = trk.malloc(f.nbytes + 16), trk.malloc(f.nbytes + 16)
    try:
        pf, po = C.c_void_p(d_f.value + off), C.c_void_p(d_o.value + off)
        trk.h2d(pf, f)
        trk.memset(d_o, 0x5a, f.nbytes + 16)
        hits, n = trk.subset_dev(pf, f.shape[0], f.shape[1], f.shape[2], table, po, invert, kind, want_hits)
        got = np.empty_like(f)
        trk.d2h(got, po)
        return got, hits, n
    finally:
        trk.free(d_f)
        trk.free(d_o)


def same(got, want, case):
    assert np.array_equal(got[0], want[0]), (case, np.argwhere(got[0] != want[0])[:4].tolist())
    assert got[1] is None or np.array_equal(got[1], want[1]), (case, np.flatnonzero(got[1] != want[1])[:8].tolist())
    assert got[2] == want[2], (case, got[2], want[2])


# ---- scalar and vector forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
def test_smallest_planes_and_an_offset_pointer(trk, T):
    for (ny, nx), vec in (((1, 1), 0), ((1, 3), 0), ((3, 5), 0), ((4, 8), 1)):
        f = slab_of([1, 2, 3, 40], T, ny, nx, seed=ny * nx, cover=0.8)
        f.reshape(-1)[0] = 2
        for name, table in (("id", su.table_by_id([2, 40])), ("row", su.table_by_row([[2], [1, 3], [2, 40]][:T]))):
            for invert in (False, True):
                for hits in (False, True):
                    want = su.subset(f, *table, invert)
                    case = (T, ny, nx, name, invert, hits)
                    same(dev(trk, f, table, invert, want_hits=hits), want, case)
                    assert trk.debug_subset_launch()[1] == vec == _native.subset_plan(name == "row", 40, 2, ny, nx, T)["vec"], case
                    same(dev(trk, f, table, invert, off=4, want_hits=hits), want, case + ("offset",))
                    assert trk.debug_subset_launch()[1] == 0, case
                    same(trk.subset(f, table, invert, 'mask', want_hits=hits), su.subset(f, *table, invert, su.MASK), case + ("host",))


# ---- stride loop ------------------------------------------------------------------------------------------------------------------------
def test_grid_striding_and_both_xcd_mappings(trk):
    """more (step, part) pairs than workgroups: 3 workgroups walk 2 parts x 9 steps (vector) and 5 parts x 4 steps (scalar)"""
    part = caps()["part_lanes"]
    cases = [slab_of([1, 2, 3, 4, 5], 9, 4, part + 8, seed=1), slab_of([1, 2, 3, 4, 5], 4, 1, 4 * part + 3, seed=2)]
    assert _native.subset_plan(True, 0, 3, 4, part + 8, steps=9)["blocks"] == 18 and _native.subset_plan(True, 0, 3, 1, 4 * part + 3, steps=4)["blocks"] == 20
    assert _native.subset_plan(True, 0, 3, 4, part + 8, steps=9)["vec"] == 1 and _native.subset_plan(True, 0, 3, 1, 4 * part + 3, steps=4)["vec"] == 0
    try:
        for f in cases:
            T = f.shape[0]
            tabs = {"id": su.table_by_id([2, 5]), "row": su.table_by_row([sorted({1 + t % 5, 1 + (t + 2) % 5}) for t in range(T)])}
            for name, table in tabs.items():
                for hits in (False, True):
                    want = su.subset_fast(f, *table)
                    assert 0 < want[2] < np.count_nonzero(f > 0)
                    for mode in (0, 1):
                        for cap in (0, 3, 1):
                            trk.debug_set_subset(mode, cap)
                            same(dev(trk, f, table, want_hits=hits), want, (f.shape, name, hits, mode, cap))
                            if cap:
                                assert trk.debug_subset_launch()[2] == cap
                            same(trk.subset(f, table, chunk_steps=3, want_hits=hits), want, (f.shape, name, hits, mode, cap, "host"))
    finally:
        trk.debug_set_subset()


# ---- bitmap -----------------------------------------------------------------------------------------------------------------------------
def test_bitmap_word_boundaries(trk):
    vals = [30, 31, 32, 33, 34, 62, 63, 64, 65, 66]
    f = slab_of(vals, 2, 4, 8, seed=3, cover=0.9)
    f.reshape(-1)[:len(vals)] = vals
    for ids in ([31], [32], [33], [63], [64], [65], [31, 32, 33], [63, 64, 65], [31, 33, 63, 65], [32, 64]):
        for invert in (False, True):
            want = su.subset(f, *su.table_by_id(ids), invert)
            assert 0 < want[2] < np.count_nonzero(f > 0)
            same(dev(trk, f, su.table_by_id(ids), invert, want_hits=False), want, (ids, invert))
            assert trk.debug_subset_launch()[0] == FORMS["bitmap"]
            assert _native.subset_plan(False, max(ids), len(ids), 4, 8)["lds"] == 4 * (max(ids) // 32 + 1)


# ---- capacities -------------------------------------------------------------------------------------------------------------------------
def test_bitmap_at_its_largest_id(trk):
    bits = caps()["bitmap_bits"]
    for top in (bits - 2, bits - 1, bits):
        vals = [1, 31, top - 1, top, top + 1]
        f = slab_of(vals, 2, 3, 8, seed=top % 7)
        f.reshape(-1)[:5] = vals
        table = su.table_by_id([31, top])
        for invert in (False, True):
            want = su.subset(f, *table, invert)
            assert 0 < want[2] < np.count_nonzero(f > 0)
            same(dev(trk, f, table, invert, want_hits=False), want, (top, invert))
            assert trk.debug_subset_launch()[0] == (FORMS["bitmap"] if top < bits else FORMS["search_lds"]), top


@pytest.mark.parametrize("by_row", [False, True], ids=["by id", "rows"])
@pytest.mark.parametrize("hits", [False, True], ids=["no hits", "hits"])
def test_search_forms_at_the_lds_capacity(trk, by_row, hits):
    """K ids (by id: beyond the bitmap's reach) or a longest slice of K: in LDS up to the capacity, in global memory above it; the
    first, the last and a middle entry are in the slab, and so are values just beside them"""
    c = caps()
    base = c["bitmap_bits"]                                                          # ids base + 3 k: no bitmap for them
    T = 3
    for K in (c["lds_ids"] - 1, c["lds_ids"], c["lds_ids"] + 1):
        ids = base + 3 * np.arange(K, dtype=np.int64)
        probe = [ids[0], ids[0] + 1, ids[1], ids[K // 2], ids[K // 2] - 1, ids[K - 2], ids[K - 1], ids[K - 1] + 1, 7]
        f = slab_of(probe, T, 4, 8, seed=K % 5, cover=0.9)
        f.reshape(-1)[:len(probe)] = probe
        f[1].reshape(-1)[:len(probe)] = probe
        table = su.table_by_row([[7], ids, ids[:5]]) if by_row else su.table_by_id(ids)
        for invert in (False, True):
            want = su.subset_fast(f, *table, invert)
            assert 0 < want[2] < np.count_nonzero(f > 0) and want[1].any()
            same(dev(trk, f, table, invert, want_hits=hits), want, (K, invert))
            lds = K <= c["lds_ids"]
            expect = FORMS[("row_lds" if lds else "row_glb") if by_row else ("search_lds" if lds else "search_glb")]
            assert trk.debug_subset_launch()[0] == expect == _native.subset_plan(by_row, int(ids[-1]), K, 4, 8, T, hits=hits)["form"], K
            same(trk.subset(f, table, invert, chunk_steps=2, want_hits=hits), want, (K, invert, "host"))


# ---- slices -------------------------------------------------------------------------------------------------------------------------------
def test_empty_slices_and_ids_listed_next_door(trk):
    T = 6
    f = slab_of([1, 2, 3, 4], T, 3, 8, seed=4, cover=0.9)
    for slices in ([[], [1, 2], [3], [4], [1], [2]], [[1], [2], [], [], [3], [4]], [[1], [2], [3], [4], [1, 2], []], [[]] * T):
        table = su.table_by_row(slices)
        for invert in (False, True):
            want = su.subset(f, *table, invert)
            for t, s in enumerate(slices):
                if not s:
                    assert not want[0][t].any() if not invert else np.array_equal(want[0][t], np.where(f[t] > 0, f[t], 0))
            same(dev(trk, f, table, invert), want, (slices, invert))
            for chunk in (1, 2, 4):
                same(trk.subset(f, table, invert, chunk_steps=chunk), want, (slices, invert, chunk))
    # id 9 fills the plane of step 2 and is listed at steps 1 and 3 only
    f[2] = 9
    table = su.table_by_row([[1], [9], [2], [9], [], []])
    want = su.subset(f, *table)
    assert not want[0][2].any() and want[1][[1, 3]].tolist() == [0, 0]
    same(dev(trk, f, table), want, "next door")
    for chunk in (1, 2, 3):                                                          # (cuts before, inside and after the steps around it)
        same(trk.subset(f, table, chunk_steps=chunk), want, ("next door", chunk))
        same(trk.subset_cb(f, f.shape, table, chunk_steps=chunk), want, ("next door, cb", chunk))


# ---- hits -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_row", [False, True], ids=["by id", "rows"])
def test_one_id_on_every_pixel(trk, by_row):
    """every lane of every workgroup adds to ONE counter in LDS; several parts per step, so several flushes into one total"""
    part = caps()["part_lanes"]
    T, ny, nx = 3, 4, 2 * part + 4
    f = np.full((T, ny, nx), 6, dtype=np.int32)
    table = su.table_by_row([[6], [5, 6, 7], [6, 8]]) if by_row else su.table_by_id([5, 6, 7])
    want = su.subset_fast(f, *table)
    assert want[2] == f.size and int(want[1].sum()) == f.size and sorted(want[1].tolist())[-1] >= ny * nx
    assert _native.subset_plan(by_row, 7, 3, ny, nx, T, hits=True)["bps"] >= 2
    try:
        for cap in (0, 2):
            trk.debug_set_subset(-1, cap)
            same(dev(trk, f, table), want, (by_row, cap))
            assert trk.debug_subset_launch()[0] == FORMS["row_lds" if by_row else "search_lds"]
    finally:
        trk.debug_set_subset()
