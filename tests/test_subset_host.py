"""The statement of ctk_subset_* (tests/subset_util.py) against numpy's own expressions, subset_table's validation, the rule
ctk_subset_plan through its host-only hook, and the header's new entries.  No GPU."""
import os
import re

import numpy as np
import pytest

import subset_util as su
from contrack_amd import _native
from contrack_amd.contrack import subset_table


def slab(T=5, ny=6, nx=7, seed=0, top=9):
    rng = np.random.default_rng(seed)
    f = rng.integers(-2, top + 1, size=(T, ny, nx)).astype(np.int32)
    f[rng.random(f.shape) < 0.5] = 0
    f.flat[:3] = (0, -1, np.iinfo(np.int32).min)
    return f


# ---- the statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("kind", [su.ID, su.MASK])
def test_by_id_statement_is_isin_and_where(invert, kind):
    f = slab()
    for ids in ([], [3], [2, 5, 9], [1, 2, 3, 4, 5, 6, 7, 8, 9], [4, 77]):
        off, tab = su.table_by_id(ids)
        out, hits, n = su.subset(f, off, tab, invert, kind)
        found = (f > 0) & np.isin(f, tab)
        sel = ((f > 0) & ~found) if invert else found
        assert np.array_equal(out, np.where(sel, f if kind == su.ID else 1, 0)) and out.dtype == np.int32
        assert n == np.count_nonzero(sel)
        assert hits.tolist() == [int(np.count_nonzero(f == i)) for i in ids]
        fast = su.subset_fast(f, off, tab, invert, kind)
        assert np.array_equal(fast[0], out) and np.array_equal(fast[1], hits) and fast[2] == n


@pytest.mark.parametrize("invert", [False, True])
def test_row_statement_is_a_loop_over_steps(invert):
    f = slab(T=6, seed=1)
    slices = [[], [1, 2], [9], [], [2, 3, 4, 5], [7]]
    off, tab = su.table_by_row(slices)
    out, hits, n = su.subset(f, off, tab, invert, su.ID)
    want_hits, total = [], 0
    for t, s in enumerate(slices):
        found = (f[t] > 0) & np.isin(f[t], s)
        sel = ((f[t] > 0) & ~found) if invert else found
        assert np.array_equal(out[t], np.where(sel, f[t], 0)), t
        total += np.count_nonzero(sel)
        want_hits += [int(np.count_nonzero(f[t] == i)) for i in s]
    assert n == total and hits.tolist() == want_hits
    fast = su.subset_fast(f, off, tab, invert, su.ID)
    assert np.array_equal(fast[0], out) and np.array_equal(fast[1], hits) and fast[2] == n


def test_consequences():
    f = slab(T=3, seed=2)
    assert (f <= 0).any() and (f == np.iinfo(np.int32).min).any()
    off, tab = su.table_by_id([])
    out, hits, n = su.subset(f, off, tab)
    assert not out.any() and n == 0 and len(hits) == 0
    out, hits, n = su.subset(f, off, tab, invert=True)
    assert np.array_equal(out, np.where(f > 0, f, 0)) and n == np.count_nonzero(f > 0)
    # an id listed at another step only is not found at this one
    f[:] = 0
    f[1, 0, 0] = 4
    off, tab = su.table_by_row([[4], [], [4]])
    out, hits, n = su.subset(f, off, tab)
    assert not out.any() and n == 0 and hits.tolist() == [0, 0]
    out, hits, n = su.subset(f, off, tab, invert=True)
    assert out[1, 0, 0] == 4 and n == 1 and hits.tolist() == [0, 0]


# ---- subset_table ---------------------------------------------------------------------------------------------------------------------
def test_subset_table_sorts_and_removes_duplicates():
    off, ids = subset_table([9, 3, 3, 5, 9])
    assert off.dtype == np.int64 and ids.dtype == np.int32 and off.tolist() == [0, 3] and ids.tolist() == [3, 5, 9]
    off, ids = subset_table(np.array([], dtype=np.int64))
    assert off.tolist() == [0, 0] and len(ids) == 0
    off, ids = subset_table(ids=[7, 2, 7, 5, 2 ** 31 - 1], steps=[3, 0, 3, 0, 1], T=5)
    assert off.tolist() == [0, 2, 3, 3, 4, 4] and ids.tolist() == [2, 5, 2 ** 31 - 1, 7]
    su.check_table(off, ids, 5)
    off, ids = subset_table(ids=[], steps=[], T=2)
    assert off.tolist() == [0, 0, 0] and len(ids) == 0


@pytest.mark.parametrize("kwargs", [dict(), dict(ids=[0]), dict(ids=[-3]), dict(ids=[2 ** 31]), dict(ids=[1.5]), dict(ids=[1], steps=[0]),
                                    dict(ids=[1], steps=[0], T=0), dict(ids=[1, 2], steps=[0], T=3), dict(ids=[1], steps=[3], T=3),
                                    dict(ids=[1], steps=[-1], T=3), dict(ids=[1], steps=[0.5], T=3)])
def test_subset_table_refuses(kwargs):
    with pytest.raises(ValueError):
        subset_table(**kwargs)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
FORMS = {name: i for i, name in enumerate(_native.SUBSET_FORMS)}


def test_forms_change_exactly_at_the_reported_capacities():
    caps = _native.subset_plan(False, 1, 1, 4, 8)
    bits, lds_ids = caps["bitmap_bits"], caps["lds_ids"]
    assert bits >= 64 and lds_ids >= 2
    form = lambda *a, **k: _native.subset_plan(*a, ny=4, nx=8, **k)["form"]
    # by id, no hits: a bitmap up to the largest id bits - 1, then a search by the number of ids
    assert form(False, bits - 2, 3) == form(False, bits - 1, 3) == FORMS["bitmap"] and form(False, bits, 3) == FORMS["search_lds"]
    assert form(False, bits - 1, lds_ids + 1) == FORMS["bitmap"]
    assert form(False, bits, lds_ids - 1) == form(False, bits, lds_ids) == FORMS["search_lds"] and form(False, bits, lds_ids + 1) == FORMS["search_glb"]
    assert form(False, 0, 0) == FORMS["bitmap"]
    # hits: never a bitmap
    assert form(False, 5, 3, hits=True) == FORMS["search_lds"]
    assert form(False, 2 ** 31 - 1, lds_ids, hits=True) == FORMS["search_lds"] and form(False, 2 ** 31 - 1, lds_ids + 1, hits=True) == FORMS["search_glb"]
    # rows: by the longest slice
    for hits in (False, True):
        assert form(True, 0, lds_ids - 1, hits=hits) == form(True, 0, lds_ids, hits=hits) == FORMS["row_lds"]
        assert form(True, 0, lds_ids + 1, hits=hits) == FORMS["row_glb"]
        assert form(True, 0, 0, hits=hits) == FORMS["row_lds"]
    # LDS of a workgroup
    assert _native.subset_plan(False, 31, 1, 4, 8)["lds"] == 4 and _native.subset_plan(False, 32, 1, 4, 8)["lds"] == 8
    assert _native.subset_plan(False, bits - 1, 1, 4, 8)["lds"] == bits // 8 <= 65536
    assert _native.subset_plan(False, bits, lds_ids, 4, 8)["lds"] == 4 * lds_ids and _native.subset_plan(False, bits, lds_ids, 4, 8, hits=True)["lds"] == 8 * lds_ids <= 65536
    assert _native.subset_plan(True, 0, lds_ids, 4, 8, hits=True)["lds"] == 8 * lds_ids
    assert _native.subset_plan(True, 0, lds_ids + 1, 4, 8)["lds"] == _native.subset_plan(False, bits, lds_ids + 1, 4, 8)["lds"] == 0


def test_vector_or_scalar_by_alignment_and_plane():
    for ny, nx, vec in ((1, 1, 0), (1, 3, 0), (3, 5, 0), (4, 8, 1), (1, 4, 1), (4, 3, 1), (2, 6, 1), (2, 3, 0), (181, 360, 1), (7, 9, 0)):
        p = _native.subset_plan(False, 9, 3, ny, nx, steps=3)
        assert (p["vec"], p["vpt"]) == (vec, 4 if vec else 1), (ny, nx)
        q = _native.subset_plan(False, 9, 3, ny, nx, steps=3, aligned=False)
        assert (q["vec"], q["vpt"]) == (0, 1), (ny, nx)
        lanes = ny * nx // p["vpt"]
        assert p["bps"] == -(-lanes // p["part_lanes"]) and p["blocks"] == 3 * p["bps"]


def test_grid_caps_and_xcd_mode():
    # by id: a workgroup takes as many parts as keep its table at table_share bytes per part -- one where the table is that small
    p = _native.subset_plan(False, 440, 440, 181, 360, steps=2707)
    share = p["table_share"]
    assert share >= 64 and p["lds"] <= share
    assert p["bps"] == 16 and p["blocks"] == 2707 * 16 and p["grid"] == p["blocks"] and p["xcd"] == 1
    for max_id, per_load in ((8 * share - 1, 1), (8 * share, 2), (16 * share - 1, 2), (16 * share, 3), (p["bitmap_bits"] - 1, p["bitmap_bits"] // 8 // share)):
        q = _native.subset_plan(False, max_id, 3, 181, 360, steps=2707)
        assert q["form"] == FORMS["bitmap"] and q["grid"] == -(-q["blocks"] // per_load), (max_id, per_load, q)
    q = _native.subset_plan(False, 2 ** 31 - 1, share // 8 + 1, 181, 360, steps=2707, hits=True)
    assert q["lds"] == share + 8 and q["grid"] == q["blocks"] // 2
    q = _native.subset_plan(False, 2 ** 31 - 1, p["lds_ids"] + 1, 181, 360, steps=2707)
    assert q["form"] == FORMS["search_glb"] and q["grid"] == q["blocks"]
    r = _native.subset_plan(True, 0, 5, 181, 360, steps=2707)
    assert r["blocks"] == p["blocks"] and r["grid"] == r["blocks"] and r["xcd"] == 1
    huge = _native.subset_plan(True, 0, 5, 721, 1440, steps=100000)
    assert huge["blocks"] > 2 ** 24 - 1 and huge["grid"] == 2 ** 24 - 1
    for by_row in (False, True):
        assert _native.subset_plan(by_row, 3, 3, 4, 8, steps=7)["grid"] == 7 and _native.subset_plan(by_row, 3, 3, 4, 8, steps=7)["xcd"] == 0
        assert _native.subset_plan(by_row, 3, 3, 4, 8, steps=7, grid_max=3)["grid"] == 3
        assert _native.subset_plan(by_row, 3, 3, 4, 8, steps=2, grid_max=3)["grid"] == 2
    assert _native.subset_plan(False, 3, 3, 4, 8, steps=2047)["xcd"] == 0 and _native.subset_plan(True, 3, 3, 4, 8, steps=2048)["xcd"] == 1
    assert _native.subset_plan(True, 0, p["lds_ids"], 181, 360, steps=2707, hits=True)["grid"] == r["blocks"]        # rows: a workgroup per part whatever the slice


def test_plan_hook_refuses():
    for args in ((False, -1, 1, 4, 8), (False, 2 ** 31, 1, 4, 8), (False, 1, -1, 4, 8), (False, 1, 1, 0, 8), (False, 1, 1, 4, 0), (False, 1, 1, 65536, 32768)):
        with pytest.raises(ValueError):
            _native.subset_plan(*args)
    with pytest.raises(ValueError):
        _native.subset_plan(False, 1, 1, 4, 8, steps=0)


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_subset_entries():
    """by tests/test_abi_exports.py's own route: its expression over the header text"""
    import test_abi_exports as tae
    prod, dbg = tae.declared("contrack_hip.h"), tae.declared("contrack_hip_debug.h")
    for n in ("ctk_subset", "ctk_subset_dev", "ctk_subset_cb"):
        assert n in prod and n in _native.EXPORTS and hasattr(_native.lib(), n), n
    for n in ("ctk_debug_subset_plan", "ctk_debug_set_subset", "ctk_debug_subset_form", "ctk_debug_time_subset"):
        assert n in dbg and n not in prod and hasattr(_native.lib(), n), n
    assert _native.ABI.constants["CTK_SUBSET_ID"] == su.ID == 0 and _native.ABI.constants["CTK_SUBSET_MASK"] == su.MASK == 1
    text = open(os.path.join(tae.INC, "contrack_hip.h")).read()
    assert re.search(r"ctk_subset_cb\([^;]*ctk_read_chunk_fn reader[^;]*ctk_write_chunk_fn writer", text, flags=re.S)
    tae.test_every_declared_entry_point_is_exported()
