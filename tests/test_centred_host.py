"""The host side of the block-centred composite (include/contrack_hip.h, "block-centred composites"): the entries are declared,
exported and bound; the launch rule against its restatement (tests/centred_util.py); lifecycle_bins for every `by`; the stable time
sort of the stamps; the Step / Row / Col columns of lifecycle_columns; and the proof that the numpy statement the GPU tests compare
with can see a reversed stamp order, a float32 accumulator and a split of a bin's stamps.  No GPU is needed."""
import itertools
import os
import re

import numpy as np
import pytest

import centred_util as cu
from contrack_amd import _native
from contrack_amd.contrack import centred_numpy, centred_stamps, contrack, lifecycle_bins, lifecycle_columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ["ctk_centred_f32_dev", "ctk_centred_f64_dev", "ctk_centred_f32", "ctk_centred_f64", "ctk_centred_cb"]
DEBUG = ["ctk_debug_centred_plan", "ctk_debug_set_centred", "ctk_debug_centred_launch", "ctk_debug_time_centred"]


# ---- declared, exported, bound ----------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    lib = _native.lib()
    prod = open(os.path.join(ROOT, "include", "contrack_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "contrack_hip_debug.h")).read()
    for name in PRODUCT:
        assert re.search(r"^int %s\(" % name, prod, flags=re.M), name
    for name in DEBUG:
        assert re.search(r"^int %s\(" % name, dbg, flags=re.M), name
    assert "README.rst:198-228" in prod and "for r = 0 .. R-1, RISING" in prod
    for name in PRODUCT + DEBUG:
        assert name in _native.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("centred", "centred_cb", "centred_dev", "debug_set_centred", "debug_centred_launch", "time_centred"):
        assert callable(getattr(_native.Tracker, name)), name
    assert callable(_native.centred_plan)
    import contrack_amd
    assert contrack_amd.centred_numpy is centred_numpy and contrack_amd.lifecycle_bins is lifecycle_bins
    assert callable(contrack.calc_centred_composite)


# ---- the launch rule --------------------------------------------------------------------------------------------------------------
def test_centred_plan_is_the_restated_rule():
    seen = set()
    windows = ((0, 0), (0, 1), (3, 4), (2, 6), (0, 31), (0, 32), (7, 8), (6, 10), (20, 40), (80, 160))
    stamps = ((0, 0), (1, 1), (127, 127), (128, 128), (127, 5000), (128, 5000), (614, 5681), (3610, 33294), (10 ** 6, 10 ** 9))
    for eb, nbins, (hy, hx), (max_bin, kept), form in itertools.product((4, 8), (1, 2, 16, 39, 40, 402, 2048, 2049), windows, stamps, (-1, 0, 1)):
        for unroll, threads in ((-1, -1), (1, 1), (2, 64), (3, 127), (4, 128), (8, 255), (16, 256), (31, 1024), (32, -1), (99, -1)):
            got = _native.centred_plan(eb, nbins, hy, hx, max_bin, kept, form, unroll, threads)
            want = cu.plan(eb, nbins, hy, hx, max_bin, kept, form, unroll, threads)
            assert got == want, (eb, nbins, hy, hx, max_bin, kept, form, unroll, threads, got, want)
            seen.add((got["form"], got["unroll"], got["threads"], form))
    assert {u for f, u, th, _ in seen if f == 0} == {1, 2, 4, 8, 16, 32} and {th for f, u, th, _ in seen if f == 0} == {64, 128, 256}
    assert {(u, th) for f, u, th, _ in seen if f == 1} == {(8, 64), (4, 64)}
    assert {f for f, u, th, forced in seen if forced == -1} == {0, 1}                     # the rule itself takes both forms
    # plain: 128 bytes of values per lane in flight, 32 float32 stamps or 16 float64; fed: 32 bytes per feeder lane, 8 or 4
    assert _native.centred_plan(4, 1, 20, 40) == dict(form=0, unroll=32, threads=64, parts=52, blocks=52, grid=52)
    assert _native.centred_plan(8, 1, 20, 40)["unroll"] == 16
    assert _native.centred_plan(4, 1, 20, 40, 33294) == dict(form=1, unroll=8, threads=64, parts=52, blocks=52, grid=52)
    assert _native.centred_plan(8, 1, 20, 40, 33294)["unroll"] == 4
    # the form: the six measured workloads of tools/centred_probe.py (1 degree and a quarter degree; one bin, ages below 16, all ages)
    # go where they ran faster
    assert _native.centred_plan(4, 1, 20, 40, 33294, 33294)["form"] == 1                  # 0.77 ms fed, 5.96 plain
    assert _native.centred_plan(4, 16, 20, 40, 3610, 30000)["form"] == 1                  # 0.13 fed, 0.65 plain
    assert _native.centred_plan(4, 410, 20, 40, 3610, 33294)["form"] == 1                 # 0.21 fed, 0.72 plain
    assert _native.centred_plan(4, 1, 80, 160, 5681, 5681)["form"] == 1                   # 0.38 fed, 1.06 plain
    assert _native.centred_plan(4, 16, 80, 160, 614, 5000)["form"] == 0                   # 0.33 fed, 0.19 plain
    assert _native.centred_plan(4, 402, 80, 160, 614, 5681)["form"] == 0                  # 1.53 fed, 0.35 plain
    # a bin of less than 128 stamps stays with the plain form
    assert [_native.centred_plan(4, 1, 20, 40, m)["form"] for m in (127, 128)] == [0, 1]
    # plain: single waves up to 2048 of them, 256 cells per workgroup beyond: 39 bins of a 41 x 81 window are 2028 waves, 40 are 2080
    assert _native.centred_plan(4, 39, 20, 40) == dict(form=0, unroll=32, threads=64, parts=52, blocks=2028, grid=2028)
    assert _native.centred_plan(4, 40, 20, 40) == dict(form=0, unroll=32, threads=256, parts=13, blocks=520, grid=520)
    assert [_native.centred_plan(4, n, 0, 0)["threads"] for n in (2048, 2049)] == [64, 256]
    # one cell below, at and above a workgroup's share of a bin: 63, 65 (no window has 64 cells: both sides are odd), 255, 273
    assert [_native.centred_plan(4, 1, hy, hx)["parts"] for hy, hx in ((3, 4), (2, 6))] == [1, 2]
    assert [_native.centred_plan(4, 1, hy, hx, form=1)["parts"] for hy, hx in ((3, 4), (2, 6))] == [1, 2]
    assert [_native.centred_plan(4, 1, hy, hx, threads=256)["parts"] for hy, hx in ((7, 8), (6, 10))] == [1, 2]
    for bad in ((2, 1, 0, 0), (4, 0, 0, 0), (4, 1, -1, 0), (4, 1, 0, -1), (4, 2, 16383, 32767), (4, 1, 0, 0, -1), (4, 1, 0, 0, 5, 4)):
        with pytest.raises(ValueError):
            _native.centred_plan(*bad)


# ---- lifecycle_bins ---------------------------------------------------------------------------------------------------------------
# block 7: steps 3, 4, 6, 7 (a gap at 5: duration 5); block 9: one row at step 9; block 2: steps 0 .. 5; the rows are not sorted
BLOCK = np.array([7, 2, 7, 9, 2, 2, 7, 2, 2, 7, 2])
STEP = np.array([3, 0, 4, 9, 1, 2, 6, 3, 4, 7, 5])


def test_lifecycle_bins_age_and_to_lysis():
    b, nb = lifecycle_bins(BLOCK, STEP, "age")
    assert b.dtype == np.int32 and nb == 6
    assert b.tolist() == [0, 0, 1, 0, 1, 2, 3, 3, 4, 4, 5]                      # block 7 at step 6 has age 3: the gap counts
    b, nb = lifecycle_bins(BLOCK, STEP, "to_lysis")
    assert nb == 6 and b.tolist() == [4, 5, 3, 0, 4, 3, 1, 2, 1, 0, 0]
    b, nb = lifecycle_bins(BLOCK, STEP, "age", max_age=3)                       # cut: later rows are dropped
    assert nb == 4 and b.tolist() == [0, 0, 1, 0, 1, 2, 3, 3, -1, -1, -1]
    b2, nb2 = lifecycle_bins(BLOCK, STEP, "age", nbins=4)
    assert nb2 == 4 and b2.tolist() == b.tolist()
    b, nb = lifecycle_bins(BLOCK, STEP, "to_lysis", max_age=0)
    assert nb == 1 and b.tolist() == [-1, -1, -1, 0, -1, -1, -1, -1, -1, 0, 0]
    b, nb = lifecycle_bins(BLOCK, STEP, "age", max_age=8)                       # a longer axis than any block: empty bins
    assert nb == 9 and b.max() == 5
    with pytest.raises(ValueError):
        lifecycle_bins(BLOCK, STEP, "age", nbins=4, max_age=5)


def test_lifecycle_bins_normalized():
    b, nb = lifecycle_bins(BLOCK, STEP, "normalized", nbins=5)
    # block 7 (duration 5): ages 0, 1, 3, 4 -> 0, 1, 3, 4; block 9 (duration 1): 0; block 2 (duration 6): ages 0..5 -> 0, 0, 1, 2, 3, 4
    assert nb == 5 and b.tolist() == [0, 0, 1, 0, 0, 1, 3, 2, 3, 4, 4]
    b, nb = lifecycle_bins(BLOCK, STEP, "normalized", nbins=10)                 # duration < nbins: bins stay empty, none is out of range
    assert nb == 10 and b.tolist() == [0, 0, 2, 0, 1, 3, 6, 5, 6, 8, 8] and b.max() < 10
    with pytest.raises(ValueError, match="nbins"):
        lifecycle_bins(BLOCK, STEP, "normalized")


def test_lifecycle_bins_none_array_and_keys():
    b, nb = lifecycle_bins(BLOCK, STEP, None)
    assert nb == 1 and b.tolist() == [0] * 11 and b.dtype == np.int32
    given = np.array([2, -1, 0, 5, -7, 1, 1, 0, 0, 3, 2])
    b, nb = lifecycle_bins(BLOCK, STEP, given)
    assert nb == 6 and b.tolist() == given.tolist() and b.dtype == np.int32
    assert lifecycle_bins(BLOCK, STEP, given, nbins=9)[1] == 9
    with pytest.raises(ValueError):
        lifecycle_bins(BLOCK, STEP, given, nbins=5)
    with pytest.raises(ValueError):
        lifecycle_bins(BLOCK, STEP, "onset")
    # (Flag, member) keys: the same id in two members is two blocks
    keys = [(1, 0), (1, 1), (1, 0), (1, 1)]
    assert lifecycle_bins(keys, np.array([2, 7, 3, 9]), "age")[0].tolist() == [0, 0, 1, 2]
    assert lifecycle_bins(np.array(keys), np.array([2, 7, 3, 9]), "age")[0].tolist() == [0, 0, 1, 2]
    assert lifecycle_bins([1, 1, 1, 1], np.array([2, 7, 3, 9]), "age")[0].tolist() == [0, 5, 1, 7]
    b, nb = lifecycle_bins([], np.zeros(0, np.int64), "age")
    assert nb == 1 and b.shape == (0,)


# ---- the stamps -------------------------------------------------------------------------------------------------------------------
def test_stamps_are_sorted_stably_by_time():
    t = np.array([5, 2, 5, 0, 2, 5, 2])
    row = np.arange(7)
    col = np.arange(7) * 10
    bin = np.array([0, 1, 2, -1, 1, 0, 2])
    st, sr, sc, sb = centred_stamps(t, row, col, bin)
    assert st.tolist() == [0, 2, 2, 2, 5, 5, 5]
    assert sr.tolist() == [3, 1, 4, 6, 0, 2, 5]                                 # the given order among equal t
    assert sc.tolist() == [30, 10, 40, 60, 0, 20, 50] and sb.tolist() == [-1, 1, 1, 2, 0, 2, 0]
    assert centred_stamps(t, row, col)[3].tolist() == [0] * 7                   # bin None: one bin
    with pytest.raises(ValueError, match="one length"):
        centred_stamps(t, row[:5], col, bin)
    with pytest.raises(ValueError, match="integers"):
        centred_stamps(t.astype(np.float64), row, col, bin)
    with pytest.raises(ValueError, match="a reader needs"):
        centred_numpy(lambda t0, nt, out: None, t, row, col)


def test_lifecycle_columns_give_the_grid_indices():
    """Row / Col are the indices whose coordinates the truncated Latitude / Longitude came from, Step the position in time"""
    lat, lon = np.arange(30.5, 40.5, 1.0), np.arange(-5.25, 6.75, 1.0)         # 10 x 12
    dates = ["d%02d" % k for k in range(6)]
    rows = np.zeros(3, dtype=_native.LIFE_ROW)
    rows["t"], rows["label"], rows["shift"] = [4, 1, 5], [3, 3, 8], [0, 5, 0]
    rows["area"], rows["swv"] = 2.0, 4.0
    rows["swvy"], rows["swvx"] = [4.0 * 2.75, 4.0 * 9.5, 4.0 * 0.25], [4.0 * 3.5, 4.0 * 8.25, 4.0 * 11.75]
    plain = lifecycle_columns(rows, lat, lon, dates)
    assert list(plain) == ["Flag", "Date", "Longitude", "Latitude", "Intensity", "Size"]
    cols = lifecycle_columns(rows, lat, lon, dates, indices=True)
    assert list(cols) == list(plain) + ["Step", "Row", "Col"]
    for k in plain:
        assert np.array_equal(plain[k], cols[k])
    assert cols["Step"].tolist() == [4, 1, 5] and cols["Row"].tolist() == [2, 9, 0] and cols["Col"].tolist() == [3, (8 + 5) % 12, 11]
    for k in ("Step", "Row", "Col"):
        assert cols[k].dtype == np.int64
    assert np.array_equal(cols["Latitude"], np.trunc(lat[cols["Row"]]).astype(np.int64))
    assert np.array_equal(cols["Longitude"], np.trunc(lon[cols["Col"]]).astype(np.int64))
    member = lifecycle_columns(rows, lat, lon, dates[:3], period=3, indices=True)
    assert member["Member"].tolist() == [1, 0, 1] and member["Step"].tolist() == [1, 1, 2]


# ---- the statement has teeth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_discriminating_inputs_discriminate(dtype, seed):
    """T = 23, grid 7 x 12, 40 stamps in 3 bins, window 5 x 7, x = normal x 10**uniform(-8, 10) cast to the dtype: the statement differs
    from each of order="falling", acc="float32" and slice=4 in at least one cell -- the condition under which a GPU test that passes
    on this input cannot be blind to a reversed order, a float32 accumulator or a split of a bin's stamps"""
    x, t, row, col, bin = cu.wide_case(dtype, seed=seed)
    assert x.shape == (23, 7, 12) and x.dtype == dtype and len(t) == 40 and (np.diff(t) >= 0).all() and bin.min() == -1 and bin.max() == 2
    want, n = cu.centred(x, t, row, col, bin, 3, 2, 3)
    assert want.dtype == np.float64 and n.dtype == np.uint32 and want.shape == (3, 5, 7) and not np.isnan(want).any()
    assert n[:, 2, 3].tolist() == np.bincount(bin[bin >= 0], minlength=3).tolist()            # the centre cell is never clipped
    figures = {}
    for name, kw in (("falling", dict(order="falling")), ("float32", dict(acc="float32")), ("slice4", dict(slice=4))):
        other, n2 = cu.centred(x, t, row, col, bin, 3, 2, 3, **kw)
        assert np.array_equal(n, n2)
        figures[name] = cu.differing(want, other)
    print("cells of %d that differ from the statement (%s, seed %d): %s" % (want.size, np.dtype(dtype).name, seed, figures))
    assert all(v > 0 for v in figures.values()), figures
    assert cu.same_bits(want, cu.centred(x, t, row, col, bin, 3, 2, 3, slice=40)[0])
    # an independent statement of the same sums, cell by cell in plain Python
    s2 = np.zeros((3, 5, 7))
    for r in range(40):
        if bin[r] < 0:
            continue
        for j in range(-2, 3):
            for i in range(-3, 4):
                y = row[r] + j
                if 0 <= y < 7:
                    s2[bin[r], j + 2, i + 3] += np.float64(x[t[r], y, (col[r] + i) % 12])
    assert cu.same_bits(want, s2)


def test_statement_rules():
    x = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    x[1, 0, 0] = np.nan
    t, row, col, bin = np.array([0, 1, 1]), np.array([0, 0, 2]), np.array([0, 3, 1]), np.array([0, 0, -1])
    s, n = cu.centred(x, t, row, col, bin, 2, 1, 1)
    assert n[0].tolist() == [[0, 0, 0], [2, 2, 2], [2, 2, 2]] and (n[1] == 0).all()           # the row over the pole is not counted
    assert (s[1] == 0.0).all() and not np.signbit(s[1]).any() and s[0, 0, 0] == 0.0
    assert s[0, 1, 0] == x[0, 0, 3] + x[1, 0, 2] and np.isnan(s[0, 1, 2])                     # wrapped columns; a NaN makes its cell NaN
    s, n = cu.centred(x, t, row, col, bin, 2, 1, 1, skipna=True)
    assert s[0, 1, 2] == x[0, 0, 1] and n[0, 1, 2] == 1
    s, n = cu.centred(x, t, row, col, bin, 2, 1, 1, wrap=False)
    assert n[0].tolist() == [[0, 0, 0], [1, 2, 1], [1, 2, 1]]                                 # col -1 and col 4 are not counted
