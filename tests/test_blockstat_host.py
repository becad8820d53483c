"""The statement of ctk_blockstat_* (tests/blockstat_util.py) against numpy's own expressions and its documented consequences, the
rule ctk_blockstat_plan through its host-only hook, the header's new entries, and the columns calc_block_stats makes of the rows (the
rows themselves come from the statement here: the GPU is tests/test_gpu_blockstat*.py's).  No GPU."""
import os
import re

import numpy as np
import pytest

import blockstat_util as bu
import minixr
import subset_util as su
from contrack_amd import _native
from contrack_amd import contrack as cm

minixr.install_as_xarray()
NAN = float("nan")


def slab(T=4, ny=5, nx=11, seed=0, top=6, dtype=np.float32):
    """ids 1 .. top on half the pixels, background 0, -1 and INT32_MIN; a field of distinct values with a few NaN"""
    rng = np.random.default_rng(seed)
    f = rng.integers(1, top + 1, size=(T, ny, nx)).astype(np.int32)
    f[rng.random(f.shape) < 0.5] = 0
    f.reshape(-1)[:3] = (0, -1, np.iinfo(np.int32).min)
    x = rng.permutation(f.size).reshape(f.shape).astype(dtype) - f.size // 2      # distinct, both signs, no +-0 pair
    x[rng.random(f.shape) < 0.1] = NAN
    return f, x


def gap_by_brute_force(occ):
    """(west, width) by trying every start and every length: the longest circular stretch of empty columns bounded by occupied ones"""
    nx = len(occ)
    if occ.all():
        return 0, nx
    for ln in range(nx - 1, 0, -1):
        for s in range(nx):
            cols = [(s + k) % nx for k in range(ln)]
            if not occ[cols].any() and occ[(s - 1) % nx] and occ[(s + ln) % nx]:
                return (s + ln) % nx, nx - ln
    raise AssertionError("an occupancy with a free column has a run")


# ---- the statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_statement_is_nanmax_nanargmax_and_the_brute_force_gap(dtype):
    f, x = slab(dtype=dtype)
    T, ny, nx = f.shape
    slices = [[1, 2, 3], [], [2, 6, 9], [1, 2, 3, 4, 5, 6]]
    off, ids = su.table_by_row(slices)
    rows = bu.blockstat(f, x, off, ids)
    assert rows.dtype == bu.ROW and len(rows) == len(ids)
    seen = valid = 0
    for t, s in enumerate(slices):
        for k, i in enumerate(s):
            r = rows[off[t] + k]
            P = np.flatnonzero(f[t].reshape(-1) == i)
            assert r["n"] == len(P)
            if not len(P):
                continue
            seen += 1
            v = x[t].reshape(-1)[P]
            assert (r["r0"], r["r1"]) == (P.min() // nx, P.max() // nx)
            occ = np.zeros(nx, dtype=bool)
            occ[P % nx] = True
            assert (r["west"], r["width"]) == gap_by_brute_force(occ), (t, i)
            assert r["nv"] == np.count_nonzero(~np.isnan(v))
            if not r["nv"]:
                assert np.isnan(r["max"]) and np.isnan(r["min"]) and r["max_p"] == r["min_p"] == -1
                continue
            valid += 1
            assert r["max"] == np.nanmax(v) and r["max_p"] == P[np.nanargmax(v)]
            assert r["min"] == np.nanmin(v) and r["min_p"] == P[np.nanargmin(v)]
    assert seen >= 8 and valid >= 8 and (rows["n"] == 0).any()
    hits = su.subset(f, off, ids)[1]
    assert np.array_equal(rows["n"].astype(np.uint64), hits)                      # n is ctk_subset_*'s hits for the same table


def test_want_leaves_the_rest_empty():
    f, x = slab(seed=1)
    off, ids = su.table_by_row([[1, 2], [3], [4, 5], [6]])
    both, shape, peaks = (bu.blockstat(f, x, off, ids, w) for w in (bu.SHAPE | bu.PEAKS, bu.SHAPE, bu.PEAKS))
    assert bu.same_rows(bu.blockstat(f, None, off, ids, bu.SHAPE), shape)
    empty = bu.empty_rows(len(ids))
    for name in bu.ROW.names:
        a = lambda r: r[name].view(np.uint64) if name in ("max", "min") else r[name]
        in_shape, in_peaks = name in ("r0", "r1", "west", "width"), name in ("nv", "max", "min", "max_p", "min_p")
        assert np.array_equal(a(shape), a(empty) if in_peaks else a(both)), name
        assert np.array_equal(a(peaks), a(empty) if in_shape else a(both)), name


def one_block(cols, nx=12, rows=(1,), ny=3):
    f = np.zeros((1, ny, nx), dtype=np.int32)
    for r in rows:
        f[0, r, list(cols)] = 7
    return f


def test_consequences():
    tab = su.table_by_row([[7]])
    ext = lambda cols, **k: tuple(int(bu.blockstat(one_block(cols, **k), None, *tab, want=bu.SHAPE)[0][n]) for n in ("west", "width"))
    assert ext(range(12)) == (0, 12)                                               # a full circle
    assert ext([5]) == (5, 1) and ext([0]) == (0, 1) and ext([11]) == (11, 1)      # a single column
    assert ext([10, 11, 0, 1]) == (10, 4)                                          # over the seam: not 12 columns wide
    assert ext([0, 1, 2, 9]) == (9, 6)                                             # the gap 3 .. 8 wins over 10 .. 11
    assert ext([2, 3, 8, 9]) == (8, 8)                                             # the gap that passes the seam (10 .. 1: 4 columns) ties with 4 .. 7: s = 4 is lower
    assert ext([0, 6]) == (6, 7)                                                   # gaps 1 .. 5 and 7 .. 11, equally long: the lower start s = 1 wins
    assert ext([3, 9]) == (9, 7)                                                   # gaps 4 .. 8 (s = 4) and 10 .. 2 (s = 10): s = 4 wins
    assert ext([1, 10]) == (10, 4)                                                 # the gap 2 .. 9 is the longest: the block spans the seam
    # an absent entry, and an entry whose values are all NaN
    f = one_block([4, 5])
    x = np.full(f.shape, NAN, dtype=np.float32)
    rows = bu.blockstat(f, x, *su.table_by_row([[3, 7]]))
    assert bu.same_rows(rows[:1], bu.empty_rows(1))
    r = rows[1]
    assert (r["n"], r["nv"], r["r0"], r["r1"], r["west"], r["width"], r["max_p"], r["min_p"]) == (2, 0, 1, 1, 4, 2, -1, -1) and np.isnan(r["max"]) and np.isnan(r["min"])
    # -0.0 sorts below +0.0 whichever comes first, and the first of equal keys wins
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        x = np.full(f.shape, NAN, dtype=np.float64)
        x[0, 1, 4], x[0, 1, 5] = first, second
        r = bu.blockstat(f, x, *tab)[0]
        assert np.signbit(r["min"]) and not np.signbit(r["max"]) and r["min"] == r["max"] == 0
        assert (r["max_p"], r["min_p"]) == ((17, 16) if first < second or np.signbit(first) else (16, 17))
    x = np.zeros(f.shape, dtype=np.float32)
    r = bu.blockstat(f, x, *tab)[0]
    assert (r["max_p"], r["min_p"]) == (16, 16)
    # float64 values that differ only below float32 precision stay apart; a float32 value widens exactly
    x = np.zeros(f.shape, dtype=np.float64)
    x[0, 1, 4], x[0, 1, 5] = 1.0, 1.0 + 2.0 ** -40
    r = bu.blockstat(f, x, *tab)[0]
    assert np.float32(x[0, 1, 4]) == np.float32(x[0, 1, 5]) and (r["max_p"], r["min_p"], r["max"]) == (17, 16, 1.0 + 2.0 ** -40)
    tiny = np.float32(1e-45)
    x = np.zeros(f.shape, dtype=np.float32)
    x[0, 1, 4], x[0, 1, 5] = tiny, -tiny
    r = bu.blockstat(f, x, *tab)[0]
    assert tiny > 0 and (r["max"], r["min"]) == (float(tiny), -float(tiny)) and (r["max_p"], r["min_p"]) == (16, 17)


def test_key_is_a_total_order():
    vals = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], dtype=np.float32)
    for dt in (np.float32, np.float64):
        keys = [bu.key(v) for v in vals.astype(dt)]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
FORMS = {name: i for i, name in enumerate(_native.BLOCKSTAT_FORMS)}


@pytest.mark.parametrize("nx", [35, 104, 360, 1440])
@pytest.mark.parametrize("want", ["shape", "peaks", ("shape", "peaks")])
def test_forms_change_exactly_at_the_lds_budget(nx, want):
    p = _native.blockstat_plan(want, 1, 2, nx)
    words = 0 if want == "peaks" else -(-nx // 32)
    assert p["words"] == words and p["entry"] == 36 + 4 * words and p["lds_budget"] == 32 << 10
    cap = p["lds_entries"]
    assert cap == p["lds_budget"] // p["entry"] and cap * p["entry"] <= p["lds_budget"] < (cap + 1) * p["entry"]
    for longest, form in ((0, "row_lds"), (1, "row_lds"), (cap - 1, "row_lds"), (cap, "row_lds"), (cap + 1, "row_glb"), (10 * cap, "row_glb")):
        q = _native.blockstat_plan(want, longest, 2, nx)
        assert q["form"] == FORMS[form], (longest, q)
        assert q["lds"] == (longest * p["entry"] if form == "row_lds" else 0) <= p["lds_budget"]
    # several workgroups of a CU's 160 KB still fit
    assert 5 * p["lds_budget"] <= 160 << 10


def test_vector_or_scalar_parts_and_passes():
    for ny, nx, vec in ((1, 1, 0), (1, 3, 0), (3, 5, 0), (4, 8, 1), (1, 4, 1), (4, 3, 1), (2, 3, 0), (40, 104, 1), (33, 35, 0), (181, 360, 1)):
        p = _native.blockstat_plan(("shape", "peaks"), 3, ny, nx, steps=3)
        assert (p["vec"], p["vpt"]) == (vec, 4 if vec else 1), (ny, nx)
        q = _native.blockstat_plan(("shape", "peaks"), 3, ny, nx, steps=3, aligned=False)
        assert (q["vec"], q["vpt"]) == (0, 1), (ny, nx)
        lanes = -(-ny * nx // p["vpt"])
        assert p["bps"] == -(-lanes // p["part_lanes"]) and p["blocks"] == 3 * p["bps"] == p["grid"] and p["xcd"] == 0
    assert _native.blockstat_plan("shape", 3, 40, 104)["bps"] == 2 and _native.blockstat_plan("shape", 3, 33, 35)["bps"] == 2
    assert _native.blockstat_plan("shape", 3, 181, 360, steps=2707)["xcd"] == 1
    assert _native.blockstat_plan("shape", 3, 4, 8, steps=7, grid_max=3)["grid"] == 3
    # float64 peaks take a second launch; nothing else does
    for want, eb, passes in (("shape", 4, 1), ("shape", 8, 1), ("peaks", 4, 1), ("peaks", 8, 2), (("shape", "peaks"), 4, 1), (("shape", "peaks"), 8, 2)):
        assert _native.blockstat_plan(want, 3, 4, 8, elem_bytes=eb)["passes"] == passes


def test_plan_hook_and_want_refuse():
    for kw in (dict(want=0), dict(want=4), dict(want=7), dict(longest=-1), dict(ny=0), dict(nx=0), dict(steps=0), dict(elem_bytes=2), dict(ny=65536, nx=32768)):
        args = dict(want=3, longest=1, ny=4, nx=8)
        args.update(kw)
        with pytest.raises(ValueError):
            _native.blockstat_plan(**args)
    for want in ("extent", (), ("shape", "peak"), None):
        with pytest.raises((ValueError, TypeError)):
            _native._block_want(want)
    assert _native._block_want("shape") == bu.SHAPE and _native._block_want(("peaks", "shape", "peaks")) == bu.SHAPE | bu.PEAKS


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_blockstat_entries():
    """by tests/test_abi_exports.py's own route: its expression over the header text"""
    import test_abi_exports as tae
    prod, dbg = tae.declared("contrack_hip.h"), tae.declared("contrack_hip_debug.h")
    for n in ("ctk_blockstat_f32", "ctk_blockstat_f64", "ctk_blockstat_f32_dev", "ctk_blockstat_f64_dev", "ctk_blockstat_cb"):
        assert n in prod and n in _native.EXPORTS and hasattr(_native.lib(), n), n
    for n in ("ctk_debug_blockstat_plan", "ctk_debug_set_blockstat", "ctk_debug_blockstat_form", "ctk_debug_time_blockstat"):
        assert n in dbg and n not in prod and hasattr(_native.lib(), n), n
    assert _native.ABI.constants["CTK_BLOCK_SHAPE"] == bu.SHAPE == 1 and _native.ABI.constants["CTK_BLOCK_PEAKS"] == bu.PEAKS == 2
    assert _native.BLOCK_ROW == bu.ROW and _native.BLOCK_ROW.itemsize == 56         # the struct as the header has it is the statement's row
    assert [n for n, _ in _native.ABI.structs["ctk_block_row"]] == list(bu.ROW.names)
    text = open(os.path.join(tae.INC, "contrack_hip.h")).read()
    assert re.search(r"ctk_blockstat_cb\([^;]*ctk_read_chunk_fn flag_reader[^;]*ctk_read_chunk_fn field_reader[^;]*ctk_block_row \*rows", text, flags=re.S)
    assert "Barriopedro" in text and "Dunn-Sigouin" in text and "np.argmax(np.diff(cols))" in text
    tae.test_every_declared_entry_point_is_exported()


# ---- calc_block_stats: the columns it makes of the rows ---------------------------------------------------------------------------------
T, NY, NX = 3, 6, 12
LAT, LON = 75.0 - 10.0 * np.arange(NY), 30.0 * np.arange(NX)


def hand_made():
    """block 5 sits over the seam at steps 0 and 1, block 9 in mid-plane at step 1"""
    f = np.zeros((T, NY, NX), dtype=np.int32)
    f[0, 1:3, [11, 0, 1]] = 5
    f[1, 2, [10, 11, 0]] = 5
    f[1, 3:5, 4:7] = 9
    x = (np.arange(f.size, dtype=np.float32).reshape(f.shape) % 17) - 8
    x[0, 1, 0] = 50.0
    x[1, 4, 5] = -50.0
    x[1, 3, 4] = NAN
    return f, x


def instance(monkeypatch, dims=("time", "latitude", "longitude")):
    import pandas as pd
    f, x = hand_made()
    time = (np.datetime64("2001-01-01") + np.arange(T)).astype("datetime64[D]").astype("datetime64[ns]")
    ds = minixr.make_dataset(x, LAT, LON, time=time)
    ds["time"].attrs = {}
    canon = ("time", "latitude", "longitude")
    ds["flag"] = minixr.DataArray(f.transpose([canon.index(d) for d in dims]), dims, attrs={"units": "1"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    calls = []

    def by_statement(flag, table, x=None, want=('shape', 'peaks'), chunk_steps=None, device=None, shape=None, dtype=None):
        calls.append((want, chunk_steps))
        if callable(flag):
            got = np.empty(shape, dtype=np.int32)
            flag(0, shape[0], got)
            flag = got
        if callable(x):
            got = np.empty(shape, dtype=dtype)
            x(0, shape[0], got)
            x = got
        return bu.blockstat(flag, x, *table, want=_native._block_want(want))
    monkeypatch.setattr(cm, "blockstat_numpy", by_statement)
    frame = pd.DataFrame({"Flag": [9, 5, 5], "Date": ["b", "a", "b"], "Step": [1, 0, 1]})
    return c, f, x, frame, calls


@pytest.mark.parametrize("chunk", [None, 2])
@pytest.mark.parametrize("dims", [("time", "latitude", "longitude"), ("latitude", "time", "longitude")])
def test_calc_block_stats_columns(monkeypatch, dims, chunk):
    c, f, x, frame, calls = instance(monkeypatch, dims)
    df = c.calc_block_stats("flag", "anom", frame=frame, chunk_steps=chunk, indices=True)
    assert calls == [(('shape', 'peaks'), chunk)]
    assert list(df.columns) == ['Flag', 'Date', 'Step', 'N', 'South', 'North', 'LatExtent', 'West', 'East', 'LonExtent', 'Max', 'MaxLatitude', 'MaxLongitude',
                                'Min', 'MinLatitude', 'MinLongitude', 'Row0', 'Row1', 'ColWest', 'Width', 'NValid', 'MaxRow', 'MaxCol', 'MinRow', 'MinCol']
    assert df["Flag"].tolist() == [9, 5, 5] and df["Step"].tolist() == [1, 0, 1] and df["Date"].tolist() == ["b", "a", "b"]      # the frame's order
    assert df["N"].tolist() == [6, 6, 3] and df["NValid"].tolist() == [5, 6, 3]
    assert df["South"].tolist() == [LAT[3], LAT[1], LAT[2]] and df["North"].tolist() == [LAT[4], LAT[2], LAT[2]]
    assert df["LatExtent"].tolist() == [20.0, 20.0, 10.0]
    assert df["West"].tolist() == [120.0, 330.0, 300.0] and df["East"].tolist() == [180.0, 30.0, 0.0] and df["LonExtent"].tolist() == [90.0, 90.0, 90.0]
    assert df["Max"].tolist()[1] == 50.0 and (df["MaxLatitude"][1], df["MaxLongitude"][1]) == (LAT[1], LON[0])
    assert df["Min"].tolist()[0] == -50.0 and (df["MinLatitude"][0], df["MinLongitude"][0]) == (LAT[4], LON[5])
    assert (df["MinRow"][0], df["MinCol"][0], df["ColWest"][1], df["Width"][1], df["Row0"][2], df["Row1"][2]) == (4, 5, 11, 3, 2, 2)
    for i, (t, b) in enumerate(zip(frame["Step"], frame["Flag"])):
        v = x[t][f[t] == b]
        assert df["Max"][i] == np.nanmax(v) and df["Min"][i] == np.nanmin(v)
    shape_only = c.calc_block_stats("flag", frame=frame, chunk_steps=chunk)
    assert list(shape_only.columns) == list(df.columns)[:10] and shape_only.equals(df[list(df.columns)[:10]])
    assert calls[-1] == (('shape',), chunk)


def test_calc_block_stats_checks_the_frame(monkeypatch):
    c, f, x, frame, calls = instance(monkeypatch)
    foreign = frame.copy()
    foreign.loc[0, "Step"] = 2                                                      # block 9 is not there at step 2
    with pytest.raises(ValueError, match=r"another run.*|.*\(step 2, id 9\)"):
        c.calc_block_stats("flag", "anom", frame=foreign)
    df = c.calc_block_stats("flag", "anom", frame=foreign, check=False, indices=True)
    assert df["N"].tolist() == [0, 6, 3] and np.isnan(df["South"][0]) and np.isnan(df["West"][0]) and np.isnan(df["Max"][0]) and np.isnan(df["MaxLatitude"][0])
    assert (df["LatExtent"][0], df["LonExtent"][0], df["Row0"][0], df["ColWest"][0], df["Width"][0], df["MaxRow"][0], df["MinCol"][0]) == (0, 0, -1, -1, 0, -1, -1)
    for bad in (frame[["Flag"]], frame.assign(Step=[0, 1, T]), frame.assign(Flag=[0, 5, 5])):
        with pytest.raises(ValueError):
            c.calc_block_stats("flag", "anom", frame=bad)
    with pytest.raises(ValueError):
        c.calc_block_stats("flag")                                                 # no frame and no variable to make one from
    c.ds["flag"] = minixr.DataArray(f.astype(np.float32), ("time", "latitude", "longitude"))
    with pytest.raises(ValueError):
        c.calc_block_stats("flag", "anom", frame=frame)
