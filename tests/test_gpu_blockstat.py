"""ctk_blockstat_* on the GPU against its statement tests/blockstat_util.py: the device, host-array and callback paths and
blockstat_numpy, both field types, the three values of `want`, chunking, offset device pointers, both kernel forms reached by size
alone, the resident field and every error case.  Integers and selected values only: equality everywhere, bit for bit for the two
floats.  The slabs are built by hand, the smallest that reach each mechanism, and every case asserts its own precondition -- the tie
exists, the block crosses the part boundary, the launch took the form it was meant to reach."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import blockstat_util as bu
import reversal_util as ru
import subset_util as su
from contrack_amd import _native
from contrack_amd.contrack import blockstat_numpy

pytestmark = pytest.mark.gpu

IMIN, IMAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
NAN, INF = float("nan"), float("inf")
WANTS = {bu.SHAPE: ("shape",), bu.PEAKS: ("peaks",), bu.SHAPE | bu.PEAKS: ("shape", "peaks")}
LDS, GLB = (_native.BLOCKSTAT_FORMS.index(n) for n in ("row_lds", "row_glb"))
BOUNDARY_ID, UNWANTED_ID = 11, 99


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def hand_slab(ny, nx, dtype):
    """(flag, x, table, boundary pixel) of three steps:
    step 0  the column cases, each id on a row of its own: 31 | 32 and 63 | 64 alone and together, over the seam, a full circle, one
            column (the last: a partial bit-set word), the two tie cases
    step 1  a block over the part boundary with its maximum once in each part and its minimum too; the value cases
    step 2  an id that is present and not wanted, an empty slice
    The background holds 0, -1 and INT32_MIN; id 11 is wanted at step 0 too, where it is absent; one id is 2^31 - 1."""
    vec = ny * nx % 4 == 0
    part = _native.blockstat_plan("shape", 1, ny, nx)["part_lanes"] * (4 if vec else 1)       # pixels of a part
    assert part < ny * nx <= 2 * part, "two parts per step"
    f = np.zeros((3, ny, nx), dtype=np.int32)
    f[:, ::2, ::3] = -1
    f[:, 1::2, 1::3] = IMIN
    rng = np.random.default_rng(ny * nx)
    x = rng.permutation(f.size).reshape(f.shape).astype(dtype) / 64 - 17                       # distinct, exact in float32
    col_cases = {21: [31], 22: [32], 23: [31, 32], 28: [nx - 2, nx - 1, 0, 1], 29: list(range(nx)), 30: [nx - 1], 31: [0, nx // 2], 32: [nx // 4, nx // 4 + nx // 2]}
    if nx > 64:
        col_cases.update({24: [63], 25: [64], 26: [63, 64], 27: [31, 32, 63, 64]})
    for k, (i, cols) in enumerate(sorted(col_cases.items())):
        f[0, 2 * k, cols] = i
        f[0, 2 * k + 1, cols[:1]] = i                                                         # (two rows: r0 != r1)
    # step 1: the boundary block
    rb, cb = part // nx, part % nx
    cols = list(range(max(cb - 10, 0), min(cb + 11, nx)))
    assert rb >= 1 and rb < ny and cols[-1] - 1 >= cb and cols[0] + 1 < cb
    f[1, rb - 1:rb + 1, cols] = BOUNDARY_ID
    x[1, rb - 1:rb + 1, cols[0]:cols[-1] + 1] = rng.permutation(2 * len(cols)).reshape(2, -1).astype(dtype) / 8 - 3      # in (-3, 3)
    x[1, rb - 1, cols[0]] = x[1, rb, cols[-1]] = 9.0
    x[1, rb - 1, cols[0] + 1] = x[1, rb, cols[-1] - 1] = -9.0
    # ... and the value cases on the first rows, three pixels each
    tiny = np.float32(1e-45)
    values = {41: [-0.0, 0.0, -0.0], 42: [0.0, -0.0, 0.0], 43: [INF, 1.0, -INF], 44: [NAN, 2.5, NAN], 45: [NAN, NAN, NAN], 46: [tiny, 0.0, -tiny],
              47: [1.0, 1.0 + 2.0 ** -40, 1.0], 48: [-INF, -INF, NAN], IMAX: [5.0, 7.0, 6.0]}
    for k, (i, v) in enumerate(values.items()):
        assert k < rb - 1
        f[1, k, 4:7] = i
        x[1, k, 4:7] = v
    # step 2
    f[2, 3, 5:9] = UNWANTED_ID
    f[2, 4, 5:9] = 21
    table = su.table_by_row([sorted(set(col_cases) | {BOUNDARY_ID}), sorted(set(values) | {BOUNDARY_ID, 5}), []])
    assert (f == 0).any() and (f == -1).any() and (f == IMIN).any()
    return f, x, table, part


@functools.lru_cache(maxsize=None)
def wanted(ny, nx, dtype, want):
    f, x, table, _ = hand_slab(ny, nx, dtype)
    return bu.blockstat(f, x if want & bu.PEAKS else None, *table, want=want)


def same(got, want, case):
    assert got.dtype == bu.ROW, case
    assert bu.same_rows(got, want), (case, bu.diff_rows(got, want))


def on_device(trk, f, x, table, want, off=0, xoff=0):
    """ctk_blockstat_*_dev on copies of f and x that start `off` / `xoff` bytes past a 16-byte boundary"""
    d_f = trk.malloc(f.nbytes + 16)
    d_x = trk.malloc(x.nbytes + 16) if x is not None else None
    try:
        pf = C.c_void_p(d_f.value + off)
        trk.h2d(pf, f)
        px = None
        if x is not None:
            px = C.c_void_p(d_x.value + xoff)
            trk.h2d(px, x)
        return trk.blockstat_dev(pf, px, f.shape[0], f.shape[1], f.shape[2], table, want, f64=x is not None and x.dtype == np.float64)
    finally:
        trk.free(d_f)
        if d_x is not None:
            trk.free(d_x)


# ---- the hand-made slabs really hold what they are meant to ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 104), (33, 35)], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_preconditions_of_the_hand_made_slab(shape, dtype):
    ny, nx = shape
    f, x, table, part = hand_slab(ny, nx, dtype)
    off, ids = table
    rows = wanted(ny, nx, dtype, bu.SHAPE | bu.PEAKS)
    row = lambda t, i: rows[off[t] + list(ids[off[t]:off[t + 1]]).index(i)]
    # the block crosses the part boundary, its extremes sit once in each part and the lower index wins
    P = np.flatnonzero(f[1].reshape(-1) == BOUNDARY_ID)
    v = x[1].reshape(-1)[P]
    assert P.min() < part <= P.max()
    r = row(1, BOUNDARY_ID)
    for name, val in (("max", 9.0), ("min", -9.0)):
        at = P[v == val]
        assert len(at) == 2 and at[0] < part <= at[1] and r[name] == val and r[name + "_p"] == at[0]
    assert (v <= 9.0).all() and (v >= -9.0).all()
    # the column cases: words 0 | 1 and 1 | 2 of the bit set, the seam, the circle, the partial last word, the ties
    assert nx % 32 != 0 and (row(0, 30)["west"], row(0, 30)["width"]) == (nx - 1, 1)
    assert [(int(row(0, i)["west"]), int(row(0, i)["width"])) for i in (21, 22, 23)] == [(31, 1), (32, 1), (31, 2)]
    if nx > 64:
        assert [(int(row(0, i)["west"]), int(row(0, i)["width"])) for i in (24, 25, 26, 27)] == [(63, 1), (64, 1), (63, 2), (31, 34)]
    assert (row(0, 28)["west"], row(0, 28)["width"]) == (nx - 2, 4) and (row(0, 29)["west"], row(0, 29)["width"]) == (0, nx)
    a, b = nx // 2, nx // 4
    assert (nx - a - 1 == a - 1 or nx % 2) and row(0, 31)["west"] == (a if nx - a - 1 <= a - 1 else 0)
    assert row(0, 32)["west"] in (b, b + nx // 2) and row(0, 32)["width"] > nx // 2
    if nx == 104:                                                                  # both are ties of two 51-column gaps: the lower start won
        assert (row(0, 31)["west"], row(0, 31)["width"], row(0, 32)["west"], row(0, 32)["width"]) == (52, 53, 78, 53)
    assert (rows["r1"][:off[1]][rows["n"][:off[1]] > 0] > rows["r0"][:off[1]][rows["n"][:off[1]] > 0]).all()
    # the value cases
    assert np.signbit(row(1, 41)["min"]) and not np.signbit(row(1, 41)["max"]) and (row(1, 41)["max_p"], row(1, 41)["min_p"]) == (0 * nx + 5, 0 * nx + 4)
    assert np.signbit(row(1, 42)["min"]) and not np.signbit(row(1, 42)["max"]) and (row(1, 42)["max_p"], row(1, 42)["min_p"]) == (1 * nx + 4, 1 * nx + 5)
    assert (row(1, 43)["max"], row(1, 43)["min"]) == (INF, -INF)
    assert (row(1, 44)["n"], row(1, 44)["nv"], row(1, 44)["max"], row(1, 44)["max_p"]) == (3, 1, 2.5, 3 * nx + 5)
    assert (row(1, 45)["n"], row(1, 45)["nv"], row(1, 45)["max_p"], row(1, 45)["min_p"]) == (3, 0, -1, -1) and np.isnan(row(1, 45)["max"])
    assert row(1, 46)["max"] == float(np.float32(1e-45)) > 0 > row(1, 46)["min"] == -float(np.float32(1e-45))
    assert row(1, 47)["max_p"] == 6 * nx + (5 if dtype == np.float64 else 4) and row(1, 47)["min_p"] == 6 * nx + 4
    assert (row(1, 48)["max"], row(1, 48)["min"], row(1, 48)["max_p"], row(1, 48)["min_p"], row(1, 48)["nv"]) == (-INF, -INF, 7 * nx + 4, 7 * nx + 4, 2)
    assert row(1, IMAX)["n"] == 3 and row(1, IMAX)["max"] == 7.0
    # absent where wanted, present where not wanted, an empty slice
    assert row(0, BOUNDARY_ID)["n"] == 0 and row(1, 5)["n"] == 0 and (f[2] == UNWANTED_ID).any() and off[3] == off[2]
    assert bu.same_rows(rows[[list(ids[:off[1]]).index(BOUNDARY_ID)]], bu.empty_rows(1))


# ---- every path equals the statement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 104), (33, 35)], ids=["vector", "scalar"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_every_path_equals_the_statement(trk, shape, dtype):
    ny, nx = shape
    f, x, table, part = hand_slab(ny, nx, dtype)
    T = f.shape[0]
    vec = ny * nx % 4 == 0
    for bits, want in WANTS.items():
        rows = wanted(ny, nx, dtype, bits)
        case = (shape, dtype.__name__, want)
        for off in (0, 4, 8):
            for xoff in ((0, 4, 8) if dtype == np.float32 else (0, 8)):
                same(on_device(trk, f, x if bits & bu.PEAKS else None, table, want, off, xoff), rows, case + ("dev", off, xoff))
                form, v, grid = trk.debug_blockstat_launch()
                assert form == LDS and v == (vec and off == 0), (case, off)
                if off == 0:
                    assert grid == 2 * T, "two parts per step"
        for chunk in (1, 2, T, 0):
            same(trk.blockstat(f, table, x, want, chunk_steps=chunk), rows, case + ("host", chunk))
            same(trk.blockstat_cb(f, x if bits & bu.PEAKS else None, f.shape, dtype, table, want, chunk_steps=chunk), rows, case + ("cb", chunk))
            same(blockstat_numpy(f, table, x, want, chunk_steps=chunk), rows, case + ("numpy", chunk))
        fread = lambda t0, nt, out: out.__setitem__(Ellipsis, f[t0:t0 + nt])
        xread = (lambda t0, nt, out: out.__setitem__(Ellipsis, x[t0:t0 + nt])) if bits & bu.PEAKS else None
        same(trk.blockstat_cb(fread, xread, f.shape, dtype, table, want, chunk_steps=2), rows, case + ("readers",))
        same(blockstat_numpy(fread, table, xread, want, chunk_steps=2, shape=f.shape, dtype=dtype), rows, case + ("numpy readers",))
        same(blockstat_numpy(f.astype(np.int64), table, x, want), rows, case + ("numpy int64",))
    # a field given without peaks is not read; the empty table succeeds and writes nothing
    same(trk.blockstat(f, table, x, "shape"), wanted(ny, nx, dtype, bu.SHAPE), "field not wanted")
    empty = su.table_by_row([[], [], []])
    for got in (trk.blockstat(f, empty, x), trk.blockstat_cb(f, x, f.shape, dtype, empty), on_device(trk, f, x, empty, ("shape", "peaks"))):
        assert got.dtype == bu.ROW and len(got) == 0


def test_readers_are_called_flag_first_once_per_chunk(trk):
    f, x, table, _ = hand_slab(33, 35, np.float32)
    calls = []
    fread = lambda t0, nt, out: (calls.append(("flag", t0, nt)), out.__setitem__(Ellipsis, f[t0:t0 + nt]))
    xread = lambda t0, nt, out: (calls.append(("field", t0, nt)), out.__setitem__(Ellipsis, x[t0:t0 + nt]))
    same(trk.blockstat_cb(fread, xread, f.shape, np.float32, table, chunk_steps=2), wanted(33, 35, np.float32, 3), "readers")
    assert calls == [("flag", 0, 2), ("field", 0, 2), ("flag", 2, 1), ("field", 2, 1)]
    del calls[:]
    same(trk.blockstat_cb(fread, xread, f.shape, np.float32, table, "shape", chunk_steps=2), wanted(33, 35, np.float32, 1), "shape only")
    assert calls == [("flag", 0, 2), ("flag", 2, 1)]                               # only the flags travel

    def bad(t0, nt, out):
        raise KeyError("reader")
    with pytest.raises(KeyError):
        trk.blockstat_cb(fread, bad, f.shape, np.float32, table)
    same(trk.blockstat(f, table, x), wanted(33, 35, np.float32, 3), "after a failing reader")


# ---- the global form, reached by size alone ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded(dtype):
    """(2, 2, 1440): at step 0 every 16 pixels an id of their own, 12 of them set -- 180 ids; at step 1 two ids"""
    f = np.zeros((2, 2, 1440), dtype=np.int32)
    p = np.arange(2880)
    f[0].reshape(-1)[:] = np.where(p % 16 < 12, p // 16 + 1, 0)
    f[1, 0, 1430:] = 5
    f[1, 1, :10] = 5
    f[1, 1, 700] = 6
    rng = np.random.default_rng(3)
    x = rng.permutation(f.size).reshape(f.shape).astype(dtype) - 2000
    x[rng.random(f.shape) < 0.2] = NAN
    return f, x


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_global_form_and_the_step_one_id_below_it(trk, dtype):
    f, x = crowded(dtype)
    for bits, want in WANTS.items():
        cap = _native.blockstat_plan(want, 1, 2, 1440)["lds_entries"]
        assert (cap == 151) == bool(bits & bu.SHAPE) and (cap < 180 or not bits & bu.SHAPE)
        for n, form in ((min(cap, 180), LDS), (cap + 1, GLB)):
            if n > 180:
                continue                                                            # (without the shape a 1440-column step has no room for that many ids)
            table = su.table_by_row([list(range(1, n + 1)), [5, 6]])
            rows = bu.blockstat(f, x if bits & bu.PEAKS else None, *table, want=bits)
            assert (rows["n"] > 0).all() and (not bits & bu.SHAPE or (rows["west"][-2], rows["width"][-2]) == (1430, 20))
            case = (dtype.__name__, want, n)
            for off in (0, 4):
                same(on_device(trk, f, x if bits & bu.PEAKS else None, table, want, off), rows, case + ("dev", off))
                assert trk.debug_blockstat_launch()[:2] == (form, off == 0), case
            for chunk in (1, 0):
                same(trk.blockstat(f, table, x, want, chunk_steps=chunk), rows, case + ("host", chunk))
                assert trk.debug_blockstat_launch()[0] == form, case
    # the budget's edge is reached in both directions with the shape wanted
    assert _native.blockstat_plan("shape", 151, 2, 1440)["form"] == LDS and _native.blockstat_plan("shape", 152, 2, 1440)["form"] == GLB


# ---- the resident field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_resident_field_and_the_resident_slot(trk, dtype):
    lat = ru.grid(7.5)
    z = ru.field(lat, 8, steps=4, seed=1, dtype=dtype)
    res = trk.reversal(z, ru.table(lat), keep_resident=True)                        # (leaves its output resident, as calc_anom does)
    gen, slot = trk.resident_generation(), trk.resident_anom()
    assert slot == z.shape + (dtype == np.float64,)
    rng = np.random.default_rng(4)
    f = rng.integers(0, 4, size=z.shape).astype(np.int32)
    table = su.table_by_row([[1, 2, 3], [2], [], [1, 3]])
    rows = bu.blockstat(f, res, *table)
    assert (rows["nv"] > 0).all()
    f64 = dtype == np.float64
    same(trk.blockstat(f, table, res), rows, "explicit")
    for chunk in (0, 1, 3):
        same(trk.blockstat(f, table, None, chunk_steps=chunk, resident_f64=f64), rows, ("resident host", chunk))
        same(trk.blockstat_cb(f, None, f.shape, dtype, table, chunk_steps=chunk), rows, ("resident cb", chunk))
    d_f = trk.malloc(f.nbytes)
    try:
        trk.h2d(d_f, f)
        same(trk.blockstat_dev(d_f, None, *f.shape, table, f64=f64), rows, "resident dev")
        with pytest.raises(ValueError, match="resident"):
            trk.blockstat_dev(d_f, None, *f.shape, table, f64=not f64)              # the other type is not resident
    finally:
        trk.free(d_f)
    with pytest.raises(ValueError, match="resident"):
        trk.blockstat(f[:3], su.table_by_row([[1], [], []]), None, resident_f64=f64)        # another shape
    with pytest.raises(ValueError):
        trk.blockstat(f, (table[0], -table[1]), res)
    same(trk.blockstat(f, table, None, "shape"), bu.blockstat(f, None, *table, want=bu.SHAPE), "no field wanted")
    assert trk.resident_generation() == gen and trk.resident_anom() == slot


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_every_error_case_leaves_the_handle_working():
    L = _native.lib()
    T, ny, nx = 3, 4, 8
    rng = np.random.default_rng(5)
    f = rng.integers(0, 8, size=(T, ny, nx)).astype(np.int32)
    x = rng.normal(size=f.shape).astype(np.float32)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    good_off, good_ids = i64(0, 1, 1, 3), i32(4, 2, 6)
    want_rows = bu.blockstat(f, x, good_off, good_ids)
    rows = np.empty(4, dtype=bu.ROW)
    rows.view(np.uint8)[:] = 0x5a
    gc.collect()
    live = _native.debug_live()
    trk = _native.Tracker(0)                                                        # (a handle of its own: nothing is resident on it)
    try:
        def host(off=good_off, ids=good_ids, n_off=None, n_ids=None, T=T, ny=ny, nx=nx, flag=f, field=x, want=3, chunk=0, r=rows):
            return L.ctk_blockstat_f32(trk.handle, None if flag is None else flag.ctypes.data, None if field is None else field.ctypes.data, T, ny, nx,
                                       None if off is None else off.ctypes.data, len(off) if n_off is None else n_off, None if ids is None else ids.ctypes.data,
                                       len(ids) if n_ids is None else n_ids, want, None if r is None else r.ctypes.data, chunk)

        cases = {
            "null flag": dict(flag=None),
            "null rows": dict(r=None),
            "null off": dict(off=None, n_off=T + 1),
            "null ids": dict(ids=None, n_ids=3),
            "T < 1": dict(T=0, n_off=1),
            "ny < 1": dict(ny=0),
            "nx < 1": dict(nx=-1),
            "plane of 2^31": dict(ny=65536, nx=32768),
            "n_off": dict(off=i64(0, 1, 3)),
            "by id": dict(off=i64(0, 3), ids=i32(2, 4, 6)),
            "off[0]": dict(off=i64(1, 1, 1, 3)),
            "off decreasing": dict(off=i64(0, 2, 1, 3)),
            "off beyond": dict(off=i64(0, 4, 4, 3)),
            "off[T]": dict(off=i64(0, 1, 1, 2)),
            "id 0": dict(ids=i32(4, 0, 6)),
            "id negative": dict(ids=i32(-4, 2, 6)),
            "equal ids": dict(ids=i32(4, 2, 2)),
            "falling ids": dict(ids=i32(4, 6, 2)),
            "want 0": dict(want=0),
            "want 4": dict(want=4),
            "want 1 | 8": dict(want=9),
            "want negative": dict(want=-1),
            "peaks without a field": dict(field=None),
            "peaks only without a field": dict(field=None, want=2),
            "chunk_steps": dict(chunk=-1),
        }
        for name, kw in cases.items():
            assert host(**kw) == _native.CTK_E_INVALID, name
            msg = L.ctk_last_error().decode()
            assert "ctk_blockstat_f32" in msg, (name, msg)
            assert (rows.view(np.uint8) == 0x5a).all(), name
            same(trk.blockstat(f, (good_off, good_ids), x), want_rows, ("after", name))
        assert host(field=None, want=1) == 0 and bu.same_rows(rows[:3], bu.blockstat(f, None, good_off, good_ids, want=bu.SHAPE))
        assert (rows[3:].view(np.uint8) == 0x5a).all()                              # n_ids rows are written, no more
        rows.view(np.uint8)[:] = 0x5a
        # the same checks guard the device and the callback entries
        d = trk.malloc(f.nbytes)
        try:
            trk.h2d(d, f)
            dev = lambda off, ids, flag=d, want=1, fn=L.ctk_blockstat_f32_dev: fn(trk.handle, flag, None, T, ny, nx, off.ctypes.data, len(off), ids.ctypes.data,
                                                                                  len(ids), want, rows.ctypes.data)
            assert dev(good_off, good_ids, flag=None) == _native.CTK_E_INVALID
            assert dev(i64(0, 3), i32(2, 4, 6)) == _native.CTK_E_INVALID
            assert dev(good_off, i32(4, 2, 2)) == _native.CTK_E_INVALID
            assert dev(good_off, good_ids, want=0) == _native.CTK_E_INVALID
            assert dev(good_off, good_ids, want=3) == _native.CTK_E_INVALID          # peaks, no field, nothing resident
            assert dev(good_off, good_ids, want=2, fn=L.ctk_blockstat_f64_dev) == _native.CTK_E_INVALID
            assert (rows.view(np.uint8) == 0x5a).all()
            assert dev(good_off, good_ids) == 0 and bu.same_rows(rows[:3], bu.blockstat(f, None, good_off, good_ids, want=bu.SHAPE))
        finally:
            trk.free(d)
        rows.view(np.uint8)[:] = 0x5a
        null_reader = C.cast(None, _native.READ_CHUNK_FN)
        cb = lambda elem=4, chunk=0: L.ctk_blockstat_cb(trk.handle, elem, T, ny, nx, null_reader, None, null_reader, None, good_off.ctypes.data, 4, good_ids.ctypes.data, 3,
                                                        1, rows.ctypes.data, chunk)
        assert cb() == _native.CTK_E_INVALID and cb(elem=2) == _native.CTK_E_INVALID
        with pytest.raises(ValueError):
            trk.blockstat_cb(f, x, f.shape, np.float32, (good_off, good_ids), chunk_steps=-1)
        with pytest.raises(ValueError):
            trk.blockstat(f, (good_off, good_ids), x, want="extent")
        with pytest.raises(ValueError):
            blockstat_numpy(f, (good_off, good_ids), x, chunk_steps=-2)
        with pytest.raises(ValueError):
            trk.blockstat(f, (good_off, good_ids), x[:2])
        assert (rows.view(np.uint8) == 0x5a).all()
        same(trk.blockstat_cb(f, x, f.shape, np.float32, (good_off, good_ids)), want_rows, "at the end")
        assert _native.debug_live()[0] > live[0]
    finally:
        trk.close()
    assert _native.debug_live() == live                                             # the new buffers went with the handle
