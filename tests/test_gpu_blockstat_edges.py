"""k_blockstat and k_blockstat_finish at their edges: one workgroup over many (step, part) pairs under both XCD mappings (slices of
different lengths, an empty one in mid-stride, in LDS and in global memory), quads that cross a row, positions at and above 2^16,
slices of several hundred ids at the LDS capacity of each grid and one above it, the smallest planes, the column ring at the word
boundaries of the bit set and over every occupancy of a small circle, and the values at the ends of the key order.  Against
tests/blockstat_util.py, equality everywhere, the two floats by their bits.  The slabs are built by hand, every case asserts its own
precondition on the statement's rows or the plan hook, and every capacity comes from the plan hook."""
import contextlib
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import blockstat_util as bu
import subset_util as su
from contrack_amd import _native

pytestmark = pytest.mark.gpu

IMIN, IMAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
NAN, INF = float("nan"), float("inf")
WANTS = {bu.SHAPE: "shape", bu.PEAKS: "peaks", bu.SHAPE | bu.PEAKS: ("shape", "peaks")}
LDS, GLB = (_native.BLOCKSTAT_FORMS.index(n) for n in ("row_lds", "row_glb"))
DTYPES = pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
FORMS = pytest.mark.parametrize("form", [LDS, GLB], ids=["lds", "glb"])


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def plan(want, longest, shape, **kw):
    return _native.blockstat_plan(want, longest, shape[1], shape[2], **kw)


def same(got, want, case):
    assert got.dtype == bu.ROW, case
    assert bu.same_rows(got, want), (case, bu.diff_rows(got, want))


def row_of(rows, table, t, i):
    off, ids = table
    return rows[off[t] + list(ids[off[t]:off[t + 1]]).index(i)]


def background(f):
    f[:, ::2, ::3] = -1
    f[:, 1::2, 1::3] = IMIN


@contextlib.contextmanager
def on_device(trk, f, x):
    """run(table, want, off): ctk_blockstat_*_dev on device copies of f that start 0 and 4 bytes past a 16-byte boundary and one of x"""
    bufs = [trk.malloc(f.nbytes + 16), trk.malloc(f.nbytes + 16), trk.malloc(x.nbytes)]
    try:
        pf = {0: bufs[0], 4: C.c_void_p(bufs[1].value + 4)}
        for p in pf.values():
            trk.h2d(p, f)
        trk.h2d(bufs[2], x)

        def run(table, want, off):
            peaks = _native._block_want(want) & bu.PEAKS
            return trk.blockstat_dev(pf[off], bufs[2] if peaks else None, f.shape[0], f.shape[1], f.shape[2], table, want, f64=x.dtype == np.float64)
        yield run
    finally:
        for b in bufs:
            trk.free(b)


def reference(f, x, table, bits):
    return bu.blockstat(f, x if bits & bu.PEAKS else None, *table, want=bits)


def padded(slices, longest, at=-1):
    """the table of `slices` with absent ids above every id of the slab appended to slice `at`, which then has `longest` ids"""
    slices = [list(s) for s in slices]
    assert len(slices[at]) <= longest and max(slices[at], default=0) < (1 << 30)
    slices[at] += list(range(1 << 30, (1 << 30) + longest - len(slices[at])))
    return su.table_by_row(slices)


def check(trk, run, f, x, table, bits, rows, form, case, chunks=(1, 0)):
    """the device entry at both pointer offsets and the host entry: the rows, and the launch against the plan hook"""
    want = WANTS[bits]
    longest = int(np.diff(table[0]).max())
    for off in (0, 4):
        same(run(table, want, off), rows, case + ("dev", off))
        pl = plan(want, longest, f.shape, steps=f.shape[0], elem_bytes=x.dtype.itemsize, aligned=off == 0)
        assert pl["form"] == form and pl["vec"] == (off == 0 and f[0].size % 4 == 0), case
        assert trk.debug_blockstat_launch() == (pl["form"], pl["vec"], pl["grid"]), (case, off)
    for chunk in chunks:
        same(trk.blockstat(f, table, x, want, chunk_steps=chunk), rows, case + ("host", chunk))
        assert trk.debug_blockstat_launch()[0] == form, (case, chunk)


# ---- a. the stride loop -------------------------------------------------------------------------------------------------------------------
SHAPE_A = (5, 182, 362)
BIG, QUAD, FAR, LASTQ, ALL, SEAM, ENDS = 7, 9, 12, 15, 4, 5, 3
QUAD_ROW = 4
LIVE3 = (0, 1, 255, 256, 257, 299, 390, 511, 512, 910)          # positions of the step-3 slice whose ids are in the slab
ID3 = lambda k: 1000 + 2 * k


@functools.lru_cache(maxsize=None)
def stride_slab(dtype):
    """step 0  a block over 16 vector parts and the last row, its extremes three times each (first part, last part of the rows, at
               p >= 2^16); a quad over two rows; an id above 2^16 only; the plane's last quad; an unwanted id
    step 1  one id on every pixel, a tenth of its values NaN
    step 2  wanted nowhere (ids present)
    step 3  six pixels across each of ten part boundaries, their ids at positions 0 .. 910 of the slice; values between, below and
            above the wanted ids
    step 4  an id on the first and last pixels of the plane, a block over the seam, an unwanted id"""
    T, ny, nx = SHAPE_A
    f = np.zeros(SHAPE_A, dtype=np.int32)
    background(f)
    rng = np.random.default_rng(11)
    x = rng.permutation(f.size).reshape(f.shape).astype(dtype) / 64 - 17                      # distinct, exact in float32, below 1e6
    f[0, 10:171, 100:141] = f[0, 181, 100:141] = BIG
    x[0, 10, 100] = x[0, 170, 140] = x[0, 181, 139] = 1e6
    x[0, 10, 101] = x[0, 170, 139] = x[0, 181, 140] = -1e6
    f[0, QUAD_ROW, 360:362] = f[0, QUAD_ROW + 1, 0:2] = QUAD
    f[0, 181, 200:261] = FAR
    f[0, 181, 358:362] = LASTQ
    f[0, 3, 5:9] = 13
    f[1] = ALL
    x[1][rng.random((ny, nx)) < 0.1] = NAN
    f[2, 20:30, 50:60] = BIG
    f[2, 181, 358:362] = LASTQ
    g, v = f[3].reshape(-1), x[3].reshape(-1)
    for k, pos in enumerate(LIVE3):
        g[4096 * (k + 1) - 3:4096 * (k + 1) + 3] = ID3(pos)
        v[4096 * (k + 1) - (k % 3)] = NAN
    for k, i in enumerate((999, ID3(0) + 1, ID3(256) + 1, ID3(910) + 1, 5000000, IMAX)):
        g[1024 * (4 * k + 2) - 1:1024 * (4 * k + 2) + 2] = i
    f[4, 0, 0:2] = f[4, 181, 360:362] = ENDS
    f[4, 50:61, 355:362] = f[4, 50:61, 0:7] = SEAM
    f[4, 100, 100:104] = 6
    assert (f == 0).any() and (f == -1).any() and (f == IMIN).any()
    return f, x


def stride_table(longest):
    return su.table_by_row([[BIG, QUAD, FAR, LASTQ, 16, 5000000], [ALL], [], [ID3(k) for k in range(longest)], [ENDS, SEAM, 8]])


@functools.lru_cache(maxsize=None)
def stride_rows(dtype, bits, longest):
    f, x = stride_slab(dtype)
    return reference(f, x, stride_table(longest), bits)


@DTYPES
def test_preconditions_of_the_stride_slab(dtype):
    T, ny, nx = SHAPE_A
    npix = ny * nx
    f, x = stride_slab(dtype)
    assert npix == 65884 and npix % 4 == 0 and nx % 4 == 2
    for off, bps in ((0, 17), (4, 65)):
        pl = plan("shape", 1, SHAPE_A, steps=T, aligned=off == 0)
        assert (pl["vec"], pl["bps"], pl["blocks"]) == (off == 0, bps, T * bps)
    part = plan("shape", 1, SHAPE_A)["part_lanes"] * 4                                          # pixels of a vector part
    table = stride_table(300)
    assert len(set(np.diff(table[0]).tolist())) == T and np.diff(table[0])[2] == 0              # five slice lengths, an empty one inside
    rows = stride_rows(dtype, bu.SHAPE | bu.PEAKS, 300)
    row = lambda t, i: row_of(rows, table, t, i)
    # the block: sixteen parts and the last, its extremes in three of them and the lowest position reported
    P = np.flatnonzero(f[0].reshape(-1) == BIG)
    v = x[0].reshape(-1)[P]
    assert len(set((P // part).tolist())) >= 3 and (row(0, BIG)["r0"], row(0, BIG)["r1"]) == (10, 181)
    for name, val in (("max", 1e6), ("min", -1e6)):
        at = P[v == val]
        assert (at // part).tolist() == [0, 15, 16] and at[2] >= 65536 and row(0, BIG)[name] == val and row(0, BIG)[name + "_p"] == at[0]
    assert (np.abs(v) <= 1e6).all()
    assert row(0, FAR)["max_p"] >= 65536 and row(0, FAR)["min_p"] >= 65536 and row(0, FAR)["max_p"] != row(0, FAR)["min_p"]
    # the quad over two rows, the last quad of the plane (alone in the last partial part), one id on every pixel
    q = row(0, QUAD)
    assert QUAD_ROW % 2 == 0 and (QUAD_ROW * nx + 360) % 4 == 0 and (q["n"], q["r0"] + 1, q["west"], q["width"]) == (4, q["r1"], 360, 4)
    assert np.flatnonzero(f[0].reshape(-1) == LASTQ).tolist() == list(range(npix - 4, npix)) and (npix - 4) // part == 16
    assert (row(0, LASTQ)["n"], row(0, LASTQ)["r0"], row(0, LASTQ)["west"]) == (4, ny - 1, nx - 4)
    a = row(1, ALL)
    assert (a["n"], a["width"], a["west"], a["r0"], a["r1"]) == (npix, nx, 0, 0, ny - 1) and 0 < a["nv"] < npix
    # the long slice: live entries beyond 256, most ids absent, every live one across a part boundary of both forms
    n3 = rows["n"][table[0][3]:table[0][4]]
    assert np.flatnonzero(n3).tolist() == [k for k in LIVE3 if k < 300] and (n3[n3 > 0] == 6).all()
    assert n3[299] == 6 and row(3, ID3(257))["nv"] == 5
    assert (row(4, SEAM)["west"], row(4, SEAM)["width"]) == (355, 14) and (row(4, ENDS)["n"], row(4, ENDS)["r0"], row(4, ENDS)["r1"]) == (4, 0, 181)
    assert row(0, 16)["n"] == 0 and row(0, 5000000)["n"] == 0 and row(4, 8)["n"] == 0 and (f[2] == BIG).any() and (f[4] == 6).any()


@FORMS
@DTYPES
def test_one_workgroup_over_many_parts_and_both_xcd_mappings(trk, dtype, form):
    """the whole product: xcd modes 0, 1, 2 x caps 0 (a workgroup per part), 1, 3, 9, 16 x the three wants, on the device at pointer
    offsets 0 (vector: 85 parts) and 4 (scalar: 325) and once through the host entry in chunks of two steps.  LDS: a longest slice
    of 300; global: one above the capacity of the want.  Under cap 1 a single workgroup takes every part in turn."""
    T = SHAPE_A[0]
    f, x = stride_slab(dtype)
    esz = x.dtype.itemsize
    with on_device(trk, f, x) as run:
        try:
            for bits, want in WANTS.items():
                cap_lds = plan(want, 1, SHAPE_A)["lds_entries"]
                assert cap_lds == (910 if bits == bu.PEAKS else 390)
                longest = 300 if form == LDS else cap_lds + 1
                table, rows = stride_table(longest), stride_rows(np.float32 if bits == bu.SHAPE else dtype, bits, longest)
                assert rows["n"][table[0][4] - 1] == 6                                      # the slice's last entry is live
                for mode, cap in itertools.product((0, 1, 2), (0, 1, 3, 9, 16)):
                    trk.debug_set_blockstat(mode, cap)
                    case = (dtype.__name__, want, longest, mode, cap)
                    for off in (0, 4):
                        pl = plan(want, longest, SHAPE_A, steps=T, elem_bytes=esz, aligned=off == 0, grid_max=cap)
                        assert pl["blocks"] == (85 if off == 0 else 325) and pl["grid"] == (cap or pl["blocks"]) and pl["form"] == form
                        same(run(table, want, off), rows, case + ("dev", off))
                        assert trk.debug_blockstat_launch() == (form, off == 0, pl["grid"]), (case, off)
                    same(trk.blockstat(f, table, x, want, chunk_steps=2), rows, case + ("host",))
                    got = trk.debug_blockstat_launch()                                      # (the last chunk: step 4 alone)
                    assert got == (form, got[1], plan(want, longest, SHAPE_A, steps=1, elem_bytes=esz, aligned=got[1], grid_max=cap)["grid"]), case
        finally:
            trk.debug_set_blockstat()


# ---- b. the LDS capacity of each grid ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pairs_slab(ny, nx, dtype):
    """step 0: pair j of pixels holds 3 j + 1 -- every seventh 3 j + 2, a value between two wanted ids, every eleventh the background
    -- and the last pair 2^31 - 1; step 1: values below, between and above its two wanted ids"""
    f = np.zeros((2, ny, nx), dtype=np.int32)
    j = np.arange(ny * nx // 2)
    v = np.where(j % 7 == 3, 3 * j + 2, np.where(j % 11 == 5, np.where(j % 2, -1, IMIN), 3 * j + 1))
    v[-1] = IMAX
    f[0].reshape(-1)[:] = np.repeat(v, 2)
    f[1].reshape(-1)[:24] = np.repeat([1, 45, 40, 40, 40, 50], 4)
    f[1].reshape(-1)[-8:] = np.repeat([50, 60, IMAX, -1], 2)
    rng = np.random.default_rng(ny * nx)
    x = rng.permutation(f.size).reshape(f.shape).astype(dtype) - 1000
    x[rng.random(f.shape) < 0.2] = NAN
    return f, x


@pytest.mark.parametrize("shape", [(240, 8), (6, 362), (4, 480)], ids=["nx8", "nx362", "nx480"])
@DTYPES
def test_slices_at_the_lds_capacity_and_one_above(trk, shape, dtype):
    ny, nx = shape
    f, x = pairs_slab(ny, nx, dtype)
    literal = {8: (819, 910, 819), 362: (390, 910, 390), 480: (341, 910, 341)}[nx]
    with on_device(trk, f, x) as run:
        for (bits, want), lit in zip(WANTS.items(), literal):
            cap = plan(want, 1, f.shape)["lds_entries"]
            assert cap == lit > 256 and cap < f[0].size // 2
            for longest, form in ((cap, LDS), (cap + 1, GLB)):
                table = su.table_by_row([[3 * k + 1 for k in range(longest - 1)] + [IMAX], [40, 50]])
                rows = reference(f, x, table, bits)
                n0 = rows["n"][:longest]
                assert n0[0] == 2 and n0[-1] == 2 and n0[256:].sum() > 100 and (longest < 600 or n0[512:].sum() > 100) and (n0 == 0).sum() > 30
                assert table[1][0] == 1 and (rows["n"][longest:] == (12, 6)).all()
                check(trk, run, f, x, table, bits, rows, form, (shape, dtype.__name__, want, longest))


# ---- c. the smallest planes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@DTYPES
def test_smallest_planes(trk, T, dtype):
    for ny, nx in ((1, 1), (1, 3), (4, 1), (2, 2), (4, 3), (2, 6), (3, 5), (1, 4)):
        rng = np.random.default_rng(16 * ny + nx)
        f = rng.choice(np.array([0, -1, 1, 2, 3, 3], dtype=np.int32), size=(T, ny, nx))
        x = rng.permutation(f.size).reshape(f.shape).astype(dtype)
        x[rng.random(f.shape) < 0.2] = NAN
        f.reshape(-1)[0] = 2
        slices = [[1, 2, 3], [2], [1, 3]][:T]
        if (ny, nx) in ((4, 1), (2, 2), (4, 3)):                                    # one quad over 4, 2 and 2 rows
            q = 4 if (ny, nx) == (4, 3) else 0
            f[0].reshape(-1)[q:q + 4] = 9
            slices[0] = [1, 2, 3, 9]
        table = su.table_by_row(slices)
        vec = ny * nx % 4 == 0
        with on_device(trk, f, x) as run:
            for bits, want in WANTS.items():
                rows = reference(f, x, table, bits)
                assert rows["n"].any()
                if 9 in slices[0] and bits & bu.SHAPE:
                    r = row_of(rows, table, 0, 9)
                    assert r["n"] == 4 and r["r1"] - r["r0"] == {(4, 1): 3, (2, 2): 1, (4, 3): 1}[(ny, nx)]
                assert plan(want, 3, f.shape, steps=T)["vec"] == vec and plan(want, 3, f.shape, steps=T, aligned=False)["vec"] == 0
                check(trk, run, f, x, table, bits, rows, LDS, (T, ny, nx, dtype.__name__, want), chunks=(1,))


# ---- d. the column ring ---------------------------------------------------------------------------------------------------------------------
def rule(cols, nx):
    """(west, width) from the sorted occupied columns: the empty runs between neighbours round the circle, the longest, the lowest start"""
    c = sorted(set(cols))
    runs = [((a + 1) % nx, b - a - 1) for a, b in zip(c, c[1:] + [c[0] + nx]) if b - a > 1]
    if not runs:
        return 0, nx
    ln = max(r[1] for r in runs)
    s = min(r[0] for r in runs if r[1] == ln)
    return (s + ln) % nx, nx - ln


def ring_slab(patterns, nx, dtype):
    """pattern k, a list of columns, is id k + 1 on row k of one step"""
    f = np.zeros((1, len(patterns), nx), dtype=np.int32)
    for k, cols in enumerate(patterns):
        f[0, k, list(cols)] = k + 1
    x = np.random.default_rng(nx).permutation(f.size).reshape(f.shape).astype(dtype)
    return f, x


def ring_check(trk, f, x, patterns, nx, case):
    ids = list(range(1, len(patterns) + 1))
    with on_device(trk, f, x) as run:
        for bits in (bu.SHAPE, bu.SHAPE | bu.PEAKS):
            cap = plan(WANTS[bits], 1, f.shape)["lds_entries"]
            for form, table in ((LDS, su.table_by_row([ids])), (GLB, padded([ids], cap + 1))):
                assert (form == LDS) == (len(table[1]) <= cap)
                rows = reference(f, x, table, bits)
                got = [(int(r["west"]), int(r["width"])) for r in rows[:len(ids)]]
                assert got == [rule(cols, nx) for cols in patterns], case
                assert (rows["n"][len(ids):] == 0).all() and (rows["r0"][:len(ids)] == np.arange(len(ids))).all()
                check(trk, run, f, x, table, bits, rows, form, case + (WANTS[bits], form), chunks=(0,))


@pytest.mark.parametrize("nx", [5, 8])
@DTYPES
def test_every_occupancy_of_a_small_circle(trk, nx, dtype):
    patterns = [[c for c in range(nx) if m >> c & 1] for m in range(1, 1 << nx)]
    pairs = {rule(cols, nx) for cols in patterns}
    assert pairs == {(0, nx)} | {(w, n) for w in range(nx) for n in range(1, nx)} and len(pairs) == {5: 21, 8: 57}[nx]
    # among them the tie that only the walk's last run can win: the run from column 0 is closed last and has the lowest start
    assert nx != 8 or rule([2, 5, 7], 8) == (2, 6)
    f, x = ring_slab(patterns, nx, dtype)
    ring_check(trk, f, x, patterns, nx, (nx, dtype.__name__))


@pytest.mark.parametrize("nx", [1, 2, 31, 32, 33, 63, 64, 65, 96])
def test_ring_at_the_word_boundaries_of_the_bit_set(trk, nx):
    patterns = [[c] for c in range(nx)] + [[0, nx - 1], list(range(nx))]
    expect = [(c, 1) for c in range(nx)] + [(nx - 1, 2) if nx > 2 else (0, nx), (0, nx)]
    holes = sorted({h for h in (0, 31, 32, nx - 1) if h < nx}) if nx > 1 else []    # (no hole fits a circle of one)
    patterns += [[c for c in range(nx) if c != h] for h in holes]
    expect += [((h + 1) % nx, nx - 1) for h in holes]
    if nx % 2 == 0 and nx >= 8:                                                     # two equal gaps: the lower start wins -- the last
        for k in (0, 3, nx // 2 - 1):                                               # pair's second gap starts at column 0
            patterns.append([k, k + nx // 2])
            expect.append((k + nx // 2 if k < nx // 2 - 1 else k, nx // 2 + 1))
    if nx % 3 == 0 and nx >= 6:                                                     # ... and three
        patterns.append([1, 1 + nx // 3, 1 + 2 * (nx // 3)])
        expect.append((1 + nx // 3, nx - nx // 3 + 1))
    if nx >= 31:                                                                    # the tie won by the run that starts at column 0
        k = (nx - 1) // 3
        assert nx - 2 * k - 3 <= k and 2 * k + 1 < nx - 1
        patterns.append([k, 2 * k + 1, nx - 1])
        expect.append((k, nx - k))
    assert [rule(cols, nx) for cols in patterns] == expect
    f, x = ring_slab(patterns, nx, np.float32)
    ring_check(trk, f, x, patterns, nx, (nx,))


# ---- e. values ------------------------------------------------------------------------------------------------------------------------------
# the bits of -NaN, a quiet NaN with a payload and a negative signalling NaN
NANS = {np.float32: np.array([0xffc00000, 0x7fc12345, 0xff800001], dtype=np.uint32).view(np.float32),
        np.float64: np.array([0xfff8000000000000, 0x7ff8123400000005, 0xfff0000000000001], dtype=np.uint64).view(np.float64)}
SAME, ZEROS = 61, 62


@functools.lru_cache(maxsize=None)
def value_slab(dtype):
    """(flag, x, the slices of its two steps, what the preconditions need): the value cases on rows of their own at step 0, a 50-pixel
    block of one value across the part boundary at step 0 and one of -0.0 at step 1"""
    ny, nx = 40, 104
    part = _native.blockstat_plan("peaks", 1, ny, nx)["part_lanes"] * 4
    assert part < ny * nx and part % _native.blockstat_plan("peaks", 1, ny, nx)["part_lanes"] == 0          # a boundary of both forms
    f = np.zeros((2, ny, nx), dtype=np.int32)
    background(f)
    x = np.random.default_rng(7).permutation(f.size).reshape(f.shape).astype(dtype) / 8 - 99
    fi = np.finfo(dtype)
    tiny, fmax, one = dtype(fi.smallest_subnormal), dtype(fi.max), dtype(1)
    assert tiny > 0 and tiny / 2 == 0 and np.isfinite(fmax) and fmax == np.nextafter(dtype(INF), dtype(0))
    neg_nan, payload, neg_snan = NANS[dtype]
    assert all(np.isnan(v) for v in (neg_nan, payload, neg_snan)) and np.signbit(neg_nan) and np.signbit(neg_snan) and not np.signbit(payload)
    A = lambda *v: np.array(v, dtype=dtype)
    values = {51: A(neg_nan, 2.5, payload), 52: A(neg_nan, neg_nan, neg_nan), 53: A(tiny, 0.0, -0.0, -tiny), 54: A(fmax, INF, -INF, -fmax),
              55: A(-fmax, fmax, fmax, -fmax), 56: A(1.0, one + dtype(2.0 ** -20), 1.0), 57: A(1.0, 1.0 + 2.0 ** -40, 1.0), 58: A(neg_snan, -tiny, -0.0),
              59: A(payload, neg_snan, -INF, neg_nan)}
    for k, (i, v) in enumerate(values.items()):
        f[0, k, 4:4 + len(v)] = i
        x[0, k, 4:4 + len(v)] = v
        assert x[0, k, 4:4 + len(v)].tobytes() == v.tobytes()                       # sign and payload of the NaNs arrive
    lo = part - 25
    f[0].reshape(-1)[lo:lo + 50] = SAME
    x[0].reshape(-1)[lo:lo + 50] = 2.5
    f[1].reshape(-1)[lo:lo + 50] = ZEROS
    x[1].reshape(-1)[lo:lo + 50] = -0.0
    return f, x, [sorted(values) + [SAME], [ZEROS]], lo


@FORMS
@DTYPES
def test_values_at_the_ends_of_the_key_order(trk, dtype, form):
    f, x, slices, lo = value_slab(dtype)
    nx = f.shape[2]
    cap = plan("peaks", 1, f.shape)["lds_entries"]
    assert cap >= plan("shape", 1, f.shape)["lds_entries"]
    table = su.table_by_row(slices) if form == LDS else padded(slices, cap + 1)
    rows = reference(f, x, table, bu.SHAPE | bu.PEAKS)
    row = lambda t, i: row_of(rows, table, t, i)
    p = lambda i: (i - 51) * nx + 4                                                  # the first pixel of a value case
    tiny, fmax = (float(v) for v in (np.finfo(dtype).smallest_subnormal, np.finfo(dtype).max))
    peaks = lambda i: tuple(row(0, i)[n] for n in ("n", "nv", "max", "max_p", "min", "min_p"))
    assert peaks(51) == (3, 1, 2.5, p(51) + 1, 2.5, p(51) + 1)
    assert peaks(52)[:2] == (3, 0) and np.isnan(row(0, 52)["max"]) and np.isnan(row(0, 52)["min"]) and (row(0, 52)["max_p"], row(0, 52)["min_p"]) == (-1, -1)
    assert peaks(53) == (4, 4, tiny, p(53), -tiny, p(53) + 3) and 0 < tiny < 1e-44
    assert peaks(54) == (4, 4, INF, p(54) + 1, -INF, p(54) + 2)
    assert peaks(55) == (4, 4, fmax, p(55) + 1, -fmax, p(55))
    assert peaks(56) == (3, 3, 1.0 + 2.0 ** -20, p(56) + 1, 1.0, p(56))
    assert peaks(57) == ((3, 3, 1.0 + 2.0 ** -40, p(57) + 1, 1.0, p(57)) if dtype == np.float64 else (3, 3, 1.0, p(57), 1.0, p(57)))
    assert peaks(58)[:2] == (3, 2) and (row(0, 58)["min"], row(0, 58)["min_p"], row(0, 58)["max_p"]) == (-tiny, p(58) + 1, p(58) + 2) and np.signbit(row(0, 58)["max"])
    assert peaks(59) == (4, 1, -INF, p(59) + 2, -INF, p(59) + 2)
    part = plan("peaks", 1, f.shape)["part_lanes"] * 4
    assert lo < part < lo + 49
    assert peaks(SAME) == (50, 50, 2.5, lo, 2.5, lo)
    z = row(1, ZEROS)
    assert (z["n"], z["nv"], z["max_p"], z["min_p"]) == (50, 50, lo, lo) and z["max"] == 0 and np.signbit(z["max"]) and np.signbit(z["min"])
    with on_device(trk, f, x) as run:
        for bits in WANTS:
            want_rows = rows if bits == bu.SHAPE | bu.PEAKS else reference(f, x, table, bits)
            check(trk, run, f, x, table, bits, want_rows, form, (dtype.__name__, WANTS[bits], form))       # (peaks fit the most: all wants share the form)
