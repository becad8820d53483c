"""The local wave activity kernels at their capacity and scan edges, against the numpy statement tests/lwa_util.py by bit pattern, the
output and the contours alike (test_gpu_lwa.both_same).  What tests/test_gpu_lwa.py never reaches, one group of CASES each:
    cap     one domain of 2 043 rows, all active: k_lwa_contour at exactly 65 536 bytes of dynamic LDS, k_lwa_integral<double, true>
            at 65 376, strips of one unit in both forms
    scan    1 023, 1 024 and 1 025 active rows: one and two buckets per thread in the suffix scan, the latter also with gaps
    weight  the 2 043-row table with all weights 2^32 - 1 (bucket sums near 2^45) and all 1
    probe   n_act at and beside every power of two up to 512: exactly enough halvings of the search over the pivots
    strip   600 rows in strips of one vector unit and in scalar strips of 3 + 2 columns, 1 030 rows in five strips of one column,
            under every workgroup-to-XCD mapping and with fewer workgroups than strips
    pair    two domains of unequal length, one of them possibly without an active row, walked by ONE workgroup: the LDS words of
            one (step, domain) are reused by the next
    zero    zero-weight rows inside a domain: equal caps, equal pivots; a plane whose weighted pixels are all equal
    round   exactly 1 round (two adjacent keys; -0.0 / +0.0, across the sign bit), the full 32 / 64 rounds (-max .. +max), and rows
            out of reach behind NaNs, where the clamp of the search is taken
tests/test_lwa_host.py checks without a GPU that every case reaches the edge it is named for, that the statement is the per-pixel
loop on it, and that no ordinary case could pass with an all-zero output.  The statement of a case is computed once (want)."""
import functools

import numpy as np
import pytest

import lwa_util as lu
from contrack_amd import _native
from test_gpu_lwa import SCALAR, VECTOR, both_same, on_device

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PROBE_NA = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)
POWERS = tuple(na for na in PROBE_NA if na & (na - 1) == 0)
MODES, GRID_CAPS = (-1, 0, 1, 2), (0, 1, 7)


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def tag(dtype):
    return "f64" if dtype == F64 else "f32"


# ---- the cases: name -> (group, builder of (z, table), ordinary: at least half of the statement's active pixels are not 0) --------------
CASES = {}


def add(group, name, build, ordinary=True):
    assert name not in CASES
    CASES[name] = (group, build, ordinary)


def full(n):
    return lu.custom_table([n], [range(n)])


def last_active(n, na):
    return lu.custom_table([n], [range(n - na, n)])


def scattered():
    """1 024 active rows with gaps among 2 043"""
    return lu.custom_table([2043], [np.sort(np.random.default_rng(1024).choice(2043, 1024, replace=False))])


def steep(table, nx, steps, seed, dtype, noise=60.0):
    def build():
        tab = table()
        return lu.steep_field(tab, nx, steps, seed, dtype, noise), tab
    return build


for nx, dtype in ((4, F32), (4, F64), (1, F32), (3, F32)):
    add("cap", "cap-nx%d-%s" % (nx, tag(dtype)), steep(functools.partial(full, 2043), nx, 2, 2043 + nx, dtype))
for nx in (4, 5):
    for na in (1023, 1024, 1025):
        for dtype in (F32, F64) if na == 1024 else (F32,):
            add("scan", "scan-na%d-nx%d-%s" % (na, nx, tag(dtype)), steep(functools.partial(last_active, 1030, na), nx, 2, na + nx, dtype))
    for dtype in (F32, F64):
        add("scan", "scan-gaps-nx%d-%s" % (nx, tag(dtype)), steep(scattered, nx, 2, 77 + nx, dtype))
for kind in ("max", "one"):
    add("weight", "weight-" + kind, steep(functools.partial(lu.custom_table, [2043], [range(2043)], kind), 4, 2, 5, F32))
for nx, dtype, nas in ((3, F32, PROBE_NA), (4, F32, PROBE_NA), (3, F64, POWERS), (4, F64, POWERS)):
    for na in nas:                                                               # n = n_act + 3: two inactive rows before, one behind; weather alone, as few as 3 pixels must cross
        add("probe", "probe-na%d-nx%d-%s" % (na, nx, tag(dtype)), steep(functools.partial(lu.custom_table, [na + 3], [range(2, na + 2)]), nx, 1, 10 * na + nx, dtype, 2000.0))


def half(n):
    return lu.custom_table([n], [range(1, n, 2)])


add("strip", "strip-600-nx24", steep(functools.partial(half, 600), 24, 3, 624, F32))
add("strip", "strip-600-nx5", steep(functools.partial(half, 600), 5, 3, 605, F32))
add("strip", "strip-1030-nx5", steep(functools.partial(half, 1030), 5, 3, 1035, F32))
# what ctk_lwa_plan gives them: (rows, nx) -> (vec, strip, nstrips)
STRIP_PLANS = {"strip-600-nx24": (600, 24, (1, 4, 6)), "strip-600-nx5": (600, 5, (0, 3, 2)), "strip-1030-nx5": (1030, 5, (0, 1, 5))}

TEN = range(20, 30)
PAIRS = {"long-short": ([700, 37], [range(700), TEN], False), "short-long": ([37, 700], [TEN, range(700)], False),
         "idle-short": ([700, 37], [[], TEN], False), "short-idle": ([37, 700], [TEN, []], False),
         "shared": ([700, 37], [range(1, 700), TEN], True)}
for pair, (lengths, active, shared) in PAIRS.items():
    for nx in (4, 5):
        add("pair", "pair-%s-nx%d" % (pair, nx), steep(functools.partial(lu.custom_table, lengths, active, "cos", None, shared), nx, 3, len(pair) + nx, F32, 150.0))

ZERO_ROWS, ZERO_ACTIVE = (17, 18, 19, 20), range(10, 35)                           # positions of a 40-row domain; 18 and 19 are active AND weigh nothing


def zero_table():
    W = lu.custom_table([40], [ZERO_ACTIVE])["W"].copy()
    W[[39 - p for p in ZERO_ROWS]] = 0                                           # (position p of the one domain is row 39 - p)
    return lu.custom_table([40], [ZERO_ACTIVE], W)


def zero_flat(dtype):
    """5 500 m on every weighted row, weather on the four rows that weigh nothing: no round, and yet not a constant plane"""
    def build():
        tab = zero_table()
        z = lu.steep_field(tab, 8, 2, 40, dtype, 300.0)
        z[:, tab["W"] != 0, :] = dtype(5500.0)
        return z, tab
    return build


for dtype in (F32, F64):
    add("zero", "zero-steep-" + tag(dtype), steep(zero_table, 8, 2, 41, dtype, 150.0))
    add("zero", "zero-flat-" + tag(dtype), zero_flat(dtype))


def round_table():
    return lu.custom_table([40], [range(1, 38)])


def valued(pick, dtype):
    def build():
        tab = round_table()
        lo, hi = pick(dtype)
        return lu.two_valued(tab, 8, 2, lo, hi, 8, dtype), tab
    return build


def holes(dtype):
    """a fifth of the pixels of step 0 are NaN: the rows next to the equator are out of reach there, and the clamp is taken"""
    def build():
        tab = round_table()
        return lu.sprinkle(lu.steep_field(tab, 8, 2, 9, dtype, 150.0), tab, [np.nan], share=0.2, seed=3, steps=[0]), tab
    return build


TWO_VALUES = {"adjacent": lambda dt: (dt(5500.0), np.nextafter(dt(5500.0), dt(np.inf))), "zeros": lambda dt: (dt(-0.0), dt(0.0)),
              "span": lambda dt: (-np.finfo(dt).max, np.finfo(dt).max)}
for dtype in (F32, F64):
    for name, pick in TWO_VALUES.items():
        add("round", "round-%s-%s" % (name, tag(dtype)), valued(pick, dtype), ordinary=False)
    add("round", "round-nan-" + tag(dtype), holes(dtype))


def names(group):
    return [name for name, (g, _, _) in CASES.items() if g == group]


@functools.lru_cache(maxsize=None)
def case(name):
    """(z, table) of a case, built once and read-only from then on"""
    z, tab = CASES[name][1]()
    z.setflags(write=False)
    for v in tab.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return z, tab


@functools.lru_cache(maxsize=None)
def want(name, part=0):
    """the statement (out, ref) of a case, computed once"""
    z, tab = case(name)
    out, ref = lu.from_table(z, tab, part, return_ref=True)
    out.setflags(write=False)
    ref.setflags(write=False)
    return out, ref


def form_of(z, off=0):
    return VECTOR if z.shape[2] % 4 == 0 and off == 0 else SCALAR


def entries(trk, name, parts=(0,)):
    """the host entry, the _dev entry on aligned pointers and the _dev entry one element past a 16-byte boundary (the scalar form)"""
    z, tab = case(name)
    for part in parts:
        w = want(name, part)
        assert both_same(trk.lwa(z, tab, part=part, want_ref=True), w), (name, part, "host")
        assert trk.debug_lwa_form() == form_of(z)
        for off in (0, z.itemsize):
            assert both_same(on_device(trk, z, tab, part, off=off), w), (name, part, off)
            assert trk.debug_lwa_form() == form_of(z, off), (name, off)


# ---- a: the capacity edge, accepted side (2 044 rows are refused: test_gpu_lwa.test_argument_errors_leave_the_handle_usable) --------------
@pytest.mark.parametrize("name", names("cap"))
def test_2043_rows_at_the_lds_limit_of_both_kernels(trk, name):
    z, _tab = case(name)
    p = _native.lwa_plan(z.itemsize, 2043, z.shape[2])
    assert p["ok"] == 1 and p["lds_sel"] == 65536 and p["lds"] == 2043 * z.itemsize * (4 if p["vec"] else 1)
    entries(trk, name, parts=(0, 1, 2) if name == "cap-nx4-f32" else (0,))


# ---- b: one and two buckets per thread of the suffix scan ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("scan"))
def test_suffix_scan_at_1023_1024_and_1025_active_rows(trk, name):
    z, tab = case(name)
    assert both_same(trk.lwa(z, tab, want_ref=True), want(name)), name
    assert trk.debug_lwa_form() == form_of(z)


# ---- c: the largest and the smallest weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("weight"))
def test_weights_of_all_ones_and_all_2_to_32_minus_1(trk, name):
    z, tab = case(name)
    assert both_same(trk.lwa(z, tab, want_ref=True), want(name)), name
    assert both_same(on_device(trk, z, tab), want(name)), name


# ---- d: the halvings of the search over the pivots ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx, dtype", [(3, F32), (4, F32), (3, F64), (4, F64)], ids=["nx3-f32", "nx4-f32", "nx3-f64", "nx4-f64"])
def test_active_rows_at_and_beside_every_power_of_two(trk, nx, dtype):
    for na in PROBE_NA if dtype == F32 else POWERS:
        name = "probe-na%d-nx%d-%s" % (na, nx, tag(dtype))
        z, tab = case(name)
        assert int(tab["active"].sum()) == na and z.shape == (1, na + 3, nx)
        assert both_same(trk.lwa(z, tab, want_ref=True), want(name)), name


# ---- e: strips of one unit --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("strip"))
def test_narrow_strips_under_every_mapping_and_grid_cap(trk, name):
    z, tab = case(name)
    rows, nx, (vec, strip, nstrips) = STRIP_PLANS[name]
    p = _native.lwa_plan(4, rows, nx, 1, 3)
    assert (p["vec"], p["strip"], p["nstrips"], p["blocks"]) == (vec, strip, nstrips, 3 * nstrips) and z.shape == (3, rows, nx)
    try:
        for mode in MODES:
            for cap in GRID_CAPS:
                trk.debug_set_lwa(mode, cap)
                assert both_same(trk.lwa(z, tab, want_ref=True), want(name)), (name, mode, cap)
                assert trk.debug_lwa_launch() == (vec, min(cap or p["blocks"], p["blocks"]))
    finally:
        trk.debug_set_lwa()


# ---- f: unequal domains through one workgroup -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("pair"))
def test_unequal_and_idle_domains_walked_by_one_workgroup(trk, name):
    z, tab = case(name)
    assert z.shape[0] == 3 and int(tab["ndom"]) == 2
    try:
        for cap in (1, 0):
            trk.debug_set_lwa(-1, cap)
            assert both_same(trk.lwa(z, tab, want_ref=True), want(name)), (name, cap)
            assert both_same(on_device(trk, z, tab), want(name)), (name, cap)
            if cap:
                assert trk.debug_lwa_launch()[1] == 1
    finally:
        trk.debug_set_lwa()


# ---- g: zero-weight rows inside a domain --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("zero"))
def test_zero_weight_rows_inside_a_domain(trk, name):
    z, tab = case(name)
    for part in (0, 1, 2):
        assert both_same(trk.lwa(z, tab, part=part, want_ref=True), want(name, part)), (name, part)
    assert both_same(on_device(trk, z, tab, off=z.itemsize), want(name)), name


# ---- h: the number of rounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("round"))
def test_one_round_all_rounds_and_the_clamp(trk, name):
    z, tab = case(name)
    for part in (0, 1, 2):
        assert both_same(trk.lwa(z, tab, part=part, want_ref=True), want(name, part)), (name, part)
    assert both_same(on_device(trk, z, tab), want(name)), name
    assert both_same(on_device(trk, z, tab, off=z.itemsize), want(name)), name
