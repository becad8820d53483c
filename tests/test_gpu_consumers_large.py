"""The device-pointer entries of the map consumers past 2^31 and 2^32 elements: spells, composite, band, block-centred composite, level
mean, reversal, std field, percentile field and percentile groups on the shape of tests/test_gpu_frequency_large.py, 4200 x 721 x 1440
(4.36 G elements, 17.4 GB per slab).  No host slab: a slab is a memset background plus four windows of 24 steps (tests/large_util.py)
-- A wholly below element 2^31, B across it, C across element 2^32, D the last steps -- whose contents differ from the background only
in a few patches of the plane.  Every expected value is an existing numpy statement evaluated on the windows and patches by
large_util, which tests/test_large_util_host.py proves equal to the statement on the whole slab, and dependent on C and on D, at a
size that fits; comparisons are those of the small tests: equal counts, equal bits of the float64 sums, no tolerance.

float64 slabs are left out: the kernels are templates over the value type and their offsets count elements, so a float64 slab of
this length would double the memory without any new index arithmetic.
Needs ~55 GB of device memory (three slabs) and ~2 GB of host memory."""
import ctypes as C

import numpy as np
import pytest

import band_util
import composite_util
import large_util as lu
import level_util

from contrack_amd import _native

pytestmark = pytest.mark.gpu

L = lu.LAYOUT_FULL
T, NY, NX, NPIX = L.T, L.ny, L.nx, L.npix
SLAB = T * NPIX * 4
G = 12


class _Slabs:
    """one handle, three device slabs, and what each of them holds (a large_util.Sparse, or None after something else was written)"""

    def __init__(self, trk, ptrs):
        self.trk, self.p, self.holds = trk, ptrs, [None] * len(ptrs)
        self.flag, self.field, self.level = lu.flag_spec(L), lu.field_spec(L), lu.level_spec(L)
        self.ids = L.ids()
        self.lists = {}
        self.life = None                                                            # the lifecycle field, built by its test

    def put(self, k, spec):
        if self.holds[k] is not spec:
            self.holds[k] = None
            lu.place(self.trk, self.p[k], spec)
            self.holds[k] = spec
        return self.p[k]

    def scratch(self, k, byte=None, nbytes=SLAB):
        """slab k as an output: no longer what it held, poisoned with `byte`"""
        self.holds[k] = None
        if byte is not None:
            self.trk.memset(self.p[k], byte, nbytes)
        return self.p[k]

    def spell_lists(self, by_id, segments):
        key = (by_id, tuple(segments) if segments else None)
        if key not in self.lists:
            self.lists[key] = lu.spell_lists(L, self.flag, by_id, segments)
        return self.lists[key]


@pytest.fixture(scope="module")
def big():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    trk = _native.Tracker(0)
    ptrs = []
    try:
        for _ in range(3):
            ptrs.append(trk.malloc(SLAB))
    except MemoryError as e:
        for p in ptrs:
            trk.free(p)
        trk.close()
        pytest.fail("the consumers' slabs need 3 x %.1f GB of device memory: %s" % (SLAB / 1e9, e))
    yield _Slabs(trk, ptrs)
    for p in ptrs:
        trk.free(p)
    trk.close()


def _same_maps(got, want, case):
    for name, g, w in zip(("events", "steps", "longest"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (case, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (case, name, int(np.count_nonzero(g != w)), np.argwhere(g != w)[:4].tolist())


def test_shape_crosses_both_marks():
    assert T * NPIX > 2 ** 32
    assert 2 ** 31 // NPIX == 2068 and 2 ** 32 // NPIX == 4136
    a, b, c, d = L.firsts
    assert (a + L.n) * NPIX < 2 ** 31                                             # A: wholly below
    assert b <= 2068 < b + L.n and b * NPIX < 2 ** 31 < (b + L.n) * NPIX            # B holds element 2^31
    assert c <= 4136 < c + L.n and c * NPIX < 2 ** 32 < (c + L.n) * NPIX            # C holds element 2^32
    assert d == T - L.n and c < L.seg_start < c + L.n
    assert L.level_steps * L.nlev == T and [s * L.nlev for s in L.level_firsts] == [20, 2056, 4124, T - 24]
    assert 2 ** 31 // (L.nlev * NPIX) == 517 and 2 ** 32 // (L.nlev * NPIX) == 1034


@pytest.mark.parametrize("segments", [None, [0, L.seg_start]], ids=["whole", "segments"])
@pytest.mark.parametrize("by_id", [True, False])
def test_spells_in_windows(big, by_id, segments):
    flag = big.put(0, big.flag)
    lists = big.spell_lists(by_id, segments)
    assert len(lists[0]) > 4 * len(L.patch_pixels())
    for ng, ids in ((1, None), (G, big.ids)):
        for md in (1, 3):
            got = big.trk.spells_dev(flag, T, NY, NX, group=ids, ngroups=ng, by_id=by_id, min_duration=md, segments=segments)
            _same_maps(got, lu.want_spells(L, lists, ids, ng, md), (by_id, segments, ng, md))


def test_spells_solid_slab_one_run_across_both_marks(big):
    """every byte 0x01, the last 10 steps zeroed and 1 001 pixels of step 4185: one spell of 4190 steps per pixel in the group of step 0,
    which the thread of the first slice follows over both marks; in the block two spells, of 4185 and 4 steps"""
    flag = big.scratch(0)
    lu.place_solid(big.trk, flag, L)
    for ng, ids, md in ((1, None, 1), (G, big.ids, 1), (G, big.ids, 5), (1, None, 4186)):
        got = big.trk.spells_dev(flag, T, NY, NX, group=ids, ngroups=ng, min_duration=md)
        want = lu.want_spells_solid(L, ids, ng, md)
        _same_maps(got, want, ("solid", ng, md))
    assert want[0].sum() == NPIX - L.patches[1][1] and want[2].max() == T - 10      # (min_duration 4186: the block's pixels have none)


@pytest.mark.parametrize("skipna", [False, True])
def test_composite(big, skipna):
    flag, x = big.put(0, big.flag), big.put(1, big.field)
    for ng, ids in ((1, None), (G, big.ids)):
        s, n = big.trk.composite_dev(flag, x, T, NY, NX, group=ids, ngroups=ng, skipna=skipna)
        ws, wn = lu.want_composite(L, big.flag, big.field, ids, ng, skipna)
        assert wn.any() and np.array_equal(n, wn), (skipna, ng, int(np.count_nonzero(n != wn)))
        assert composite_util.same_bits(s, ws), (skipna, ng, composite_util.differing(s, ws))


def test_band(big):
    flag, x = big.put(0, big.flag), big.put(1, big.field)
    w = 111.0 ** 2 * 0.0625 * np.cos(np.deg2rad(np.asarray(L.lat, dtype=np.float64)))                # float64 row weights
    got = big.trk.band_dev(flag, x, T, NY, NX, L.band_rows, w, sectors=L.sectors, columns=True)
    want = lu.want_band(L, big.flag, big.field, w)
    assert want["cnt"].shape == (T, NX) and want["sec_cnt"].shape == (T, 2) and want["cnt"][L.firsts[2]:].any()
    band_util.same(got, want, "band")


@pytest.mark.parametrize("form", [0, 1], ids=["plain", "fed"])
def test_centred(big, form):
    x = big.put(1, big.field)
    p2, pl = L.patches[1][0] + 500, NPIX - 200
    marks = [(2067, NPIX - 1), (2068, 100), (2068, p2), (4135, NPIX - 1), (4136, p2), (4136, pl), (L.firsts[0], 0), (T - 1, 0), (T - 1, NPIX - 1)]
    assert 2067 * NPIX + NPIX - 1 < 2 ** 31 < 2068 * NPIX + p2 and 4136 * NPIX + p2 < 2 ** 32 < 4136 * NPIX + pl
    st = lu.stamps(L, big.field, R=40, nbins=3, marks=marks)
    assert (st[3] < 0).any() and all(np.isin(t0 + np.arange(L.n), st[0]).any() for t0 in L.firsts)
    big.trk.debug_set_centred(form)
    try:
        for skipna in (False, True):
            s, n = big.trk.centred_dev(x, T, NY, NX, st[0], st[1], st[2], st[3], 3, 2, 3, wrap=True, skipna=skipna)
            assert big.trk.debug_centred_launch()[0] == form
            ws, wn = lu.want_centred(L, big.field, st, 3, 2, 3, skipna)
            assert np.array_equal(n, wn), (form, skipna)
            assert composite_util.same_bits(s, ws), (form, skipna, composite_util.differing(s, ws))
    finally:
        big.trk.debug_set_centred(-1)


def test_lifecycle(big):
    """the rows per (step, id) -- ids 1..3, so every id has pixels in every patch and most cross the seam -- as the small tests compare
    them (tests/test_gpu_lifecycle_forms.py): step, id, roll and area equal, the three weighted sums within rtol 1e-12 of numpy's
    pairwise sums; and some rows of every window bit for bit in the reference's own summation orders"""
    import life_util
    if big.life is None:
        big.life = lu.life_field_spec(L)
    flag, x = big.put(0, big.flag), big.put(2, big.life)
    wrow = lu.life_wrow(L)
    rows = big.trk.lifecycle_dev(flag, x, T, NY, NX, wrow)
    want = lu.want_life(L, big.flag, big.life, wrow)
    assert len(want) >= 3 * 4 * L.n - 8 and (want["shift"] > 0).any() and len(rows) == len(want)
    for k in ("t", "label", "shift", "area"):
        assert np.array_equal(rows[k], want[k]), k
    for k in ("swv", "swvy", "swvx"):
        assert np.allclose(rows[k], want[k], rtol=1e-12, atol=1e-9), k
    idx = np.flatnonzero(np.isin(want["t"], [t0 + d for t0 in L.firsts for d in (8, L.n - 1)]))
    ex = big.trk.lifecycle_exact(idx)
    exact = lu.want_life_exact(L, big.flag, big.life, wrow, want[idx])
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(ex[k], exact[k]), k


def _same_field(got, ref, case):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (case, got.dtype, got.shape, ref.dtype, ref.shape)
    bad = np.argwhere(~((got == ref) | ((got != got) & (ref != ref))))
    first = [tuple(b) for b in bad[:4].tolist()]
    assert np.array_equal(got, ref, equal_nan=True), (case, len(bad), "at", first, "got", [got[b] for b in first], "want", [ref[b] for b in first])


@pytest.mark.parametrize("skipna", [True, False])
def test_std_field(big, skipna):
    x = big.put(1, big.field)
    y0, y1 = L.std_rows
    field, ms, tile = big.trk.time_std_field(x, T, NY, NX, y0, y1, big.ids, G, window=3, ddof=1, skipna=skipna, reps=1, want_field=True)
    assert ms > 0 and tile == 32
    want = lu.want_std(L, big.field, big.ids, G, 3, 1, skipna)
    assert np.isfinite(want).any()
    _same_field(field, want, ("std", skipna))


def test_percentile_field(big):
    x = big.put(1, big.field)
    y0, y1 = L.std_rows
    pool = 3 * (T // G)
    plan = _native.debug_percentile_field_plan(4, pool, G, 3)
    want = lu.want_pfield(L, big.field, big.ids, G, 3)
    assert lu.PCTL_QS[0] == 0.9 and np.unique(want[1]).size > 1000 and np.unique(want[2]).size > 1000         # (q = 0.9 alone gives the background)
    for q, w in zip(lu.PCTL_QS, want):
        chosen, direct, ms, ms_direct, ms_read, form = big.trk.time_percentile_field(x, T, NY, NX, y0, y1, big.ids, G, q, window=3, reps=1)
        assert form == plan["form"] == 1 and ms > 0 and ms_direct > 0                # the ring form: 1050 steps per pool
        _same_field(chosen, w, ("ring", q))
        _same_field(direct, w, ("direct", q))


def test_percentile_groups(big):
    x = big.put(1, big.field)
    y0, y1 = L.std_rows
    want = lu.want_pgroups(L, big.field, big.ids, G, 3)
    assert np.all(want[1] < big.field.background) and np.all(want[2] > big.field.background)
    for q, w in zip(lu.PCTL_QS, want):
        got = big.trk.time_percentile_groups(x, T, NY, NX, y0, y1, big.ids, G, q, window=3, reps=1)[0]
        assert got.dtype == np.float64 and got.shape == (G,) and np.array_equal(got, w, equal_nan=True), (q, got.tolist(), w.tolist())


def _check_windows(trk, out, steps, wins, case):
    """the windows of a float32 result (steps, ny, nx) against `wins`; the planes next to each window and the first and the last plane
    are +0.0, and the whole result has no more non-zero words than the windows"""
    plane = NPIX * 4
    zero_steps = {0, steps - 1}
    for t0, w in wins:
        got = np.empty(w.shape, dtype=np.float32)
        trk.d2h(got, lu._off(out, t0 * plane))
        assert level_util.same_bits(got, w), (case, "window at step", t0, level_util.differing(got, w))
        zero_steps |= {t0 - 1, t0 + len(w)}
    inside = set()
    for t0, w in wins:
        inside |= set(range(t0, t0 + len(w)))
    one = np.empty((NY, NX), dtype=np.int32)
    for t in sorted(t for t in zero_steps if 0 <= t < steps and t not in inside):
        trk.d2h(one, lu._off(out, t * plane))
        assert not one.any(), (case, "background step", t, int(np.count_nonzero(one)))
    nz = lu.nonzero_words(wins)
    assert nz > 0 and trk.checksum_i32(out, steps * NPIX, 0)[1] == nz, (case, nz)


@pytest.mark.parametrize("skipna", [False, True])
def test_level_mean(big, skipna):
    """1050 steps of 4 levels: the same 17.4 GB; the input offset passes 2^31 in step 517 and 2^32 in step 1034"""
    x = big.put(2, big.level)
    steps = L.level_steps
    out = big.scratch(0, 0xff, steps * NPIX * 4)                                  # (every pixel of the result must be WRITTEN)
    w = [0.5, 0, 1.5, 1]
    big.trk.level_mean_dev(x, steps, L.nlev, NY, NX, w, out, skipna=skipna)
    _check_windows(big.trk, out, steps, lu.want_level(L, big.level, w, skipna), ("level", skipna))


@pytest.mark.parametrize("mask", [False, True])
def test_reversal(big, mask):
    x = big.put(1, big.field)
    out = big.scratch(2, 0xff)
    tab = L.reversal_table()
    big.trk.reversal_dev(x, T, NY, NX, tab, out, mask=mask)
    _check_windows(big.trk, out, T, lu.want_reversal(L, big.field, tab, mask), ("reversal", mask))
