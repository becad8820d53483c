"""The premise of tests/test_gpu_consumers_large.py at a size where the whole slab fits (60 x 9 x 40): for every entry, what large_util
builds from the windows and patches equals the numpy statement on the materialised slab bit for bit -- in particular a step without a
flag adds nothing, so compaction keeps the order of the float64 additions -- and it changes when window C or window D is taken away: a
kernel that never reads beyond the third window's first element, or reads background in its place, cannot give it."""
import numpy as np
import pytest

import band_util
import centred_util
import composite_util
import large_util as lu
import level_util
import pctl_util
import pfield_util
import reversal_util
import spell_util
import std_util

L = lu.LAYOUT_SMALL
FLAG, FIELD, LEVEL = lu.flag_spec(L), lu.field_spec(L), lu.level_spec(L)
IDS = L.ids()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    """equal dtype, shape and bits, NaNs by position"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def _all_same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return _same(a, b)


def _each_differs(a, b):
    """every output of a differs from its partner in b"""
    if isinstance(a, dict):
        return all(not _same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return all(not _same(x, y) for x, y in zip(a, b))
    return not _same(a, b)


def _premise(build, statement, pick=lambda out: out):
    """build(flag, field, level) from the sparse slabs == statement(dense flag, dense field, dense level); without C, without D: another
    result in every output (pick: the outputs that depend on the values at all)"""
    want = build(FLAG, FIELD, LEVEL)
    assert _all_same(want, statement(FLAG.dense(), FIELD.dense(), LEVEL.dense()))
    for k in (2, 3):
        assert _each_differs(pick(want), pick(build(FLAG.without(k), FIELD.without(k), LEVEL.without(k)))), "window %s changes nothing" % "ABCD"[k]


def test_layouts_and_slabs():
    F = lu.LAYOUT_FULL
    assert F.T * F.npix > 2 ** 32
    assert F.firsts[1] * F.npix < 2 ** 31 < (F.firsts[1] + F.n) * F.npix and F.firsts[2] * F.npix < 2 ** 32 < (F.firsts[2] + F.n) * F.npix
    assert F.patches[:2] == ((0, 512), (517_003, 1_001)) and F.patches[-1] == (F.npix - 515, 515)
    d = FLAG.dense()
    inside = np.zeros(L.npix, dtype=bool)
    inside[L.patch_pixels()] = True
    assert not d.reshape(L.T, -1)[:, ~inside].any() and d.max() == 3 and all(d[t0:t0 + L.n].any() for t0 in L.firsts)
    assert not np.delete(d, FLAG.steps(), axis=0).any()
    x = FIELD.dense().reshape(L.T, -1)
    assert np.all(x[:, ~inside] == FIELD.background) and FIELD.background != 0 and np.isnan(x).any()
    assert np.array_equal(FLAG.steps(), FIELD.steps()) and np.array_equal(FLAG.compact()[0], d[FLAG.steps()])
    assert LEVEL.background == 0.0 and np.array_equal(FIELD.rows(4, 6), FIELD.dense()[:, 4:6], equal_nan=True)


@pytest.mark.parametrize("by_id", [True, False])
@pytest.mark.parametrize("segments", [None, [0, L.seg_start]])
def test_spells(by_id, segments):
    for G, ids in ((1, None), (12, IDS)):
        for md in (1, 3):
            _premise(lambda f, x, lv: lu.want_spells(L, lu.spell_lists(L, f, by_id, segments), ids, G, md),
                     lambda f, x, lv: tuple(m.astype(np.uint32) for m in spell_util.spells(f, ids, G, 0, by_id, md, segments)))


def test_spells_solid():
    d = lu.solid_dense(L)
    for G, ids in ((1, None), (12, IDS)):
        for md in (1, 3):
            want = lu.want_spells_solid(L, ids, G, md)
            assert _all_same(want, tuple(m.astype(np.uint32) for m in spell_util.spells(d, ids, G, 0, True, md)))
    assert lu.want_spells_solid(L, None, 1, 1)[2].max() == L.T - 10


@pytest.mark.parametrize("skipna", [False, True])
def test_composite(skipna):
    for G, ids in ((1, None), (12, IDS)):
        _premise(lambda f, x, lv: lu.want_composite(L, f, x, ids, G, skipna), lambda f, x, lv: composite_util.composite(f, x, ids, G, 0, skipna))


def test_band():
    w = band_util.order_weights(L.ny)
    y0, y1 = L.band_rows
    _premise(lambda f, x, lv: lu.want_band(L, f, x, w), lambda f, x, lv: band_util.band(f, y0, y1, w, 0, x, L.sectors, True))


@pytest.mark.parametrize("skipna", [False, True])
def test_centred(skipna):
    marks = [(L.firsts[2], L.patches[-1][0]), (L.T - 1, L.npix - 1), (L.firsts[3], 0)]
    st = lu.stamps(L, FIELD, R=40, marks=marks)
    assert all(np.isin(L.firsts[k] + np.arange(L.n), st[0]).any() for k in range(4))
    _premise(lambda f, x, lv: lu.want_centred(L, x, st, 3, 1, 2, skipna), lambda f, x, lv: centred_util.centred(x, st[0], st[1], st[2], st[3], 3, 1, 2, True, skipna),
             pick=lambda out: out[:1])          # (n counts the cells inside the grid -- and the NaNs, with skipna --, not what they hold)


def test_lifecycle():
    import life_util
    wrow, x = lu.life_wrow(L), lu.life_field_spec(L)
    assert not np.isnan(x.dense()).any() and x.background == FIELD.background
    want = lu.want_life(L, FLAG, x, wrow)
    whole = life_util.numpy_rows(FLAG.dense(), x.dense(), wrow)
    assert len(want) > 3 * L.n and want.tobytes() == whole.tobytes()
    assert np.isin(want["t"], FLAG.steps()).all() and (want["shift"] > 0).any()
    for k in (2, 3):
        less = lu.want_life(L, FLAG.without(k), x.without(k), wrow)
        assert len(less) < len(want)
    pick = want[::7]
    assert lu.want_life_exact(L, FLAG, x, wrow, pick).tobytes() == life_util.numpy_exact_rows(FLAG.dense(), x.dense(), wrow, pick, extent=True).tobytes()


@pytest.mark.parametrize("skipna", [False, True])
def test_level_mean(skipna):
    w = [0.5, 0, 1.5, 1]
    _premise(lambda f, x, lv: lu.fill_windows(L.level_steps, L.ny, L.nx, np.float32, lu.want_level(L, lv, w, skipna)),
             lambda f, x, lv: level_util.level_mean(lv.reshape(L.level_steps, L.nlev, L.ny, L.nx), w, skipna))


@pytest.mark.parametrize("mask", [False, True])
def test_reversal(mask):
    tab = L.reversal_table()
    assert (tab["eq"] >= 0).sum() >= 3
    _premise(lambda f, x, lv: lu.fill_windows(L.T, L.ny, L.nx, np.float32, lu.want_reversal(L, x, tab, mask)), lambda f, x, lv: reversal_util.from_table(x, tab, mask))
    assert lu.nonzero_words(lu.want_reversal(L, FIELD, tab, mask)) > 0


@pytest.mark.parametrize("skipna", [False, True])
def test_std_field(skipna):
    _premise(lambda f, x, lv: lu.want_std(L, x, IDS, 12, 3, 1, skipna), lambda f, x, lv: std_util.want_std(x, L.std_rows, IDS, 12, 3, 1, skipna)[0])


def test_percentile_field_and_groups():
    qs = lu.PCTL_QS
    assert qs[0] == 0.9
    _premise(lambda f, x, lv: list(lu.want_pfield(L, x, IDS, 12, 3)), lambda f, x, lv: [pfield_util.want_field(x, L.std_rows, IDS, 12, 3, q) for q in qs])
    _premise(lambda f, x, lv: list(lu.want_pgroups(L, x, IDS, 12, 3)), lambda f, x, lv: [pctl_util.want(x, L.std_rows, IDS, 12, 3, q) for q in qs])


def test_percentiles_of_the_full_layout_see_the_windows():
    """on 4200 steps the windows are few: q = 0.9 gives the background whatever they hold; the two added q give the windows' values"""
    F = lu.LAYOUT_FULL
    y0, y1 = F.std_rows
    px = np.concatenate([np.arange(max(p, y0 * F.nx), min(p + k, y1 * F.nx)) for p, k in F.patches])[::40] - y0 * F.nx     # some patch pixels of the band
    field = lu.field_spec(F)
    band = field.rows(y0, y1).reshape(F.T, 1, -1)[:, :, px]
    ids = F.ids()
    full = pfield_util.want_field(band, (0, 1), ids, 12, 3, list(lu.PCTL_QS))
    assert np.all(full[0] == field.background)
    for k in (2, 3):
        less = pfield_util.want_field(field.without(k).rows(y0, y1).reshape(F.T, 1, -1)[:, :, px], (0, 1), ids, 12, 3, list(lu.PCTL_QS))
        assert np.array_equal(less[0], full[0]) and not np.array_equal(less[1], full[1]) and not np.array_equal(less[2], full[2])
    assert np.mean(full[1] < field.background) > 0.9 and np.mean(full[2] > field.background) > 0.9
