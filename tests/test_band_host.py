"""The host side of the reductions over space per time step (no GPU): the numpy statement of tests/band_util.py -- its vectorised rules
against its naive triple loops, bit for bit --, the pure helpers lon_sector / band_total / band_fraction, the rule that picks the
kernel form, and every argument check that needs no device."""
import ctypes as C
import importlib

import numpy as np
import pytest

import band_util as bu
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")


# ---- band_util: vectorised == naive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 1, 1)])
@pytest.mark.parametrize("dtype", [None, np.float32, np.float64])
def test_vectorised_rules_equal_the_naive_loops(shape, dtype):
    T, ny, nx = shape
    for density in (0.0, 0.4, 1.0):
        flag = bu.flags(shape, density, seed=ny)
        x = None if dtype is None else bu.field(shape, dtype, seed=3)
        if x is not None and density < 1.0:
            x[flag <= 0] = np.nan                                          # unflagged values reach nothing
        for w in (bu.order_weights(ny), bu.cos_weights(ny)):
            for y0, y1 in {(0, ny), (0, 1), (ny // 2, ny)}:
                for above in (-1, 0, 500):
                    cols = bu.columns(flag, y0, y1, w, above, x)
                    bu.same(cols, bu.columns_naive(flag, y0, y1, w, above, x), (density, y0, y1, above))
                    sects = [(0, nx), (nx - 1, min(3, nx)), (nx // 2, 1), (0, min(2, nx))]
                    bu.same(bu.sectors(cols, sects), bu.sectors_naive(cols, sects), (density, y0, y1, above))
                    if above >= 0 and x is not None:
                        assert all(np.isfinite(v).all() for v in cols.values())


def test_the_order_sensitive_weights_tell_a_reordered_sum():
    ny = 5
    w = bu.order_weights(ny)
    assert list(w) == [1e16, 1.0, -1e16, 1.0, 1e16]
    flag = np.ones((1, ny, 1), np.int32)
    rising = bu.columns(flag, 0, 4, w)["area"][0, 0]
    falling = bu.columns(flag[:, ::-1], 0, 4, w[3::-1].tolist() + [0.0])["area"][0, 0]
    assert rising == 1.0 and falling == 0.0                             # ((1e16 + 1) - 1e16) + 1  against  ((1 - 1e16) + 1) + 1e16
    assert bu.band_total(w, 0, 4) == rising
    # ... and the sector sums depend on the column order in the same way
    cols = dict(cnt=np.ones((1, 4), np.uint32), area=w[None, :4].copy())
    got = bu.sectors(cols, [(0, 4), (1, 4)])["sec_area"][0]
    assert list(got) == [1.0, 0.0]                                      # columns 0 1 2 3 against 1 2 3 0


def test_band_total_of_band_util_is_the_all_flagged_case():
    ny, nx = 6, 5
    w = bu.cos_weights(ny)
    flag = np.ones((2, ny, nx), np.int32)
    sects = [(0, nx), (3, 4), (2, 1)]
    out = bu.band(flag, 1, 5, w, sects=sects)
    assert np.all(out["area"] == bu.band_total(w, 1, 5))
    assert np.array_equal(out["sec_area"][0].view(np.uint64), bu.band_total(w, 1, 5, sects, nx).view(np.uint64))


# ---- lon_sector, band_total, band_fraction ---------------------------------------------------------------------------------------------
LON360 = np.arange(0.0, 360.0, 2.5)
LON180 = np.arange(-180.0, 180.0, 2.5)


def _cols(lon, sector):
    x0, n = sector
    return [float(lon[(x0 + k) % len(lon)]) for k in range(n)]


def test_lon_sector_on_both_conventions():
    # the Euro-Atlantic sector 60W .. 30E wraps on a 0..360 grid and does not on a -180..180 grid: the same longitudes either way
    for west, east in ((-60, 30), (300, 30), (300, 390)):
        a, b = cm.lon_sector(LON360, west, east), cm.lon_sector(LON180, west, east)
        assert a == (120, 37) and b == (48, 37), (west, east, a, b)
        assert [v % 360 for v in _cols(LON360, a)] == [v % 360 for v in _cols(LON180, b)]
    # the Pacific sector 140E .. 120W wraps on the -180..180 grid
    assert cm.lon_sector(LON180, 140, -120) == (128, 41) and cm.lon_sector(LON360, 140, 240) == (56, 41)
    assert _cols(LON180, (128, 41))[0] == 140.0 and _cols(LON180, (128, 41))[-1] == -120.0
    # the full circle
    for lon in (LON360, LON180):
        for west, east in ((0, 360), (-180, 180), (10, 370)):
            assert cm.lon_sector(lon, west, east) == (0, len(lon))
    # one column
    assert cm.lon_sector(LON360, 357.5, 357.5) == (143, 1) and cm.lon_sector(LON180, -2.5, -2.5) == (71, 1)
    assert cm.lon_sector(LON360, 357.5, 359.0) == (143, 1) and cm.lon_sector(LON360, 357.5, 0) == (143, 2)
    # no column
    with pytest.raises(ValueError, match="selects no column"):
        cm.lon_sector(LON360, 0.5, 2.0)
    with pytest.raises(ValueError, match="selects no column"):
        cm.lon_sector(LON180, 1.0, 1.0)
    with pytest.raises(ValueError, match="ascending"):
        cm.lon_sector(LON360[::-1], 0, 10)


def test_band_total_and_fraction():
    w = bu.order_weights(6)
    assert cm.band_total(w, (0, 4)) == bu.band_total(w, 0, 4) == 1.0
    sects = [(0, 7), (5, 3)]
    assert np.array_equal(cm.band_total(w, (1, 6), sects), bu.band_total(w, 1, 6, sects, 7))
    wc = bu.cos_weights(9)
    assert cm.band_total(wc, (2, 7)).view(np.uint64) == bu.band_total(wc, 2, 7).view(np.uint64)
    area = np.array([[0.0, 1.0], [2.0, 4.0]])
    assert np.array_equal(cm.band_fraction(area, 4.0), area / 4.0)
    assert np.array_equal(cm.band_fraction(area, np.array([2.0, 4.0])), area / np.array([2.0, 4.0]))
    f = cm.band_fraction(np.array([0.0, 1.0]), 0.0)
    assert np.isnan(f[0]) and np.isinf(f[1])


# ---- the form rule -------------------------------------------------------------------------------------------------------------------
def test_band_plan():
    p = _native.debug_band_plan(57, 130)
    assert p == dict(form=1, rows=8, quads=33, grid=(57 * 33 + 255) // 256)
    assert _native.debug_band_plan(3, 64)["form"] == 0
    assert _native.debug_band_plan(3, 64, aligned16=False)["form"] == 1
    assert _native.debug_band_plan(3, 64, form=1)["form"] == 1
    assert _native.debug_band_plan(3, 65, form=0)["form"] == 1               # the vector form is never forced where it is not legal
    assert [_native.debug_band_plan(3, 64, rows=r)["rows"] for r in (1, 2, 3, 4, 7, 8, 15, 16, 100)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert _native.debug_band_plan(2707, 360) == dict(form=0, rows=8, quads=90, grid=(2707 * 90 + 255) // 256)


# ---- argument checks that need no device ------------------------------------------------------------------------------------------------
def test_argument_checks_without_a_device():
    flag = np.zeros((2, 4, 6), np.int32)
    w = np.ones(4)
    ok = dict(rows=(0, 4), weights=w)
    cases = [
        (dict(rows=(0, 5)), "band"), (dict(rows=(2, 2)), "band"), (dict(rows=(-1, 2)), "band"), (dict(rows=3), "rows"),
        (dict(weights=np.ones(3)), "one value per row"), (dict(weights=np.array([1.0, np.nan, 1.0, 1.0])), "finite"),
        (dict(sectors=[(6, 1)]), "sector 0"), (dict(sectors=[(0, 1), (0, 7)]), "sector 1"), (dict(sectors=[(0, 0)]), "sector 0"),
        (dict(sectors=[(0.5, 1)]), "integer pairs"), (dict(sectors=[1, 2, 3]), "integer pairs"),
        (dict(columns=False), "neither"), (dict(columns=False, sectors=[]), "neither"),
        (dict(above=2 ** 31), "int32"), (dict(chunk_steps=-1), "chunk_steps"),
        (dict(x=np.zeros((2, 4, 5), np.float32)), "shape"),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            cm.band_numpy(flag, **{**ok, **kw})
    with pytest.raises(ValueError, match="reader needs shape"):
        cm.band_numpy(lambda t0, nt, out: None, **ok)
    with pytest.raises(ValueError, match="reader needs shape"):
        cm.band_numpy(flag, x=lambda t0, nt, out: None, shape=flag.shape, **ok)
    with pytest.raises(ValueError, match="integer field"):
        cm.band_numpy(flag.astype(np.float32), **ok)
    with pytest.raises(ValueError, match="uint32 counts"):
        _native._band_args(1, 70000, 70000, (0, 1), np.ones(70000), None, True, 0)
    # the library's own first check
    L = _native.lib()
    spec, out = _native.BandSpec(), _native.BandOut()
    assert L.ctk_band_f32(None, None, None, 1, 1, 1, C.byref(spec), C.byref(out), 0) == -1
    assert b"ctk_band_f32: null handle" in L.ctk_last_error()
    assert L.ctk_band_dev(None, None, None, 4, 1, 1, 1, C.byref(spec), C.byref(out)) == -1
    assert b"ctk_band_dev: null handle" in L.ctk_last_error()
    assert L.ctk_debug_set_band(None, -1, -1) == -1
