"""The host side of the gradient-reversal index (no GPU): the row table contrack.reversal_rows builds against its restatement in
tests/reversal_util.py and against one table written out; the launch rule ctk_reversal_plan against its restatement; the argument
errors of the Python layer; and that the numpy statement the GPU tests compare with can see a float32 subtraction and a division by
delta instead of the rows' distance."""
import numpy as np
import pytest

import reversal_util as ru
from contrack_amd import _native
from contrack_amd.contrack import reversal_limits, reversal_numpy, reversal_rows

# the 7.5 degree grid from the north pole down (row j at 90 - 7.5 j), delta = 15: two rows; active rows 2..8 (75N..30N) and 16..22
EQ_75 = [-1, -1, 4, 5, 6, 7, 8, 9, 10, -1, -1, -1, -1, -1, -1, -1, 14, 15, 16, 17, 18, 19, 20, -1, -1]
PO_75 = [-1, -1, 0, 1, 2, 3, 4, 5, 6, -1, -1, -1, -1, -1, -1, -1, 18, 19, 20, 21, 22, 23, 24, -1, -1]
EQ2_75 = [-1, -1, 6, 7, 8, 9, 10, 11, 12, -1, -1, -1, -1, -1, -1, -1, 12, 13, 14, 15, 16, 17, 18, -1, -1]


def same_rows(lat, **kw):
    got = reversal_rows(lat, **kw)
    eq, po, eq2, dE, dP, dE2 = ru.rows(lat, **kw)
    assert got["eq"].dtype == np.int32 and got["dE"].dtype == np.float64
    assert np.array_equal(got["eq"], eq) and np.array_equal(got["po"], po)
    assert np.array_equal(got["dE"], dE) and np.array_equal(got["dP"], dP)
    if kw.get("second"):
        assert np.array_equal(got["eq2"], eq2) and np.array_equal(got["dE2"], dE2)
    else:
        assert got["eq2"] is None and got["dE2"] is None
    return got


def test_pinned_table_and_its_mirror():
    lat = ru.grid(7.5)
    assert lat.shape == (25,) and lat[0] == 90 and lat[-1] == -90
    r = same_rows(lat, second=True)
    assert r["eq"].tolist() == EQ_75 and r["po"].tolist() == PO_75 and r["eq2"].tolist() == EQ2_75
    act = np.array(EQ_75) >= 0
    assert np.all(r["dE"][act] == 15) and np.all(r["dP"][act] == 15) and np.all(r["dE2"][act] == 15) and np.all(r["dE"][~act] == 0)
    m = same_rows(lat[::-1].copy(), second=True)                              # rising latitude: row j becomes 24 - j
    for key, want in (("eq", EQ_75), ("po", PO_75), ("eq2", EQ2_75)):
        assert m[key].tolist() == [24 - v if v >= 0 else -1 for v in want[::-1]], key
    two = same_rows(lat)
    assert two["eq"].tolist() == EQ_75 and two["eq2"] is None
    t = reversal_limits(r, 0.0, -10.0, -5.0)
    assert np.all(t["tS"] == 0) and np.all(t["tN"][act] == -150) and np.all(t["tS2"][act] == -75) and t["eq"] is r["eq"]
    assert reversal_limits(two)["tS2"] is None


def test_delta_that_is_no_multiple_of_the_spacing():
    lat = ru.grid(10.0)
    assert np.all(same_rows(lat, delta=15.)["eq"] == -1)                      # 5 degrees from both candidates: half the spacing is not "nearer than"
    r = same_rows(lat, delta=20.)
    assert r["eq"].tolist() == [-1, -1, 4, 5, 6, 7, 8] + [-1] * 5 + [10, 11, 12, 13, 14, -1, -1]
    r = same_rows(ru.grid(2.5), delta=14.)                                     # the nearest row: 15 degrees away, and the gradients say so
    assert np.all(r["dE"][r["eq"] >= 0] == 15.0) and np.count_nonzero(r["eq"] >= 0) == 38
    assert np.all(same_rows(lat, delta=3.)["eq"] == -1)                       # the nearest row is the row itself: no partner


def test_irregular_grid():
    lat = ru.gaussian()
    assert np.abs(np.diff(lat)).max() - np.abs(np.diff(lat)).min() > 0.01
    for second in (False, True):
        r = same_rows(lat, second=second)
        act = r["eq"] >= 0
        assert np.count_nonzero(act) >= 20
        assert np.all(np.abs(r["dE"][act] - 15) < 2) and np.all(r["dE"][act] != 15.0)
        assert np.any(r["dE"][act].astype(np.float32).astype(np.float64) != r["dE"][act])       # not representable in float32
        assert np.array_equal(r["dE"][act], np.abs(lat[act] - lat[r["eq"][act]]))


def test_hemispheres_equator_and_the_pole():
    lat = ru.grid(7.5)
    n, s, b = (same_rows(lat, hemisphere=hm) for hm in ("north", "south", "both"))
    assert np.flatnonzero(n["eq"] >= 0).tolist() == list(range(2, 9)) and np.flatnonzero(s["eq"] >= 0).tolist() == list(range(16, 23))
    assert np.array_equal(np.where(n["eq"] >= 0, n["eq"], s["eq"]), b["eq"])
    for hm in ("north", "south"):
        r = same_rows(lat, hemisphere=hm, lat_bounds=(0, 60))
        assert r["eq"][12] == -1 and np.count_nonzero(r["eq"] >= 0) == 8      # 0 is in the bounds, the equator in neither hemisphere; 60 .. 7.5 are active
    assert same_rows(lat, lat_bounds=(0, 60))["eq"][12] == 10              # 'both': the equator counts as south (s = -1), its equatorward partner is 15N
    r = same_rows(lat, lat_bounds=(30, 85))                                   # 82.5: its poleward partner would lie at 97.5
    assert r["eq"][1] == -1 and r["eq"][23] == -1 and r["eq"][2] == 4
    r = same_rows(lat, lat_bounds=(30, 75), second=True, delta=30.)          # 30N: the second equatorward partner at 30S exists; 67.5N and 75N: po beyond the pole
    assert np.flatnonzero(r["eq"] >= 0).tolist() == [4, 5, 6, 7, 8, 16, 17, 18, 19, 20]


def test_plan_equals_its_restatement():
    seen = set()
    for es in (4, 8):
        for ny, nx in ((1, 1), (2, 3), (9, 65), (181, 360), (721, 1440)):     # npix 1, 6, 585, 65 160, 1 038 240
            for steps in (1, 65537, 438000):
                for aligned in (0, 1):
                    got, want = _native.reversal_plan(es, ny, nx, steps, aligned), ru.plan(es, ny, nx, steps, aligned)
                    assert got == want, (es, ny, nx, steps, aligned)
                    assert got["grid"] * ru.THREADS < 1 << 32 and got["blocks"] == got["bps"] * steps
                    assert got["bps"] * ru.THREADS * got["vpt"] >= ny * nx
                    seen.add((got["vec"], got["xcd"], got["grid"] < got["blocks"]))
    assert {v for v, _, _ in seen} == {0, 1} and {x for _, x, _ in seen} == {0, 1} and {c for _, _, c in seen} == {False, True}
    assert _native.reversal_plan(4, 9, 65, 7, 1)["vec"] == 0 and _native.reversal_plan(4, 9, 64, 7, 1)["vec"] == 1
    assert _native.reversal_plan(4, 2, 6, 7, 1)["vec"] == 0                   # the plane is a multiple of 16 bytes, a row is not
    with pytest.raises(ValueError):
        _native.reversal_plan(2, 9, 65, 7)


def test_argument_errors_are_raised_before_the_library_is_touched(monkeypatch):
    import contrack_amd.contrack as mod

    def no_tracker(device=None):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(mod, "_tracker", no_tracker)
    lat = ru.grid(7.5)
    z = ru.field(lat, 3)
    for kw, exc in ((dict(stat="sum"), ValueError), (dict(hemisphere="east"), ValueError), (dict(delta=0.), ValueError), (dict(delta=np.nan), ValueError),
                    (dict(lat_bounds=(75, 30)), ValueError), (dict(lat_bounds=(30,)), ValueError), (dict(ghgs=np.inf), ValueError), (dict(ghgs2=np.nan), ValueError),
                    (dict(chunk_steps=-1), ValueError)):
        with pytest.raises(exc):
            reversal_numpy(z, lat, **kw)
    with pytest.raises(ValueError, match="1-D"):
        reversal_numpy(z, lat.reshape(5, 5))
    with pytest.raises(ValueError, match="rows"):
        reversal_numpy(z, lat[:-1])
    with pytest.raises(ValueError, match="steps, lat, lon"):
        reversal_numpy(z[0], lat)
    with pytest.raises(TypeError):
        reversal_numpy(z.astype(np.complex64), lat)
    with pytest.raises(ValueError, match="reader"):
        reversal_numpy(lambda t0, nt, out: None, lat)
    with pytest.raises(ValueError, match="second=True"):
        reversal_limits(reversal_rows(lat), ghgs2=-5.)
    with pytest.raises(AssertionError, match="touched"):                     # (the guard itself)
        reversal_numpy(z, lat)


@pytest.mark.parametrize("step", [7.5, 5.0, 2.5])
def test_fixture_fields_have_blocked_pixels(step):
    """the condition of every bit comparison on the GPU: between 5 % and 50 % of the active band is blocked in the statement"""
    lat = ru.grid(step)
    assert len(lat) == {7.5: 25, 5.0: 37, 2.5: 73}[step]
    for nx in (1, 3, 8, 65):
        z = ru.field(lat, nx, steps=6, seed=int(step * 10) + nx)
        for ghgs2 in (None, -5.0):
            eq = ru.table(lat, ghgs2=ghgs2)["eq"]
            for stat in ("gradient", "mask"):
                share = ru.blocked_share(ru.reversal(z, lat, ghgs2=ghgs2, stat=stat), eq)
                assert 0.05 <= share <= 0.5, (step, nx, ghgs2, stat, share)


def test_the_statement_sees_a_float32_subtraction():
    lat = ru.grid(7.5)
    z = np.exp(np.random.default_rng(3).normal(7.0, 1.0, (6, 25, 8))).astype(np.float32)      # neighbours a factor of two apart and more: z[j] - z[eq] rounds in float32
    want = ru.reversal(z, lat)
    assert 0.05 <= ru.blocked_share(want, ru.table(lat)["eq"]) <= 0.5
    assert ru.differing(want, ru.reversal(z, lat, f32_sub=True)) > 0
    zs = ru.field(lat, 8)                                                      # (the fixture field: Sterbenz, the float32 difference is exact)
    assert ru.differing(ru.reversal(zs, lat), ru.reversal(zs, lat, f32_sub=True)) == 0


def test_the_statement_sees_a_division_by_delta():
    lat = ru.gaussian()
    z = ru.field(lat, 8, dtype=np.float64)
    want = ru.reversal(z, lat)
    assert 0.05 <= ru.blocked_share(want, ru.table(lat)["eq"]) <= 0.5
    wrong = ru.reversal(z, lat, div_delta=True)
    assert np.array_equal(want != 0, wrong != 0) and ru.differing(want, wrong) == np.count_nonzero(want)
    reg = ru.grid(7.5)
    zr = ru.field(reg, 8)
    assert ru.differing(ru.reversal(zr, reg), ru.reversal(zr, reg, div_delta=True)) == 0      # (a regular grid cannot tell)
