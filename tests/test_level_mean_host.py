"""The host side of the vertical mean (README.rst:235-240 of the reference, first step of its third recipe): the weights from a level
coordinate, the launch rule against its restatement (tests/level_util.py), the argument errors the Python layer raises before it
touches the library, and the proof that the numpy oracle the GPU tests compare with can see a wrong summation order and a fused
multiply-add.  No GPU is needed."""
import itertools

import numpy as np
import pytest

import level_util as lu
from contrack_amd import _native
from contrack_amd.contrack import level_mean_numpy, level_weights


# ---- weights from a level coordinate ----------------------------------------------------------------------------------------------
def test_pinned_example_and_its_mirror():
    w = level_weights(lu.PINNED_LEVELS, (150, 500))
    assert w.dtype == np.float64 and np.array_equal(w, lu.PINNED_WEIGHTS) and w.sum() == 350.0
    assert np.array_equal(level_weights(lu.PINNED_LEVELS[::-1], (150, 500)), lu.PINNED_WEIGHTS[::-1])


def test_bounds_in_either_order_and_none():
    assert np.array_equal(level_weights(lu.PINNED_LEVELS, (500, 150)), lu.PINNED_WEIGHTS)
    w = level_weights([100.0, 200.0, 400.0], None)
    assert np.array_equal(w, [50.0, 150.0, 100.0])                       # half the distance to each neighbour
    assert np.array_equal(level_weights([100.0, 200.0, 400.0]), w)


def test_single_selected_level_gets_one():
    assert np.array_equal(level_weights(lu.PINNED_LEVELS, (440, 460)), (lu.PINNED_LEVELS == 450).astype(np.float64))
    assert np.array_equal(level_weights([500.0]), [1.0])


def test_weight_errors():
    with pytest.raises(ValueError, match="monotonic"):
        level_weights([1000, 850, 900, 500], (150, 500))
    with pytest.raises(ValueError, match="monotonic"):
        level_weights([500, 500, 400])
    with pytest.raises(ValueError, match="select no level"):
        level_weights(lu.PINNED_LEVELS, (510, 690))


# ---- the launch rule --------------------------------------------------------------------------------------------------------------
def test_level_plan_is_the_restated_rule():
    seen = set()
    for eb, nsel, npix, steps, al in itertools.product((4, 8), range(1, 18), (1, 4, 6, 585, 64, 65160, 1038240), (1, 65537, 438000), (0, 1)):
        got, want = _native.level_plan(eb, nsel, npix, steps, al), lu.plan(eb, nsel, npix, steps, al)
        assert got == want, (eb, nsel, npix, steps, al, got, want)
        seen.add((got["vec"], got["unroll"]))
    assert seen == {(v, u) for v in (0, 1) for u in (1, 2, 4, 8)}
    # steps never sit in a grid dimension that ends at 65 535; a launch stays below 2^32 work-items (2^24 - 1 workgroups of 256), the
    # kernel strides over the rest -- configs[4] of the baseline (438 000 steps of 192 x 288) is beyond that
    p = _native.level_plan(4, 8, 4, 1 << 33, 1)
    assert p["blocks"] == 1 << 33 and p["grid"] == (1 << 24) - 1 and p["grid"] * 256 < 1 << 32 and p["xcd"] == 1
    p = _native.level_plan(4, 8, 192 * 288, 438000, 1)
    assert p["bps"] == 54 and p["blocks"] == 23652000 and p["grid"] == (1 << 24) - 1
    assert _native.level_plan(4, 8, 1, (1 << 24) - 1, 1)["grid"] == (1 << 24) - 1 == _native.level_plan(4, 8, 1, 1 << 24, 1)["grid"]
    assert [_native.level_plan(4, 8, 4, s, 1)["xcd"] for s in (1, 2047, 2048)] == [0, 0, 1]
    # the forms named by the issue: 9 x 65 and odd planes are scalar in float32, 2 x 3 is vector in float64 only
    assert _native.level_plan(4, 3, 585, 7, 1)["vec"] == 0 and _native.level_plan(8, 3, 585, 7, 1)["vec"] == 0
    assert _native.level_plan(4, 3, 6, 7, 1)["vec"] == 0 and _native.level_plan(8, 3, 6, 7, 1)["vec"] == 1
    assert _native.level_plan(4, 3, 64, 7, 1)["vec"] == 1 and _native.level_plan(4, 3, 64, 7, 0)["vec"] == 0
    with pytest.raises(ValueError):
        _native.level_plan(2, 1, 1, 1, 1)


# ---- errors raised before the library is touched (no GPU here: reaching it would fail differently) -------------------------------------
def test_python_argument_errors():
    x = np.zeros((3, 4, 2, 2), dtype=np.float32)
    with pytest.raises(ValueError, match=r"\(steps, level, lat, lon\)"):
        level_mean_numpy(x[0], weights=np.ones(4))
    with pytest.raises(ValueError, match="one value per level"):
        level_mean_numpy(x, weights=np.ones(5))
    with pytest.raises(ValueError, match="finite and >= 0"):
        level_mean_numpy(x, weights=[1.0, -1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="finite and >= 0"):
        level_mean_numpy(x, weights=[1.0, np.nan, 1.0, 1.0])
    with pytest.raises(ValueError, match="all weights are zero"):
        level_mean_numpy(x, weights=np.zeros(4))
    with pytest.raises(ValueError, match="needs shape"):
        level_mean_numpy(lambda t0, nt, out: None, weights=np.ones(4))
    with pytest.raises(ValueError, match="select 3"):
        level_mean_numpy(lambda t0, nt, out: None, weights=[1.0, 0.0, 1.0, 1.0], shape=(3, 4, 2, 2), dtype=np.float32)


# ---- the oracle has teeth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["pinned", "random"])
def test_oracle_sees_order_and_contraction_in_float64(weights):
    """7 x 15 levels x 9 x 65 float64 (the GPU tests' case): summing from the top level down, or with one rounding per
    multiply-add, changes output bits, so a kernel that does either cannot pass.  The float32 cases cannot tell (the rounding to
    float32 hides it at this size): they pin indexing, conversion and NaN handling."""
    x = lu.field(np.float64)
    w = lu.PINNED_WEIGHTS if weights == "pinned" else lu.random_weights_on(lu.PINNED_WEIGHTS)
    want = lu.level_mean(x, w)
    assert want.shape == (7, 9, 65) and not np.isnan(want).any()
    assert np.allclose(want, np.tensordot(w / w.sum(), x, axes=(0, 1)), rtol=1e-12, atol=1e-12)
    falling, fused = lu.differing(want, lu.level_mean(x, w, order="falling")), lu.differing(want, lu.level_mean(x, w, fma=True))
    print("outputs of %d that differ: falling order %d, fused multiply-add %d" % (want.size, falling, fused))
    assert falling >= 1 and fused >= 1
    x32 = x.astype(np.float32)
    assert lu.level_mean(x32, w).dtype == np.float32


def test_oracle_nan_rules():
    x = lu.field(np.float32, steps=2, nlev=4, ny=2, nx=3)
    w = np.array([0.0, 2.0, 1.0, 0.0])
    x[:, 0] = np.nan                                   # an unselected level does not show
    x[0, 1, 0, 0] = np.nan
    x[1, 1:3, 1, 2] = np.nan
    a, b = lu.level_mean(x, w), lu.level_mean(x, w, skipna=True)
    assert np.isnan(a[0, 0, 0]) and np.isnan(a[1, 1, 2]) and np.count_nonzero(np.isnan(a)) == 2
    assert b[0, 0, 0] == x[0, 2, 0, 0] and np.isnan(b[1, 1, 2]) and np.count_nonzero(np.isnan(b)) == 1
    assert lu.same_bits(a, a.copy()) and not lu.same_bits(a, b)
