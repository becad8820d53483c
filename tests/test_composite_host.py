"""The host side of the composite over flagged time steps (include/contrack_hip.h, "composites"): the entries are declared, exported
and bound; the launch rule against its restatement (tests/composite_util.py); composite_mean; the argument errors calc_composite
raises before it touches the library; and the proof that the numpy statement the GPU tests compare with can see a reversed time
order, a float32 accumulator and a split of T.  No GPU is needed."""
import itertools
import os
import re

import numpy as np
import pytest

import composite_util as cu
import minixr
from contrack_amd import _native
from contrack_amd.contrack import composite_mean, composite_numpy, contrack

minixr.install_as_xarray()          # only when the real package is absent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT = ["ctk_composite_f32_dev", "ctk_composite_f64_dev", "ctk_composite_f32", "ctk_composite_f64", "ctk_composite_cb"]
DEBUG = ["ctk_debug_composite_plan", "ctk_debug_set_composite", "ctk_debug_composite_launch", "ctk_debug_time_composite"]


# ---- declared, exported, bound ----------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    lib = _native.lib()
    prod = open(os.path.join(ROOT, "include", "contrack_hip.h")).read()
    dbg = open(os.path.join(ROOT, "include", "contrack_hip_debug.h")).read()
    for name in PRODUCT:
        assert re.search(r"^int %s\(" % name, prod, flags=re.M), name
    for name in DEBUG:
        assert re.search(r"^int %s\(" % name, dbg, flags=re.M), name
    assert "README.rst:156-164" in prod
    for name in PRODUCT + DEBUG:
        assert name in _native.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    for name in ("composite", "composite_cb", "composite_dev", "debug_set_composite", "time_composite"):
        assert callable(getattr(_native.Tracker, name)), name
    assert callable(_native.composite_plan)
    import contrack_amd
    assert contrack_amd.composite_numpy is composite_numpy and contrack_amd.composite_mean is composite_mean
    assert callable(contrack.calc_composite)


# ---- the launch rule --------------------------------------------------------------------------------------------------------------
def test_composite_plan_is_the_restated_rule():
    seen = set()
    planes = (1, 3, 4, 64, 65, 255, 256, 257, 1037, 65160, 87381, 87382, 1038240, 1 << 33)
    for eb, npix, unroll in itertools.product((4, 8), planes, (-1, 1, 2, 3, 4, 7, 8, 16, 99)):
        got, want = _native.composite_plan(eb, npix, unroll), cu.plan(eb, npix, unroll)
        assert got == want, (eb, npix, unroll, got, want)
        seen.add(got["unroll"])
    assert seen == {1, 2, 4, 8, 16}
    # a 1-degree plane takes 16 steps per batch (about 8 MB in flight), a quarter-degree plane fills the chip by itself and takes 8;
    # the rule turns where 16 steps of the plane pass 8 MiB
    assert _native.composite_plan(4, 181 * 360) == dict(unroll=16, blocks=255, grid=255)
    assert _native.composite_plan(8, 181 * 360)["unroll"] == 8
    assert _native.composite_plan(4, 721 * 1440) == dict(unroll=8, blocks=4056, grid=4056)
    assert [_native.composite_plan(4, n)["unroll"] for n in (65536, 65537)] == [16, 8]
    # a launch stays below 2^32 work-items (2^24 - 1 workgroups of 256); the kernel strides over the rest
    p = _native.composite_plan(4, 1 << 33)
    assert p["blocks"] == 1 << 25 and p["grid"] == (1 << 24) - 1 and p["grid"] * 256 < 1 << 32
    with pytest.raises(ValueError):
        _native.composite_plan(2, 64)
    with pytest.raises(ValueError):
        _native.composite_plan(4, 0)


# ---- composite_mean ---------------------------------------------------------------------------------------------------------------
def test_composite_mean_is_sum_over_n():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((3, 4, 5)) * 1e3
    n = rng.integers(0, 7, (3, 4, 5)).astype(np.uint32)
    s[n == 0] = 0.0
    s[0, 0, 0], n[0, 0, 0] = np.inf, 2
    s[0, 0, 1], n[0, 0, 1] = np.nan, 3
    m = composite_mean(s, n)
    assert m.dtype == np.float64 and m.shape == s.shape
    assert np.array_equal(np.isnan(m), (n == 0) | np.isnan(s))
    ok = n > 0
    assert cu.same_bits(m[ok], s[ok] / n[ok].astype(np.float64))
    assert m[0, 0, 0] == np.inf


# ---- errors raised before the library is touched ----------------------------------------------------------------------------------
def _dataset(T=6, ny=4, nx=5):
    time = (np.datetime64("2000-10-20") + np.arange(T) * 40).astype("datetime64[D]").astype("datetime64[ns]")
    lat, lon = np.arange(ny, dtype=np.float64) * 2 + 40, np.arange(nx, dtype=np.float64) * 2
    ds = minixr.make_dataset(np.zeros((T, ny, nx), np.float32), lat, lon, time=time, time_units="days since 2000-10-20")
    ds["flag"] = minixr.DataArray(np.zeros((T, ny, nx), np.int32), ("time", "latitude", "longitude"), attrs={"units": "flag"})
    return ds


def test_calc_composite_argument_errors():
    ds = _dataset()
    ds["fflag"] = minixr.DataArray(np.zeros((6, 4, 5), np.float32), ("time", "latitude", "longitude"))
    ds["short"] = minixr.DataArray(np.zeros((4, 5), np.float32), ("latitude", "longitude"))
    c = contrack(ds=ds)
    with pytest.raises(ValueError, match="stat must be"):
        c.calc_composite('anom', stat='median')
    with pytest.raises(ValueError, match="not an integer field"):
        c.calc_composite('anom', flag='fflag')
    with pytest.raises(ValueError, match="they must be the same"):
        c.calc_composite('short')
    with pytest.raises(ValueError, match="must have the dimensions"):
        c.calc_composite('anom', flag='short')


def test_composite_numpy_argument_errors():
    flag, x = np.zeros((3, 2, 2), np.int32), np.zeros((3, 2, 2), np.float32)
    with pytest.raises(ValueError, match=r"\(time, lat, lon\)"):
        composite_numpy(flag[0], x[0])
    with pytest.raises(ValueError, match="integer field"):
        composite_numpy(x, x)
    with pytest.raises(ValueError, match="the field has shape"):
        composite_numpy(flag, x[:2])
    with pytest.raises(ValueError, match="a reader needs"):
        composite_numpy(lambda t0, nt, out: None, x)
    with pytest.raises(ValueError, match="a reader needs"):
        composite_numpy(flag, lambda t0, nt, out: None, shape=flag.shape)


# ---- the statement has teeth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_discriminating_inputs_discriminate(dtype):
    """one group, T = 61, plane 5 x 13, x = normal x 10**uniform(-8, 10) cast to the dtype, 30 % flagged: the statement differs from
    each of order="falling", acc="float32" and slice=8 in at least one output -- the condition under which a GPU test that passes
    on this input cannot be blind to a reversed order, a float32 accumulator or a split of T"""
    flag, x = cu.wide_case(dtype)
    assert flag.shape == (61, 5, 13) and x.dtype == dtype and 0.2 < np.mean(flag > 0) < 0.4
    want, n = cu.composite(flag, x, None, 1)
    assert want.dtype == np.float64 and n.dtype == np.uint32 and want.shape == (1, 5, 13) and not np.isnan(want).any()
    assert np.array_equal(n[0], (flag > 0).sum(axis=0)) and n.min() >= 2
    assert np.allclose(want[0], np.where(flag > 0, x.astype(np.float64), 0.0).sum(axis=0), rtol=1e-9)
    figures = {}
    for name, kw in (("falling", dict(order="falling")), ("float32", dict(acc="float32")), ("slice8", dict(slice=8))):
        other, n2 = cu.composite(flag, x, None, 1, **kw)
        assert np.array_equal(n, n2)
        figures[name] = cu.differing(want, other)
    print("outputs of %d that differ from the statement (%s): %s" % (want.size, np.dtype(dtype).name, figures))
    assert all(v >= 1 for v in figures.values()), figures
    # and the variants are the statement where they must be: a slice as long as T, rising order stated
    assert cu.same_bits(want, cu.composite(flag, x, None, 1, slice=61)[0])


def test_statement_rules():
    flag = np.array([1, 0, 2, 1, 0, 3], dtype=np.int32).reshape(6, 1, 1)
    x = np.array([1.5, np.nan, -np.inf, np.nan, np.inf, 2.0], dtype=np.float32).reshape(6, 1, 1)
    ids = np.array([0, 0, 1, 2, 1, 1])
    s, n = cu.composite(flag, x, ids, 4)
    assert s[0, 0, 0] == 1.5 and n[0, 0, 0] == 1                     # the unselected NaN at t = 1 does not show
    assert s[1, 0, 0] == -np.inf and n[1, 0, 0] == 2                 # the unselected +inf at t = 4 does not show
    assert np.isnan(s[2, 0, 0]) and n[2, 0, 0] == 1                  # a selected NaN
    assert s[3, 0, 0] == 0.0 and not np.signbit(s[3, 0, 0]) and n[3, 0, 0] == 0
    s, n = cu.composite(flag, x, ids, 4, skipna=True)
    assert s[2, 0, 0] == 0.0 and n[2, 0, 0] == 0
    s, n = cu.composite(flag, x, ids, 4, above=1)                    # a flag equal to `above` is not selected
    assert n[:, 0, 0].tolist() == [0, 2, 0, 0] and s[1, 0, 0] == -np.inf
    s, n = cu.composite(np.ones((2, 1, 1), np.int32), np.array([np.inf, -np.inf], np.float64).reshape(2, 1, 1), None, 1)
    assert np.isnan(s[0, 0, 0]) and n[0, 0, 0] == 2
    s, n = cu.composite(np.ones((2, 1, 1), np.int32), np.full((2, 1, 1), -0.0, np.float32), None, 1)
    assert s[0, 0, 0] == 0.0 and not np.signbit(s[0, 0, 0])          # +0.0 + -0.0 = +0.0
