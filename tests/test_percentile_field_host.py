"""the percentile threshold field without a GPU: the launch rule ctk_pfield_plan against its restatement, the numpy yardstick
(tests/pfield_util.py) against the one of the per-group percentile, and what the array-level entry and the class check before they
touch the tracker."""
import importlib

import numpy as np
import pytest

import minixr
import pctl_util
import pfield_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

minixr.install_as_xarray()          # only when the real package is absent


def test_plan_is_the_restated_rule():
    assert hasattr(_native.lib(), "ctk_percentile_field_f32") and hasattr(_native.lib(), "ctk_percentile_field_f64")
    for name in ("ctk_percentile_field_f32", "ctk_percentile_field_f64", "ctk_debug_percentile_field_plan", "ctk_debug_percentile_field_form",
                 "ctk_debug_time_percentile_field"):
        assert name in _native.EXPORTS, name
    for kb in (4, 8):
        cap = _native.debug_percentile_field_plan(kb, 1, 1, 1)["cap"]
        assert cap == pfield_util.plan_py(kb, 1, 1, 1)["cap"] and cap * 8 * kb <= 160 * 1024, (kb, cap)
        edges = sorted({1, 2, 40, cap // 8, cap // 4, cap // 2, cap - 1, cap, cap + 1, 2 * cap, 2 ** 31 - 1}
                       | {pfield_util.plan_py(kb, 1, 1, 1)["ring_bytes"] // (32 * kb) + d for d in (-1, 0, 1)}
                       | {pfield_util.plan_py(kb, cap // 3, 1, 1)["ring_bytes"] // (16 * kb) + d for d in (-1, 0, 1)})
        for steps in edges:
            for G, W in ((1, 1), (2, 1), (12, 3), (366, 31), (366, 366), (366, 400)):
                got = _native.debug_percentile_field_plan(kb, steps, G, W)
                assert got == pfield_util.plan_py(kb, steps, G, W), (kb, steps, G, W, got)
                assert got["form"] == (1 if steps <= cap else 0), (kb, steps, G, W)
                if got["form"] == 1:                     # the ring holds the longest pool and fits beside the selection's LDS
                    assert got["ring_bytes"] >= steps * got["tile"] * kb and got["tile"] in (8, 16, 32), (kb, steps, got)
                    assert got["ring_bytes"] + got["tile"] * (257 * 4 + 64) + 512 * 4 <= 160 * 1024, (kb, steps, got)
    for bad in ((3, 1, 1, 1), (4, -1, 1, 1), (4, 1, 0, 1), (4, 1, 1, 0)):
        with pytest.raises(ValueError):
            _native.debug_percentile_field_plan(*bad)


def test_yardstick_agrees_with_the_per_group_yardstick():
    """on a band of one pixel the field is the per-group percentile; a sequence of q gives what every q gives alone"""
    rng = np.random.default_rng(1)
    T, ny, nx, G = 60, 4, 3, 7
    for dtype in (np.float32, np.float64):
        x = (20.0 * rng.standard_normal((T, ny, nx))).astype(dtype)
        x[rng.random(x.shape) < 0.1] = np.nan
        x[:, 2, 1] = np.nan                              # an all-NaN pixel
        group = pctl_util.groups_for("gaps", T, G, rng)
        for W in (1, 2, 3, G, G + 5):
            many = pfield_util.want_field(x, (1, 4), group, G, W, pctl_util.QS)
            assert many.shape == (len(pctl_util.QS), G, 3, nx)
            for qi, q in enumerate(pctl_util.QS):
                f = pfield_util.want_field(x, (1, 4), group, G, W, q)
                assert f.shape == (G, 3, nx) and f.dtype == np.float64
                assert np.array_equal(many[qi], f, equal_nan=True), (dtype.__name__, W, q)
                for y in range(1, 4):
                    for xx in range(nx):
                        one = pctl_util.want(x[:, :, xx:xx + 1], (y, y + 1), group, G, W, q)
                        assert np.array_equal(f[:, y - 1, xx], one, equal_nan=True), (dtype.__name__, W, q, y, xx)
            assert np.isnan(many[:, :, 1, 1]).all()
    inf = np.array([1.0, np.inf]).reshape(2, 1, 1)
    assert np.isnan(pfield_util.want_field(inf, (0, 1), np.zeros(2, int), 1, 1, 1.0)[0, 0, 0])    # numpy: inf - inf


class Forbidden:
    """a tracker that fails on any call"""

    def __getattr__(self, name):
        raise AssertionError("the tracker was touched (%s)" % name)


class Recording:
    def __init__(self):
        self.calls = []

    def percentile_field(self, x, y0, y1, group, ngroups, q, window=1):
        self.calls.append((None if x is None else x.shape, y0, y1, np.array(group), ngroups, q, window))
        return np.full((ngroups, y1 - y0, x.shape[2]), 2.5)


def _class(T=400, ny=13, nx=8):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((T, ny, nx)).astype(np.float32)
    lat = np.linspace(90.0, 0.0, ny).astype(np.float32)
    lon = (np.arange(nx) * 45.0).astype(np.float32)
    time = (np.datetime64("2001-03-01") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(a, lat, lon, time=time)
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c, a, lat, time


def test_refusals_come_before_the_tracker(monkeypatch):
    monkeypatch.setattr(cm, "_tracker", lambda device=None: Forbidden())
    c, _, _, _ = _class()
    for kw in (dict(window=0), dict(window=-3), dict(window=2.5), dict(q=-0.01), dict(q=1.5), dict(q=float("nan")), dict(lat_bounds=(91, 95)),
               dict(lat_bounds=(100, 200))):
        args = dict(variable="anom", q=0.1, lat_bounds=(30, 90), groupby="dayofyear", window=31)
        args.update(kw)
        with pytest.raises(ValueError):
            c.percentile_field(**args)
    x, g = np.zeros((4, 3, 2), np.float32), np.zeros(4, int)
    for args, kw in (((x, (0, 4), g, 0.5), {}), ((x, (2, 2), g, 0.5), {}), ((x, (-1, 2), g, 0.5), {}), ((x, (0, 2), g, 0.5), dict(window=0)),
                     ((x, (0, 2), g, 0.5), dict(window=1.5)), ((x, (0, 2), g, 2.0), {}), ((x, (0, 2), g, float("nan")), {}), ((x[0], (0, 2), g, 0.5), {}),
                     ((x, (0, 2), np.zeros(3, int), 0.5), {}), ((x, (0, 2), np.zeros(4), 0.5), {})):
        with pytest.raises(ValueError):
            cm.percentile_field_numpy(*args, **kw)
    import contrack_amd
    assert contrack_amd.percentile_field_numpy is cm.percentile_field_numpy


def test_class_covers_the_grid_and_blanks_outside_the_band(monkeypatch):
    rec = Recording()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: rec)
    c, a, lat, time = _class()
    out = c.percentile_field(variable="anom", q=0.1, groupby="dayofyear", window=31, lat_bounds=(30, 90))
    shape, y0, y1, group, G, q, window = rec.calls[0]
    import pandas as pd
    doy = np.asarray(pd.DatetimeIndex(time).dayofyear)
    days = np.unique(doy)
    assert (shape, y0, y1, G, q, window) == (a.shape, 0, 9, len(days), 0.1, 31) and np.array_equal(days[group], doy)
    assert tuple(out.dims) == ("dayofyear", "latitude", "longitude") and np.asarray(out.data).shape == (len(days), 13, 8)
    assert np.array_equal(np.asarray(out["dayofyear"].data), days) and np.array_equal(np.asarray(out["latitude"].data), lat)
    v = np.asarray(out.data)
    assert (v[:, :9] == 2.5).all() and np.isnan(v[:, 9:]).all()
    assert out.attrs["q"] == 0.1 and out.attrs["window"] == 31 and out.attrs["lat_bounds"] == (30.0, 90.0)
    planes, pos = c._doy_field(out)                      # what run_contrack makes of it
    assert np.array_equal(np.asarray(planes), v, equal_nan=True) and np.array_equal(days[np.asarray(pos)], doy)
    whole = c.percentile_field(variable="anom", q=0.5, groupby="month")
    assert rec.calls[1][1:3] == (0, 13) and rec.calls[1][-1] == 1 and tuple(whole.dims) == ("month", "latitude", "longitude")
    assert not np.isnan(np.asarray(whole.data)).any()
