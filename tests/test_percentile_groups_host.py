"""percentile thresholds per group without a GPU: the window rule and the numpy yardstick the GPU tests compare against
(tests/pctl_util.py), the C ABI's declarations and exports, and what the class checks before it touches the tracker."""
import importlib
import os
import re

import numpy as np
import pytest

import minixr
import pctl_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

minixr.install_as_xarray()          # only when the real package is absent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_membership():
    m = pctl_util.window_members
    assert m(0, 366, 1) == [0]
    assert m(5, 12, 3) == [4, 5, 6]
    assert m(5, 12, 2) == [4, 5]                         # even: one more behind than ahead (lo = g - W // 2, hi = g + (W - 1) // 2)
    assert m(5, 12, 4) == [3, 4, 5, 6]
    assert m(0, 12, 3) == [0, 1, 11]                     # circular: the first group sees the last
    assert m(11, 12, 3) == [0, 10, 11]
    assert m(0, 366, 31) == sorted(list(range(351, 366)) + list(range(0, 16)))
    assert m(0, 12, 2) == [0, 11]
    for G in (1, 2, 3, 12):
        for W in (G, G + 1, G + 5, 3 * G + 1):
            for g in range(G):
                assert m(g, G, W) == list(range(G))      # W >= G pools every group, each once
    assert m(0, 1, 1) == [0] and m(0, 1, 31) == [0]
    for G, W in ((12, 5), (12, 6), (366, 31), (7, 2)):
        for g in range(G):
            assert len(m(g, G, W)) == W


def test_yardstick_is_the_formula():
    rng = np.random.default_rng(0)
    T, ny, nx, G = 30, 5, 4, 6
    x = rng.standard_normal((T, ny, nx)).astype(np.float32)
    x[rng.random(x.shape) < 0.1] = np.nan
    group = np.arange(T) % G
    group[group == 4] = 3                                # group 4 owns no timestep
    for W in (1, 2, 3, 6, 9):
        for q in (0.0, 0.1, 0.5, 1.0):
            got = pctl_util.want(x, (1, 4), group, G, W, q)
            for g in range(G):
                days = {(g + d) % G for d in range(-(W // 2), (W - 1) // 2 + 1)}
                pool = x[np.isin(group, list(days)), 1:4].astype(np.float64)
                ref = np.nanquantile(pool, q) if np.isfinite(pool).any() else np.nan
                assert np.array_equal(got[g], ref, equal_nan=True), (W, q, g)
    assert np.isnan(pctl_util.want(x, (1, 4), group, G, 1, 0.5)[4])              # an empty pool
    assert not np.isnan(pctl_util.want(x, (1, 4), group, G, 3, 0.5)[4])          # ... but a value from its window
    allnan = np.full((3, 2, 2), np.nan)
    assert np.isnan(pctl_util.want(allnan, (0, 2), np.zeros(3, int), 1, 1, 0.5)).all()
    inf = np.array([1.0, np.inf]).reshape(2, 1, 1)
    assert np.isnan(pctl_util.want(inf, (0, 1), np.zeros(2, int), 1, 1, 1.0)[0])    # numpy: 1 + (inf - 1) * 1 taken from the far end -> inf - inf


def test_header_declares_and_library_exports_both_entries():
    text = open(os.path.join(ROOT, "include", "contrack_hip.h")).read()
    for name in ("ctk_percentile_groups_f32", "ctk_percentile_groups_f64"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(ctk_handle \*h, const (float|double) \*x, int64_t T, int ny, int nx, int y0, int y1, "
                      r"const int32_t \*group, int ngroups, int window,\s*double q, double \*out" % name, text, re.S)
        assert m, name
        assert "README.rst:235-240" in m.group(1) and "contrack.py:648-661" in m.group(1), name
        assert name in _native.EXPORTS
        assert hasattr(_native.lib(), name)
        assert len(getattr(_native.lib(), name).argtypes) == 12
    assert "ctk_debug_percentile_groups_sweeps" in open(os.path.join(ROOT, "include", "contrack_hip_debug.h")).read()


class Forbidden:
    """a tracker that fails on any call"""

    def __getattr__(self, name):
        raise AssertionError("the tracker was touched (%s)" % name)


class Recording:
    def __init__(self):
        self.calls = []

    def percentile(self, x, y0, y1, q):
        self.calls.append(("percentile", None if x is None else x.shape, y0, y1, q))
        return 1.25

    def percentile_groups(self, x, y0, y1, group, ngroups, q, window=1):
        self.calls.append(("percentile_groups", None if x is None else x.shape, y0, y1, np.array(group), ngroups, q, window))
        return np.arange(ngroups, dtype=np.float64)


def _class(T=800, ny=13, nx=8, t0="2001-03-01"):
    rng = np.random.default_rng(4)
    a = rng.standard_normal((T, ny, nx)).astype(np.float32)
    lat = np.linspace(90.0, 0.0, ny).astype(np.float32)
    lon = (np.arange(nx) * 45.0).astype(np.float32)
    time = (np.datetime64(t0) + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(a, lat, lon, time=time)
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c, a, lat, time


def test_class_refuses_bad_arguments_before_the_tracker(monkeypatch):
    monkeypatch.setattr(cm, "_tracker", lambda device=None: Forbidden())
    c, _, _, _ = _class()
    for kw in (dict(window=0), dict(window=-3), dict(window=2.5), dict(q=-0.01), dict(q=1.5), dict(q=float("nan")), dict(lat_bounds=(91, 95)),
               dict(lat_bounds=(100, 200))):
        args = dict(variable="anom", q=0.1, lat_bounds=(30, 90), groupby="dayofyear", window=31)
        args.update(kw)
        with pytest.raises(ValueError):
            c.percentile_threshold(**args)
    with pytest.raises(ValueError):
        cm.percentile_groups_numpy(np.zeros((4, 3, 2), np.float32), (0, 4), np.zeros(4, int), 0.5)
    with pytest.raises(ValueError):
        cm.percentile_groups_numpy(np.zeros((4, 3, 2), np.float32), (0, 2), np.zeros(4, int), 0.5, window=0)
    with pytest.raises(ValueError):
        cm.percentile_groups_numpy(np.zeros((4, 3, 2), np.float32), (0, 2), np.zeros(4, int), 2.0)


def test_class_routes_groupby(monkeypatch):
    rec = Recording()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: rec)
    c, a, lat, time = _class()
    assert c.percentile_threshold(variable="anom", q=0.9, lat_bounds=(30, 90)) == 1.25           # groupby=None: the scalar path, as before
    assert rec.calls == [("percentile", a.shape, 0, 9, 0.9)]
    out = c.percentile_threshold(variable="anom", q=0.1, lat_bounds=(30, 90), groupby="dayofyear", window=31)
    kind, shape, y0, y1, group, G, q, window = rec.calls[1]
    import pandas as pd
    doy = np.asarray(pd.DatetimeIndex(time).dayofyear)
    days = np.unique(doy)
    assert (kind, shape, y0, y1, G, q, window) == ("percentile_groups", a.shape, 0, 9, len(days), 0.1, 31)
    assert np.array_equal(days[group], doy)
    assert tuple(out.dims) == ("dayofyear",) and np.array_equal(np.asarray(out["dayofyear"].data), days)
    assert np.array_equal(np.asarray(out.data), np.arange(len(days), dtype=np.float64))
    assert out.attrs["q"] == 0.1 and out.attrs["window"] == 31 and out.attrs["lat_bounds"] == (30.0, 90.0)
    # what run_contrack reads from it: the value of every step's day
    thr = c._thresholds_per_step(out, len(doy), np.float32)
    assert np.array_equal(thr, np.searchsorted(days, doy).astype(np.float64))
    out = c.percentile_threshold(variable="anom", q=0.5, lat_bounds=(30, 90), groupby="month")
    assert tuple(out.dims) == ("month",) and np.array_equal(np.asarray(out["month"].data), np.arange(1, 13)) and rec.calls[2][-1] == 1
