"""the standard-deviation threshold field without a GPU: the statement of ctk_std_field_* (tests/std_util.want_std, a loop over time)
against numpy bit for bit where numpy reduces the same way (planes of two or more points) and a documented case where it does not
(a one-point plane), the launch rule ctk_std_plan against its restatement, and what the array-level entry and the class refuse before
they touch the tracker."""
import importlib

import numpy as np
import pytest

import minixr
import pctl_util
import std_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

minixr.install_as_xarray()          # only when the real package is absent


def _same(got, ref, case):
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
    first = [tuple(b) for b in bad[:4].tolist()]
    assert np.array_equal(got, ref, equal_nan=True), (case, len(bad), "at", first, "got", [got[b] for b in first], "want", [ref[b] for b in first])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", pctl_util.KINDS)
def test_statement_is_numpy_on_planes_of_two_or_more_points(kind, dtype):
    rng = np.random.default_rng(300 + pctl_util.KINDS.index(kind) * 2 + (dtype == np.float64))
    for G, W, (ny, nx), rows in ((1, 1, (3, 5), (0, 3)), (3, 2, (4, 1), (1, 3)), (12, 3, (3, 7), (1, 2)), (12, 31, (2, 2), (1, 2)), (5, 1, (3, 2), (0, 3))):
        T = max(2 * G + 5, 40)
        for rule in ("cyclic", "gaps", "shuffled"):
            group = pctl_util.groups_for(rule, T, G, rng)
            x = pctl_util.edge_slab(kind, rng, T, ny, nx, dtype, group)
            for skipna in (True, False):
                q, m, n = std_util.moments(x, rows, group, G, W, skipna)
                for ddof in (0, 1):
                    _same(std_util.finish(q, n, ddof), std_util.numpy_std(x, rows, group, G, W, ddof, skipna), (kind, dtype.__name__, G, W, rule, skipna, ddof))


def test_statement_is_numpy_on_long_pools():
    """pools of 129, 1000 and 5000 steps (numpy's pairwise blocks are 128 values long: along the first axis of a plane of two or more
    points it adds plane after plane, in time order)"""
    rng = np.random.default_rng(5)
    for n in (129, 1000, 5000):
        for dtype in (np.float32, np.float64):
            x = (1e3 + 50.0 * rng.standard_normal((n, 1, 2))).astype(dtype)
            x[rng.random(x.shape) < 0.02] = np.nan
            for skipna in (True, False):
                for ddof in (0, 1):
                    got = std_util.want_std(x, (0, 1), np.zeros(n, int), 1, 1, ddof, skipna)[0]
                    _same(got, std_util.numpy_std(x, (0, 1), np.zeros(n, int), 1, 1, ddof, skipna), (n, dtype.__name__, skipna, ddof))


def test_one_point_plane_is_not_numpy():
    """a 1 x 1 plane: numpy reduces the contiguous time axis pairwise, the statement adds in time order -- the statement is what the
    library computes (tests/test_gpu_std_field.py compares a 1 x 1 band against want_std, not numpy)"""
    rng = np.random.default_rng(6)
    differs = 0
    for n in (300, 1000, 4000):
        x = (1e3 + 50.0 * rng.standard_normal((n, 1, 1)))
        got = std_util.want_std(x, (0, 1), np.zeros(n, int), 1, 1, 0, True)[0]
        differs += int(got[0, 0, 0] != np.nanstd(x, axis=0)[0, 0])
        two = np.concatenate([x, x], axis=2)             # the same values as one of two points: numpy's bits are the statement's
        assert np.nanstd(two, axis=0)[0, 0] == got[0, 0, 0], n
    assert differs > 0


def test_nan_rule_and_empty_pools():
    x = np.array([1.0, 3.0, np.nan, 7.0]).reshape(4, 1, 1) * np.ones((1, 1, 2))
    g = np.array([0, 0, 1, 2])
    for skipna in (True, False):
        std, mean, n = std_util.want_std(x, (0, 1), g, 4, 1, 1, skipna)
        assert n[:, 0, 0].tolist() == [2, 0 if skipna else 1, 1, 0], (skipna, n[:, 0, 0])
        assert std[0, 0, 0] == np.std([1.0, 3.0], ddof=1) and np.isnan(std[1:]).all(), (skipna, std[:, 0, 0])      # n - ddof <= 0: NaN, never inf
        assert mean[0, 0, 0] == 2.0 and np.isnan(mean[1, 0, 0]) and mean[2, 0, 0] == 7.0 and np.isnan(mean[3, 0, 0])
    inf = np.array([1.0, np.inf]).reshape(2, 1, 1) * np.ones((1, 1, 2))
    assert np.isnan(std_util.want_std(inf, (0, 1), np.zeros(2, int), 1, 1, 0, True)[0]).all()     # inf - inf, as numpy


def test_plan_is_the_restated_rule():
    for name in ("ctk_std_field_f32", "ctk_std_field_f64", "ctk_debug_std_field_plan", "ctk_debug_std_field_form", "ctk_debug_time_std_field"):
        assert hasattr(_native.lib(), name) and name in _native.EXPORTS, name
    for skipna in (True, False):
        last = {tile: std_util.planes_max(tile, skipna) for tile in (32, 16, 8)}
        assert last[32] < 366 <= last[16], "366 calendar days take 16 pixels per workgroup, with counts and without"
        edges = sorted({1, 2, 12, 366} | {last[t] + d for t in last for d in (-1, 0, 1)} | {2 * last[8], 100000})
        for G in edges:
            for W in (1, 31, G, G + 5):
                got = _native.debug_std_field_plan(G, W, skipna)
                assert got == std_util.plan_py(G, W, skipna), (G, W, skipna, got)
                if W >= G:
                    assert (got["tile"], got["planes"]) == (32, 1), (G, W, skipna, got)
                else:
                    want_tile = 32 if G <= last[32] else 16 if G <= last[16] else 8 if G <= last[8] else 0
                    assert got["tile"] == want_tile and got["max_groups"] == last[8], (G, W, skipna, got)
                assert got["lds_bytes"] <= 160 * 1024
                if got["tile"]:                          # accumulators of every plane and the staged steps at 8 bytes a value
                    assert got["lds_bytes"] == got["planes"] * got["tile"] * (20 if skipna else 16) + 64 * got["tile"] * 8
    assert std_util.planes_max(8, True) == 998 and std_util.planes_max(8, False) == 1248
    for bad in ((0, 1, 1), (1, 0, 1), (-1, 1, 0)):
        with pytest.raises(ValueError):
            _native.debug_std_field_plan(*bad)


class Forbidden:
    """a tracker that fails on any call"""

    def __getattr__(self, name):
        raise AssertionError("the tracker was touched (%s)" % name)


class Recording:
    def __init__(self):
        self.calls = []

    def std_field(self, x, y0, y1, group, ngroups, window=1, ddof=0, skipna=True, want_mean=False, want_n=False):
        self.calls.append((None if x is None else x.shape, y0, y1, np.array(group), ngroups, window, ddof, skipna))
        return np.full((ngroups, y1 - y0, x.shape[2]), 2.5) * (1 + np.arange(ngroups))[:, None, None]


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
    for kw in (dict(window=0), dict(window=-3), dict(window=2.5), dict(ddof=-1), dict(ddof=0.5), dict(lat_bounds=(91, 95)), dict(lat_bounds=(100, 200))):
        for fn in (c.std_field, c.std_threshold):
            args = dict(variable="anom", k=1.5, lat_bounds=(30, 90), groupby="dayofyear", window=31)
            args.update(kw)
            with pytest.raises(ValueError):
                fn(**args)
    x, g = np.zeros((4, 3, 2), np.float32), np.zeros(4, int)
    for args, kw in (((x, (0, 4), g), {}), ((x, (2, 2), g), {}), ((x, (-1, 2), g), {}), ((x, (0, 2), g), dict(window=0)), ((x, (0, 2), g), dict(window=1.5)),
                     ((x, (0, 2), g), dict(ddof=-1)), ((x, (0, 2), g), dict(ddof=1.5)), ((x[0], (0, 2), g), {}), ((x, (0, 2), np.zeros(3, int)), {}),
                     ((x, (0, 2), np.zeros(4)), {})):
        with pytest.raises(ValueError):
            cm.std_field_numpy(*args, **kw)
    # more groups than the accumulators of 8 pixels hold: the message names the largest ngroups
    for skipna, most in ((True, 998), (False, 1248)):
        big = np.zeros((most + 1, 1, 2), np.float32)
        with pytest.raises(ValueError, match="at most %d groups" % most):
            cm.std_field_numpy(big, (0, 1), np.arange(most + 1), window=3, skipna=skipna)
    import contrack_amd
    assert contrack_amd.std_field_numpy is cm.std_field_numpy


def test_class_covers_the_grid_scales_and_blanks_outside_the_band(monkeypatch):
    rec = Recording()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: rec)
    c, a, lat, time = _class()
    out = c.std_field(variable="anom", k=-1.5, groupby="dayofyear", window=31, lat_bounds=(30, 90), ddof=1, skipna=False)
    shape, y0, y1, group, G, window, ddof, skipna = rec.calls[0]
    import pandas as pd
    doy = np.asarray(pd.DatetimeIndex(time).dayofyear)
    days = np.unique(doy)
    assert (shape, y0, y1, G, window, ddof, skipna) == (a.shape, 0, 9, len(days), 31, 1, False) and np.array_equal(days[group], doy)
    assert tuple(out.dims) == ("dayofyear", "latitude", "longitude") and np.asarray(out.data).shape == (len(days), 13, 8)
    assert np.array_equal(np.asarray(out["dayofyear"].data), days) and np.array_equal(np.asarray(out["latitude"].data), lat)
    v = np.asarray(out.data)
    assert np.array_equal(v[:, :9], -1.5 * 2.5 * (1 + np.arange(len(days)))[:, None, None] * np.ones((1, 9, 8))) and np.isnan(v[:, 9:]).all()
    assert out.attrs["k"] == -1.5 and out.attrs["ddof"] == 1 and out.attrs["window"] == 31 and out.attrs["lat_bounds"] == (30.0, 90.0)
    planes, pos = c._doy_field(out)                      # what run_contrack makes of it
    assert np.array_equal(np.asarray(planes), v, equal_nan=True) and np.array_equal(days[np.asarray(pos)], doy)
    one = c.std_field(variable="anom", k=2.0, groupby=None)
    assert rec.calls[1][1:3] == (0, 13) and rec.calls[1][4:6] == (1, 1) and not rec.calls[1][3].any()
    assert tuple(one.dims) == ("latitude", "longitude") and (np.asarray(one.data) == 5.0).all()
    thr = c.std_threshold(variable="anom", k=2.0)
    assert isinstance(thr, float) and thr == 5.0 and rec.calls[2][1:3] == (2, 6)          # 50-80N of 90, 82.5, 75, ...
    per = c.std_threshold(variable="anom", k=2.0, groupby="month", lat_bounds=(30, 90))
    assert tuple(per.dims) == ("month",) and np.array_equal(np.asarray(per.data), 5.0 * (1 + np.arange(12)))
    assert np.array_equal(np.asarray(per["month"].data), 1 + np.arange(12))
