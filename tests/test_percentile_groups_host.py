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


# ---- the library's plan (ctk_pctl_form, ctk_pctl_refusal: contrack_amd/csrc/ctk_forms.h) against its restatement in pctl_util ----------
def _plan_pair(keybits, nband, G, W, steps=1):
    got = _native.debug_percentile_groups_plan(keybits, nband, G, W, steps)
    ref = dict(pctl_util.pctl_form(keybits, nband, G, W), refusal=pctl_util.pctl_refusal(nband, G, W, steps))
    assert got == ref, (keybits, nband, G, W, steps, got, ref)
    return got


def test_plan_digits():
    p = _plan_pair(32, 1000, 12, 3)
    assert (p["levels"], p["sweeps"], p["shift"], p["bits"]) == (3, 4, [21, 10, 0], [11, 11, 10])
    p = _plan_pair(64, 1000, 12, 3)
    assert (p["levels"], p["sweeps"], p["shift"], p["bits"]) == (6, 7, [53, 42, 31, 20, 10, 0], [11, 11, 11, 11, 10, 10])
    for keybits in (16, 0, 33, 128):
        with pytest.raises(ValueError):
            _native.debug_percentile_groups_plan(keybits, 10, 1, 1)
    for bad in (dict(nband=0), dict(G=0), dict(W=0), dict(steps=-1)):
        a = dict(nband=10, G=3, W=2, steps=1)
        a.update(bad)
        with pytest.raises(ValueError):
            _native.debug_percentile_groups_plan(32, a["nband"], a["G"], a["W"], a["steps"])


def test_plan_stride_and_chunks():
    for keybits in (32, 64):
        for G in (1, 2, 12, 366):
            for W in sorted({1, max(G - 1, 1), G, G + 1}):
                p = _plan_pair(keybits, 100, G, W)
                assert p["stride"] == (W if W < G else 1), (G, W)
        want = {1: 1, 16383: 1, 16384: 1, 16385: 2, 32768: 2, 32769: 3, 65535 * 16384: 65535, 65535 * 16384 + 1: 65536}
        for nband, chunks in want.items():
            p = _plan_pair(keybits, nband, 3, 2)
            assert (p["chunk"], p["chunks"]) == (16384, chunks), nband
            assert p["refusal"] == ("band" if chunks > 65535 else "fine"), nband


def test_plan_refusals():
    plan = _plan_pair
    # a window below the group count is held in LDS, 1024 prefixes at most: 1025 is refused for the window.  1024 passes that rule, but
    # 1100 groups x 1024 slots are more histograms than a call may ask for: refused for the slots
    assert plan(32, 20, 1100, 1025)["refusal"] == "window"
    assert plan(32, 20, 1100, 1024)["refusal"] == "slots"
    assert plan(32, 20, 1100, 1100)["refusal"] == "fine" and plan(32, 20, 1100, 5000)["refusal"] == "fine"      # W >= G: one slot per day
    assert plan(32, 20, 1024, 512)["refusal"] == "fine"                           # G x W = 2^19
    assert plan(32, 20, 1024, 513)["refusal"] == "slots"                          # 2^19 + 1024
    assert plan(64, 20, 1024, 512)["refusal"] == "fine" and plan(64, 20, 1024, 513)["refusal"] == "slots"
    assert plan(32, 20, 512, 511)["refusal"] == "fine"
    # a day's uint32 counters: steps x nband <= 2^32 - 1
    assert 65537 * 65535 == 2 ** 32 - 1
    assert plan(32, 65535, 3, 2, 65537)["refusal"] == "fine"
    assert plan(32, 65536, 3, 2, 65537)["refusal"] == "day"
    assert plan(32, 65535, 3, 2, 65538)["refusal"] == "day"
    assert plan(32, 65536, 3, 2, 0)["refusal"] == "fine"                          # no group owns a timestep
    assert plan(32, 2 ** 32 - 1, 3, 2, 1)["refusal"] == "band"                    # (the band rule is met first)
    assert plan(32, 65535 * 16384, 3, 2, 4)["refusal"] == "fine" and plan(32, 65535 * 16384, 3, 2, 5)["refusal"] == "day"


def test_header_declares_the_plan_and_state_hooks():
    text = open(os.path.join(ROOT, "include", "contrack_hip_debug.h")).read()
    assert "int ctk_debug_percentile_groups_plan(int keybits, int64_t nband, int ngroups, int window, int64_t max_steps_of_a_group, int64_t *out22);" in text
    assert "int ctk_debug_percentile_groups_state(ctk_handle *h, int ngroups, uint32_t *nu_day, uint32_t *need, uint64_t *n_of);" in text
    for name in ("ctk_debug_percentile_groups_plan", "ctk_debug_percentile_groups_state"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)


# ---- the selection model on pools small enough to check by hand -----------------------------------------------------------------------
def test_keys_preserve_the_order():
    for dt, ut in ((np.float32, np.uint32), (np.float64, np.uint64)):
        tiny = np.finfo(dt).smallest_subnormal
        v = np.array([-np.inf, -3.5, -tiny, -0.0, 0.0, tiny, 1.0, 1.0 + np.finfo(dt).eps, np.inf], dtype=dt)
        k = pctl_util.key_of(v)
        assert k.dtype == ut and (np.diff(k.astype(object)) > 0).all()
        bits = 8 * v.dtype.itemsize
        assert int(k[3]) == (1 << (bits - 1)) - 1 and int(k[4]) == 1 << (bits - 1)          # -0.0 and 0.0: neighbours, flipped / sign set
        assert int(k[0]) == (~int(v[:1].view(ut)[0])) & ((1 << bits) - 1)
    assert int(pctl_util.key_of(np.array([1.0], np.float32))[0]) == 0xbf800000
    assert int(pctl_util.key_of(np.array([-1.0], np.float32))[0]) == 0x407fffff


def test_day_targets_mirror_the_window():
    for G, W in ((12, 1), (12, 2), (12, 4), (12, 5), (12, 11), (7, 3), (3, 2), (12, 12), (3, 7)):
        for d in range(G):
            assert sorted(pctl_util.day_targets(d, G, W)) == [g for g in range(G) if d in pctl_util.window_members(g, G, W)], (G, W, d)
    assert pctl_util.day_targets(0, 12, 4) == [11, 0, 1, 2] and pctl_util.window_members(0, 12, 4) == [0, 1, 10, 11]


def test_selection_model_by_hand():
    key = lambda v: int(pctl_util.key_of(np.array([v], np.float32))[0])
    # three groups of one timestep, one row of four values each; window 1
    x = np.array([[[1.0, 2.0, 3.0, np.nan]], [[5.0, 5.0, 5.0, 5.0]], [[1.0, 1.0 + 2 ** -23, 4096.0, -2.0]]], np.float32)
    group = np.arange(3)
    m = pctl_util.selection_model(x, (0, 1), group, 3, 1, 0.5)
    assert m["n"].tolist() == [3, 4, 4] and (m["levels"], m["shift"], m["bits"]) == (3, [21, 10, 0], [11, 11, 10])
    # g0: rank floor(2 * .5) = 1 -> 2.0; the next rank holds 3.0 = 0x40400000, whose upper 22 bits differ from 2.0's 0x40000000: need
    # g1: every value 5.0: le = 4 > k0 + 1: no next key is read
    # g2: sorted -2, 1, 1 + ulp, 4096: rank floor(3 * .5) = 1 -> 1.0; the next key is one ulp up, under the same upper 22 bits: no need
    assert m["key"].tolist() == [key(2.0), key(5.0), key(1.0)] and m["need"].tolist() == [1, 0, 0]
    assert [a.tolist() for a in m["nu"]] == [[1, 1, 1]] * 3                                  # W = 1: a day has one target
    m = pctl_util.selection_model(x, (0, 1), group, 3, 1, 0.75)
    # g2: rank floor(3 * .75) = 2 -> 1 + ulp, next 4096.0: need.  g0: rank floor(2 * .75) = 1
    assert m["key"].tolist() == [key(2.0), key(5.0), key(np.float32(1.0) + np.float32(2 ** -23))] and m["need"].tolist() == [1, 0, 1]
    m = pctl_util.selection_model(x, (0, 1), group, 3, 1, 1.0)
    assert m["key"].tolist() == [key(3.0), key(5.0), key(4096.0)] and m["need"].tolist() == [0, 0, 0]       # no rank k0 + 1
    # window 2 of 3 groups: g pools g - 1 and g; the targets of day d are d and d + 1
    m = pctl_util.selection_model(x, (0, 1), group, 3, 2, 0.5)
    assert m["n"].tolist() == [7, 7, 8]
    # g0 pools {-2, 1, 1+ulp, 4096} + {1, 2, 3}: sorted -2 1 1 1+ulp 2 3 4096, rank 3 -> 1 + ulp, next 2.0 (other upper bits): need
    # g1 pools {1, 2, 3} + {5 x 4}: rank 3 -> 5.0, le = 7: no.  g2 pools {5 x 4} + {-2, 1, 1+ulp, 4096}: rank floor(7 * .5) = 3 ->
    # sorted -2 1 1+ulp 5 5 5 5 4096 -> 5.0, le = 7 != 4: no
    assert m["key"].tolist() == [key(np.float32(1.0) + np.float32(2 ** -23)), key(5.0), key(5.0)] and m["need"].tolist() == [1, 0, 0]
    # days 0, 1, 2 have targets {0, 1}, {1, 2}, {2, 0}: 1+ulp and 5.0 differ in their top 11 bits already (0x3f8 / 0x40a above the sign)
    assert [a.tolist() for a in m["nu"]] == [[2, 1, 2]] * 3
    # float64, keys that part only at the last digit: 1.0 and 1.0 + 2^-52 share every prefix but the last
    x = np.array([[[1.0]], [[1.0 + 2 ** -52]]], np.float64)
    m = pctl_util.selection_model(x, (0, 1), np.arange(2), 4, 1, 0.5)
    assert m["n"].tolist() == [1, 1, 0, 0] and m["key"][2] == 0 and m["need"].tolist() == [0] * 4
    m = pctl_util.selection_model(x, (0, 1), np.arange(2), 4, 3, 0.0)
    # windows {3,0,1} {0,1,2} {1,2,3} {2,3,0}: keys 1.0, 1.0, 1+ulp, 1.0; the targets of day d are d-1, d, d+1
    k1 = int(pctl_util.key_of(np.array([1.0]))[0])
    assert m["key"].tolist() == [k1, k1, k1 + 1, k1] and m["n"].tolist() == [2, 2, 1, 1] and m["need"].tolist() == [0] * 4
    assert [a.tolist() for a in m["nu"]] == [[1, 1, 1, 1]] * 5 + [[1, 2, 2, 2]]
    assert (m["levels"], m["shift"]) == (6, [53, 42, 31, 20, 10, 0])
    # a window that covers every group: one prefix per day whatever the keys are
    m = pctl_util.selection_model(x, (0, 1), np.arange(2), 2, 2, 0.5)
    assert [a.tolist() for a in m["nu"]] == [[1, 1]] * 6 and m["n"].tolist() == [2, 2]


def test_selection_model_is_the_yardsticks_lower_value():
    """the model's selected key is the value np.nanquantile interpolates from: for q with (n - 1) q whole, the yardstick itself"""
    rng = np.random.default_rng(5)
    for dt in (np.float32, np.float64):
        x = rng.standard_normal((21, 4, 5)).astype(dt)
        x[rng.random(x.shape) < 0.1] = np.nan
        group = (np.arange(21) % 4).astype(np.int32)
        for W in (1, 2, 3, 9):
            m = pctl_util.selection_model(x, (1, 3), group, 4, W, 0.0)
            ref = pctl_util.want(x, (1, 3), group, 4, W, 0.0)
            assert np.array_equal(m["key"], pctl_util.key_of(ref.astype(dt)).astype(np.uint64)), (dt.__name__, W)
            m = pctl_util.selection_model(x, (1, 3), group, 4, W, 1.0)
            ref = pctl_util.want(x, (1, 3), group, 4, W, 1.0)
            assert np.array_equal(m["key"], pctl_util.key_of(ref.astype(dt)).astype(np.uint64)) and not m["need"].any()


def test_odd_planes_take_every_residue():
    for nband in (1, 2, 3, 4, 5, 1535, 1536, 3071, 3072, 3076, 4096, 4099, 16383, 16384, 16385, 32769, 16384 + 3077):
        (ny, nx), (y0, y1) = pctl_util.odd_plane_for(nband)
        assert (y1 - y0) * nx == nband and y0 >= 1 and y1 < ny and (ny * nx) % 2 == 1, nband
        for itemsize in (4, 8):
            per16 = 16 // itemsize
            assert {(t * ny * nx + y0 * nx) % per16 for t in range(8)} == set(range(per16)), nband
