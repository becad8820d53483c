"""The numpy restatement of calc_clim / calc_anom / the percentile threshold (oracle/anom_port.py) on hand-checkable inputs.
(It is the checker of the HIP kernels in tests/test_gpu_anom.py; parity with xarray itself is unpinned -- see its header.)"""
import numpy as np
import pytest

from oracle import anom_port


def test_centred_window_convention():
    # xarray: trailing window shifted by (-w // 2) + 1 -> [i - w // 2, i + (w - 1) // 2]
    assert anom_port.centred_window(5, 1) == (5, 5)
    assert anom_port.centred_window(5, 3) == (4, 6)
    assert anom_port.centred_window(5, 4) == (3, 6)
    a = np.arange(6, dtype=np.float64)
    r = anom_port.rolling_mean_centred(a, 3)
    assert np.isnan(r[0]) and np.isnan(r[5]) and np.allclose(r[1:5], [1, 2, 3, 4])
    r = anom_port.rolling_mean_centred(a, 2)
    assert np.isnan(r[0]) and np.allclose(r[1:], [0.5, 1.5, 2.5, 3.5, 4.5])


def test_clim_fill_and_anomaly():
    # 3 "years" of 4 groups; one grid point
    x = np.array([1, 2, 3, 4, 3, 4, 5, 6, 5, 6, 7, 8], dtype=np.float64).reshape(12, 1, 1)
    g = np.tile(np.arange(4), 3)
    raw = np.array([3, 4, 5, 6], dtype=np.float64)
    c = anom_port.calc_clim(x, g, 4, window=3)[:, 0, 0]
    # centred means exist for groups 1, 2; the ends are filled with the mean of the LAST three groups of the raw climatology
    assert np.allclose(c, [raw[1:].mean(), 4.0, 5.0, raw[1:].mean()])
    a = anom_port.calc_anom(x, g, 4, window=1, smooth=1)[:, 0, 0]
    assert np.allclose(a, x[:, 0, 0] - raw[g])
    a2 = anom_port.calc_anom(x, g, 4, window=1, smooth=2)[:, 0, 0]
    assert np.isnan(a2[0]) and np.allclose(a2[1:], (a[:-1] + a[1:]) / 2)


def test_percentile_threshold():
    x = np.arange(10, dtype=np.float64).reshape(10, 1, 1) * np.ones((1, 3, 2))
    x[:, 1, :] *= 2
    assert np.isclose(anom_port.percentile_threshold(x, (0, 2), 0.9), (8.1 + 16.2) / 2)


def _rd(v, f32):
    """the kernels' (VT) cast, back in float64"""
    return v.astype(np.float32).astype(np.float64) if f32 else v


def _kernel_loops(x, group, G, window, smooth, clim=None):
    """k_clim_raw / k_clim_roll / k_anom (contrack_amd/csrc/ctk_anom.hip) restated loop for loop, one timestep at a time and
    vectorised over the pixels only: float64 sums started at 0.0, NaNs skipped or propagated where the kernels do, the (VT) casts
    where the kernels have them.  Returns (clim in the slab's dtype, anomalies in the slab's dtype)."""
    f32 = x.dtype == np.float32
    T, P = x.shape[0], x[0].size
    xs = x.reshape(T, P).astype(np.float64)
    if clim is None:
        raw = np.empty((G, P))
        for g in range(G):
            s, c = np.zeros(P), np.zeros(P, dtype=np.int64)
            for t in range(T):                                   # tlist: the group's timesteps in time order
                if group[t] == g:
                    ok = ~np.isnan(xs[t])
                    s = np.where(ok, s + np.where(ok, xs[t], 0.0), s)
                    c += ok
            with np.errstate(invalid="ignore", divide="ignore"):
                raw[g] = _rd(np.where(c > 0, s / np.maximum(c, 1), np.nan), f32)
        fs, fc = np.zeros(P), np.zeros(P, dtype=np.int64)
        for g in range(max(0, G - window), G):
            ok = ~np.isnan(raw[g])
            fs = np.where(ok, fs + np.where(ok, raw[g], 0.0), fs)
            fc += ok
        with np.errstate(invalid="ignore", divide="ignore"):
            fill = _rd(np.where(fc > 0, fs / np.maximum(fc, 1), np.nan), f32)
        cl = np.empty((G, P))
        for g in range(G):
            lo, hi = g - window // 2, g + (window - 1) // 2
            r = fill
            if lo >= 0 and hi < G:
                s = np.zeros(P)
                for j in range(lo, hi + 1):
                    s = s + raw[j]
                m = _rd(s / window, f32)
                r = np.where(np.isnan(m), fill, m)
            cl[g] = r
    else:
        cl = np.asarray(clim, dtype=x.dtype).reshape(G, P).astype(np.float64)
    out = np.empty((T, P))
    for t in range(T):
        lo, hi = t - smooth // 2, t + (smooth - 1) // 2
        r = np.full(P, np.nan)
        if lo >= 0 and hi < T:
            s = np.zeros(P)
            for j in range(lo, hi + 1):
                with np.errstate(invalid="ignore"):
                    s = s + _rd(xs[j] - cl[group[j]], f32)
            r = _rd(s / smooth, f32)
        out[t] = r
    return cl.reshape((G,) + x.shape[1:]).astype(x.dtype), out.reshape(x.shape).astype(x.dtype)


def _slab(rng, T, shape, dtype, nans=True, infs=False, wide=False):
    if wide:                                             # seven decades, either sign: x - clim inexact in float32
        x = (rng.choice([-1.0, 1.0], (T,) + shape) * 10.0 ** rng.uniform(-3, 4, (T,) + shape)).astype(dtype)
    else:
        x = (5500.0 + 50.0 * rng.standard_normal((T,) + shape)).astype(dtype)
    if nans:
        x[rng.random(x.shape) < 0.05] = np.nan
        x[:, 0, 0] = np.nan if x[0].size > 1 else x[:, 0, 0]     # an all-NaN pixel (when there is another)
        x[T // 2] = np.nan                                       # an all-NaN timestep
    if infs:
        f = x.reshape(T, -1)
        f[1 % T, -1] = np.inf
        f[(T - 2) % T, -1] = -np.inf
        f[3 % T, 0] = np.inf
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [
    # (T, shape, G, group rule, window, smooth)
    (60, (2, 3), 12, "cyclic", 1, 1),
    (60, (2, 3), 12, "cyclic", 3, 2),
    (60, (2, 3), 12, "cyclic", 4, 5),
    (60, (1, 1), 12, "cyclic", 5, 4),                  # one pixel: numpy sums a lone column pairwise, the kernels do not
    (45, (1, 1), 1, "cyclic", 1, 7),                   # one group holding every step
    (40, (2, 2), 9, "cyclic", 31, 3),                  # window > G
    (7, (2, 2), 7, "cyclic", 2, 8),                    # smooth > T: every anomaly NaN
    (1, (2, 2), 1, "cyclic", 1, 1),                    # T = 1
    (50, (2, 3), 14, "gaps", 4, 3),                    # ids with gaps, ngroups beyond the ids used
    (50, (2, 3), 10, "shuffled", 3, 2),                # ids not monotone in time
], ids=str)
def test_port_equals_the_kernels_loops_bit_for_bit(case, dtype):
    """anom_port sums in the kernels' order: its clim and anomalies equal the kernels' loops restated step by step, bit for bit
    (the exactness of tests/test_gpu_anom_exact.py rests on this)"""
    T, shape, G, rule, window, smooth = case
    rng = np.random.default_rng(T * 100 + G + window)
    if rule == "cyclic":
        group = np.arange(T) % G
    elif rule == "gaps":
        group = np.array([(0, 2, 3, 5, 6, 8, 9, 11)[i % 8] for i in range(T)])      # 1, 4, 7, 10, 12, 13 never used
    else:
        group = rng.integers(0, G, T)
    for infs, wide in ((False, False), (True, False), (False, True)):
        x = _slab(rng, T, shape, dtype, nans=True, infs=infs, wide=wide)
        want_c, want_a = _kernel_loops(x, group, G, window, smooth)
        with np.errstate(invalid="ignore"):
            got_c = anom_port.calc_clim(x, group, G, window).astype(dtype)
            got_a = anom_port.calc_anom(x, group, G, window, smooth)
        assert got_a.dtype == dtype
        assert np.array_equal(got_c, want_c, equal_nan=True), ("clim", infs)
        assert np.array_equal(got_a, want_a, equal_nan=True), ("anom", infs)
        # a climatology handed in
        cin = (want_c.astype(np.float64) + 0.37).astype(dtype)
        _, want_a2 = _kernel_loops(x, group, G, window, smooth, clim=cin)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(anom_port.calc_anom(x, group, G, window, smooth, clim=cin), want_a2, equal_nan=True), ("clim=", infs)


def test_rolling_mean_sums_in_window_order():
    """three values whose float64 sum depends on the order: the window is summed first to last, as the kernels do"""
    a = np.array([1e16, 1.0, -1e16, 1.0])
    r = anom_port.rolling_mean_centred(a, 3)
    assert r[1] == ((0.0 + 1e16 + 1.0) + -1e16) / 3 and r[2] == ((0.0 + 1.0 + -1e16) + 1.0) / 3
