"""The floating-point kernels of contrack_amd/csrc/ctk_anom.hip pinned bit for bit at their edges.

  k_clim_raw / k_clim_roll / k_anom  against oracle/anom_port.py, which sums in the kernels' order with the kernels' rounding points
                                     (tests/test_anom_port.py pins that against a step-by-step restatement of the loops); the
                                     library is built with -ffp-contract=off, so the device gives the same bits.
  k_quantile                         per grid point (ctk_debug_percentile_values) against np.nanquantile on float64 columns -- the
                                     port's definition (float32 slabs are widened first; numpy's own float32 arithmetic is not it).
  k_nanmean                          the band mean within the rounding bound of its summation tree, from the per-pixel values.

Every comparison is np.array_equal(..., equal_nan=True) (+0 and -0 compare equal); every assertion names its case."""
import math
import warnings

import numpy as np
import pytest

from contrack_amd import _native
from oracle import anom_port

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def _slab(rng, T, shape, dtype, edges=True, wide=False):
    """anomalies of about 50 on a field of about 5500 (the float32 sums of k_clim_roll would round differently); wide: values of
    either sign spread over seven decades, so that x and clim differ in exponent and x - clim is inexact in the dtype (the
    subtraction of two floats within a factor 2 of each other is exact, so on the narrow field the kernels' (VT) cast of it is
    invisible); with edges: 3% NaN, an all-NaN pixel, an all-NaN timestep and +-inf at a few places"""
    if wide:
        x = (rng.choice([-1.0, 1.0], (T,) + shape) * 10.0 ** rng.uniform(-3, 4, (T,) + shape)).astype(dtype)
    else:
        x = (5500.0 + 50.0 * rng.standard_normal((T,) + shape)).astype(dtype)
    if edges:
        f = x.reshape(T, -1)
        f[rng.random(f.shape) < 0.03] = np.nan
        if f.shape[1] > 1:
            f[:, f.shape[1] // 2] = np.nan
        if T > 2:
            f[T // 3] = np.nan
        f[1 % T, -1] = np.inf
        f[(T - 2) % T, -1] = -np.inf
        f[3 % T, 0] = np.inf
    return x


def _check_anom(trk, x, group, G, window, smooth, case):
    with np.errstate(invalid="ignore"):
        want_c = anom_port.calc_clim(x, group, G, window).astype(x.dtype)
        want_a = anom_port.calc_anom(x, group, G, window, smooth)
    anom, clim = trk.anomalies(x, group, G, window=window, smooth=smooth, want_clim=True)
    assert clim.dtype == x.dtype and anom.dtype == x.dtype, case
    assert np.array_equal(clim, want_c, equal_nan=True), ("clim", case, int(np.sum(~((clim == want_c) | (np.isnan(clim) & np.isnan(want_c))))))
    assert np.array_equal(anom, want_a, equal_nan=True), ("anom", case, int(np.sum(~((anom == want_a) | (np.isnan(anom) & np.isnan(want_a))))))
    # the clim= path, with a climatology that is not the slab's own
    cin = (want_c.astype(np.float64) * 1.0001 + 0.37).astype(x.dtype)
    with np.errstate(invalid="ignore"):
        want_a2 = anom_port.calc_anom(x, group, G, window, smooth, clim=cin)
    anom2, _ = trk.anomalies(x, group, G, window=window, smooth=smooth, clim=cin)
    assert np.array_equal(anom2, want_a2, equal_nan=True), ("anom from clim=", case)
    return anom


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("window", [1, 2, 3, 4, 31, 29, 30, 35], ids=lambda w: "window%d" % w)     # G = 30: G-1, G, G+5
def test_windows_and_smoothing(trk, window, dtype):
    T, G = 100, 30
    rng = np.random.default_rng(window)
    group = np.arange(T) % G
    for wide in (False, True):
        x = _slab(rng, T, (1, 257), dtype, wide=wide)
        for smooth in (1, 2, 5, T - 1, T, T + 1):
            _check_anom(trk, x, group, G, window, smooth, (dtype.__name__, "wide" if wide else "5500+-50", "window", window, "smooth", smooth))


EDGE_CASES = [
    # (name, T, shape, G, groups, window, smooth)
    ("T=1", 1, (3, 5), 1, "cyclic", 1, 1),
    ("T=1 G=3", 1, (3, 5), 3, "cyclic", 2, 1),
    ("G=1", 40, (3, 5), 1, "cyclic", 1, 3),
    ("G=1 wide window", 40, (3, 5), 1, "cyclic", 4, 2),
    ("one group holds every step", 40, (3, 5), 6, "one", 3, 2),
    ("ids with gaps", 90, (4, 7), 15, "gaps", 4, 3),
    ("ids with gaps, odd window", 90, (4, 7), 15, "gaps", 3, 4),
    ("ids not monotone in time", 90, (4, 7), 11, "shuffled", 3, 2),
    ("ids not monotone, even window", 90, (4, 7), 11, "shuffled", 6, 5),
    ("npix=1", 120, (1, 1), 12, "cyclic", 5, 4),
    ("npix=255", 60, (5, 51), 12, "cyclic", 4, 3),
    ("npix=256", 60, (16, 16), 12, "cyclic", 4, 3),
    ("npix=257", 60, (1, 257), 12, "cyclic", 4, 3),
    ("npix=195", 60, (3, 65), 12, "cyclic", 2, 2),
    ("daily, 1100 steps", 1100, (3, 65), 365, "doy", 31, 2),
]


def _groups(rule, T, G, rng):
    if rule == "cyclic":
        return np.arange(T) % G
    if rule == "one":
        return np.full(T, 2)                                               # groups 0, 1, 3, 4, 5 empty
    if rule == "gaps":
        return np.array([(0, 2, 3, 5, 6, 8, 11, 12)[i % 8] for i in range(T)])    # 1, 4, 7, 9, 10, 13, 14 never used
    if rule == "shuffled":
        return rng.permutation(np.arange(T) % G)
    return (np.arange(T) + 17) % G


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_shapes_and_groups(trk, case, dtype):
    name, T, shape, G, rule, window, smooth = case
    rng = np.random.default_rng(T * 31 + G)
    group = _groups(rule, T, G, rng)
    for edges, wide in ((False, False), (True, False), (True, True)):
        x = _slab(rng, T, shape, dtype, edges=edges, wide=wide)
        _check_anom(trk, x, group, G, window, smooth, (dtype.__name__, name, "edges" if edges else "plain", "wide" if wide else "5500+-50"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_keep_resident_slab_and_percentile_paths(trk, dtype):
    """keep_resident: the returned anomalies are the port's; percentile(None) on the resident slab gives the bits of the host path"""
    T, ny, nx, G = 400, 6, 70, 73
    rng = np.random.default_rng(11)
    x = _slab(rng, T, (ny, nx), dtype)
    group = np.arange(T) % G
    anom, _ = trk.anomalies(x, group, G, window=4, smooth=3, keep_resident=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(anom, anom_port.calc_anom(x, group, G, 4, 3), equal_nan=True), (dtype.__name__, "keep_resident")
    assert trk.resident_anom() == (T, ny, nx, dtype == np.float64)
    nband = 3 * nx
    for q in (0.9, 0.5, 0.0, 1.0):
        m_res = trk.percentile(None, 2, 5, q)
        v_res = trk.debug_percentile_values(nband)
        m_host = trk.percentile(anom, 2, 5, q)
        v_host = trk.debug_percentile_values(nband)
        assert np.array_equal(v_res, v_host, equal_nan=True), (dtype.__name__, q, "resident vs host values")
        assert np.array_equal(np.float64(m_res), np.float64(m_host), equal_nan=True), (dtype.__name__, q, "resident vs host mean")
        _check_values(v_host, anom[:, 2:5, :], q, (dtype.__name__, q, "resident"))


# ---- percentile ----------------------------------------------------------------------------------------------------------------
QS = (0.0, 1.0, 0.5, 0.9, 1e-9, 1 - 1e-9)
KINDS = ("normal", "allnan", "dups", "ulp", "zeros", "subnormal", "inf")


def _columns(kind, T, n, dtype, rng):
    """(T, n) columns of one kind"""
    if kind == "normal":
        c = 100.0 * rng.standard_normal((T, n))
        c[rng.random((T, n)) < 0.02] = np.nan
        return c.astype(dtype)
    if kind == "allnan":
        c = rng.standard_normal((T, n)).astype(dtype)
        c[:, ::2] = np.nan                                           # every other column holds no value
        return c
    if kind == "dups":
        return rng.integers(-3, 4, (T, n)).astype(dtype) * dtype(25.0)
    if kind == "ulp":
        # chains of np.nextafter: the values differ in the lowest key byte only (and around a sign change)
        it = np.int32 if dtype == np.float32 else np.int64
        base = np.array([1.0, -1.0, 5500.0, -0.0], dtype=dtype).view(it)
        b = base[rng.integers(0, 4, n)][None, :]
        c = (b + rng.integers(0, 200, (T, n)).astype(it)).view(dtype)
        return c
    if kind == "zeros":
        c = np.where(rng.random((T, n)) < 0.5, dtype(0.0), dtype(-0.0)).astype(dtype)
        c[rng.random((T, n)) < 0.1] = dtype(1.0)
        c[rng.random((T, n)) < 0.1] = dtype(-1.0)
        return c
    if kind == "subnormal":
        tiny = np.finfo(dtype).smallest_subnormal
        c = (rng.integers(-50, 51, (T, n)) * tiny).astype(dtype)
        c[rng.random((T, n)) < 0.05] = np.finfo(dtype).tiny
        return c
    if kind == "inf":
        c = rng.standard_normal((T, n)).astype(dtype)
        r = rng.random((T, n))
        c[r < 0.15] = np.inf
        c[(r >= 0.15) & (r < 0.25)] = -np.inf
        c[:, 0] = np.inf                                             # a column of +inf only (inf - inf at every q)
        c[-1, 1 % n] = np.inf                                        # [..., inf]: the lerp towards +inf
        return c
    raise ValueError(kind)


def _check_values(vals, band, q, case):
    """per-pixel values of the hook against np.nanquantile on the float64 columns"""
    cols = np.asarray(band, dtype=np.float64).reshape(band.shape[0], -1)
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                 # (all-NaN columns)
        want = np.nanquantile(cols, q, axis=0)
    bad = ~((vals == want) | (np.isnan(vals) & np.isnan(want)))
    assert not bad.any(), (case, "pixels", np.nonzero(bad)[0][:5].tolist(), vals[bad][:5].tolist(), want[bad][:5].tolist())


def _check_mean(mean, vals, case):
    """k_nanmean: 1024 threads each sum every 1024th value in order, then a pairwise tree of depth 10 -- every value passes through
    at most ceil(n / 1024) - 1 + 10 roundings, so |sum - exact| <= gamma_k * sum|v| (gamma_k = k u / (1 - k u), u = 2^-53); the
    division by the count rounds once more, and so does the reference fsum / count"""
    v = vals[~np.isnan(vals)]
    if len(v) == 0:
        assert math.isnan(mean), (case, "mean of no values")
        return
    if np.isinf(v).any():
        want = math.nan if (np.isposinf(v).any() and np.isneginf(v).any()) else float(v[np.isinf(v)][0])
        assert np.array_equal(np.float64(mean), np.float64(want), equal_nan=True), (case, "mean with inf", mean, want)
        return
    k = -(-len(vals) // 1024) - 1 + 10
    u = 2.0 ** -53
    gamma = k * u / (1 - k * u)
    want = math.fsum(v.tolist()) / len(v)
    bound = gamma * float(np.sum(np.abs(v))) / len(v) + u * (abs(mean) + abs(want))
    assert abs(mean - want) <= bound, (case, "mean", mean, want, bound)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("T", [1, 2, 3, 1000])
def test_percentile_per_pixel_values(trk, T, dtype):
    rng = np.random.default_rng(T)
    for nband in (1, 63, 64, 65, 1500):
        rows = 3 if nband == 1500 else 1                           # 1500 pixels: a band of three rows of 500
        nx = nband // rows
        for kind in KINDS:
            x = np.full((T, rows + 2, nx), np.nan, dtype=dtype)      # rows outside the band: NaN, must not count
            x[:, 1:rows + 1, :] = _columns(kind, T, nband, dtype, rng).reshape(T, rows, nx)
            x[:, 0, :] = dtype(7.0)
            for q in QS:
                case = (dtype.__name__, "T", T, "nband", nband, kind, "q", q)
                mean = trk.percentile(x, 1, rows + 1, q)
                vals = trk.debug_percentile_values(nband)
                _check_values(vals, x[:, 1:rows + 1, :], q, case)
                _check_mean(mean, vals, case)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_percentile_inf_neighbours(trk, dtype):
    """the lerp at t = 0 and towards / between infinities is numpy's: [1, inf] at q = 0 is NaN (1 + inf * 0), q = 1 on [1, inf] is
    NaN (inf - inf), [inf, inf] is NaN at every q, [-inf, 1] at q = 0 is NaN"""
    cols = np.array([[1.0, 1.0, np.inf, -np.inf, 1.0, 2.0],
                     [np.inf, np.inf, np.inf, 1.0, 2.0, np.nan]], dtype=dtype)
    x = cols[:, None, :]
    for q in (0.0, 1.0, 0.5, 0.25):
        trk.percentile(x, 0, 1, q)
        _check_values(trk.debug_percentile_values(cols.shape[1]), x, q, (dtype.__name__, "inf neighbours", "q", q))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("T", [1, 5, 259])                          # 259: no multiple of the 4 lanes per pixel, more than the 256 bins
def test_scalar_and_field_entries_are_one_selection(trk, T, dtype):
    """k_quantile and k_pfield_direct / k_pfield_ring run the same pf_select: one group holding every step with window 1 is the
    scalar entry's pool, and the per-pixel values agree in every bit.  65 pixels: two workgroups, the second with one pixel."""
    rng = np.random.default_rng(1000 + T)
    for kind in ("normal", "allnan"):
        x = np.full((T, 3, 65), np.nan, dtype=dtype)
        x[:, 1, :] = _columns(kind, T, 65, dtype, rng)
        x[:, 0, :] = dtype(7.0)
        for q in QS:
            trk.percentile(x, 1, 2, q)
            vals = trk.debug_percentile_values(65)
            field = trk.percentile_field(x, 1, 2, np.zeros(T, dtype=np.int32), 1, q, window=1)[0].ravel()
            assert np.array_equal(np.isnan(vals), np.isnan(field)), (dtype.__name__, "T", T, kind, "q", q, "NaN positions")
            assert np.array_equal(vals.view(np.uint64)[~np.isnan(vals)], field.view(np.uint64)[~np.isnan(field)]), (dtype.__name__, "T", T, kind, "q", q)


def test_scalar_entry_refuses_2p31_steps(trk):
    """the selection counts its pool in an int: T = 2^31 is refused before the slab is touched (the buffer holds one value)"""
    x = np.zeros(1, dtype=np.float32)
    out = _native.C.c_double(0.0)
    with pytest.raises(ValueError, match="at most 2\\^31 - 1"):
        _native.check(_native.lib().ctk_percentile_f32(trk.handle, x.ctypes.data, 2 ** 31, 1, 1, 0, 1, 0.5, _native.C.byref(out)))
    assert trk.percentile(x.reshape(1, 1, 1), 0, 1, 0.5) == 0.0      # the handle goes on working


# ---- long and large slabs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [3000, 70000], ids=["G3000", "G70000"])
def test_long_slab_beyond_grid_y_limit(trk, G):
    """T = 2.2e6 steps on a 1 x 2 grid: k_anom launches 68 750 workgroups in grid y (segments of 32 steps), and with 70 000 groups
    k_clim_raw launches 70 000 -- beyond the 65 535 that ctk_freq.hip grid-strides for.  Pins that these launches run and are exact."""
    T = 2_200_000
    rng = np.random.default_rng(G)
    x = _slab(rng, T, (1, 2), np.float32)
    group = np.arange(T) % G
    _check_anom(trk, x, group, G, 5, 3, ("T", T, "G", G))


def _mem_available():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def test_slab_beyond_2p32_elements(trk):
    """66 000 x 181 x 360 float32 = 4.30e9 elements (17.2 GB each way): sampled pixel columns -- those holding flat indices 2^31,
    2^32 and the last element among them -- against the port evaluated on those columns only (every step of the three kernels is
    independent per pixel)"""
    T, ny, nx = 66000, 181, 360
    npix = ny * nx
    n = T * npix
    assert n > 2 ** 32
    need = 2 * n * 4 + (4 << 30)
    avail = _mem_available()
    if avail is not None and avail < need:
        pytest.fail("the 2^32-element slab needs %.1f GB of host memory, %.1f GB are available" % (need / 2 ** 30, avail / 2 ** 30))
    rng = np.random.default_rng(32)
    B = 97                                                           # 97 random planes, offset per step: a slab without a short period
    block = (50.0 * rng.standard_normal((B, ny, nx))).astype(np.float32)
    off = (5500.0 + 30.0 * np.sin(np.arange(T) * 2 * np.pi / 365.0) + rng.standard_normal(T)).astype(np.float32)
    try:
        x = np.empty((T, ny, nx), dtype=np.float32)
    except MemoryError as e:
        pytest.fail("the 2^32-element slab needs 2 x 17.2 GB of host memory: %s" % e)
    for t0 in range(0, T, B):
        t1 = min(T, t0 + B)
        np.add(block[:t1 - t0], off[t0:t1, None, None], out=x[t0:t1])
    x.reshape(T, -1)[rng.random(T) < 0.002, 7] = np.nan
    group = np.arange(T) % 365
    try:
        anom, clim = trk.anomalies(x, group, 365, window=31, smooth=2, want_clim=True)
    except (MemoryError, _native.ContrackHipError) as e:
        pytest.fail("the 2^32-element slab needs 2 x 17.2 GB of device and host memory: %s" % e)
    pix = sorted({0, 7, (2 ** 31) % npix, (2 ** 32) % npix, (2 ** 32 - 1) % npix, (n - 1) % npix} | set(rng.integers(0, npix, 10).tolist()))
    cols = x.reshape(T, npix)[:, pix].reshape(T, 1, len(pix))
    want_c = anom_port.calc_clim(cols, group, 365, 31).astype(np.float32)
    want_a = anom_port.calc_anom(cols, group, 365, 31, 2)
    got_c = clim.reshape(365, npix)[:, pix].reshape(365, 1, len(pix))
    got_a = anom.reshape(T, npix)[:, pix].reshape(T, 1, len(pix))
    assert np.array_equal(got_c, want_c, equal_nan=True), "clim of the sampled pixels"
    for i, p in enumerate(pix):
        assert np.array_equal(got_a[:, 0, i], want_a[:, 0, i], equal_nan=True), ("anomalies of pixel", p)
