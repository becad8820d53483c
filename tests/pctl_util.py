"""Shared by tests/test_percentile_groups_host.py and tests/test_gpu_percentile_groups.py: the window rule and the numpy yardstick of
ctk_percentile_groups_* (include/contrack_hip.h), and the edge kinds of tests/test_gpu_anom_exact.py restated for pooled values."""
import warnings

import numpy as np

QS = [0.0, 1.0, 0.5, 0.9, 0.1, 1e-9, 1 - 1e-9]
GS = [1, 2, 3, 12, 366]


def windows_for(G):
    return sorted({1, 2, 3, 31, G, G + 5})


def window_members(g, G, W):
    """the groups pooled for group g: centred as k_clim_roll centres (lo = g - W // 2, hi = g + (W - 1) // 2), circular over G"""
    return sorted({(g + d) % G for d in range(-(W // 2), (W - 1) // 2 + 1)})


def want(x, rows, group, G, W, q):
    """out[g] = np.nanquantile(pool(g).astype(np.float64), q), NaN for an empty pool"""
    y0, y1 = rows
    x = np.asarray(x)
    group = np.asarray(group)
    per = []
    for g in range(G):
        v = x[group == g, y0:y1].astype(np.float64).ravel()
        per.append(v[~np.isnan(v)])
    out = np.full(G, np.nan)
    for g in range(G):
        pool = np.concatenate([per[m] for m in window_members(g, G, W)])
        if pool.size:
            with warnings.catch_warnings(), np.errstate(invalid="ignore"):
                warnings.simplefilter("ignore")
                out[g] = np.nanquantile(pool, q)
    return out


KINDS = ["normal_nan", "nan_groups", "duplicates", "ulp_chain_sign", "ulp_chain_one", "signed_zero", "subnormal", "one_inf", "inf_inf", "mixed_inf"]


def edge_slab(kind, rng, T, ny, nx, dtype, group):
    """(T, ny, nx) of `dtype`; group: the id of every timestep (nan_groups blanks whole groups)"""
    shape = (T, ny, nx)
    tiny = float(np.finfo(dtype).smallest_subnormal)
    if kind in ("normal_nan", "nan_groups", "mixed_inf"):
        x = (50.0 * rng.standard_normal(shape)).astype(dtype)
        x[rng.random(shape) < 0.03] = np.nan
        if kind == "nan_groups":
            x[np.asarray(group) % 3 == 1] = np.nan
        if kind == "mixed_inf":
            r = rng.random(shape)
            x[r < 0.02] = np.inf
            x[r > 0.98] = -np.inf
    elif kind == "duplicates":
        x = rng.choice(np.array([-3.5, -3.5, 0.25, 7.0, 7.0, 7.0, 1e3], dtype=dtype), shape)
    elif kind == "ulp_chain_sign":
        x = (rng.integers(-12, 13, shape) * tiny).astype(dtype)                  # ..., -2 ulp, -1 ulp, 0, 1 ulp, ... (subnormals)
    elif kind == "ulp_chain_one":
        x = (1.0 + rng.integers(-6, 7, shape) * float(np.finfo(dtype).eps)).astype(dtype)
    elif kind == "signed_zero":
        x = rng.choice(np.array([0.0, -0.0, tiny, -tiny], dtype=dtype), shape)
    elif kind == "subnormal":
        x = (rng.integers(-2 ** 20, 2 ** 20, shape) * tiny).astype(dtype)
    elif kind == "one_inf":
        x = rng.choice(np.array([1.0, np.inf], dtype=dtype), shape)
    elif kind == "inf_inf":
        x = np.full(shape, np.inf, dtype=dtype)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(x, dtype=dtype)


def poison_outside(x, rows, rng):
    """rows outside the band get values far beyond the band's on either side (and NaNs): reading one of them changes every quantile"""
    y0, y1 = rows
    out = np.array(x)
    for sl in (slice(0, y0), slice(y1, x.shape[1])):
        part = out[:, sl]
        part[...] = rng.choice(np.array([-1e30, 1e30, np.nan, -np.inf], dtype=x.dtype), part.shape)
    return out


def groups_for(rule, T, G, rng):
    if rule == "cyclic":
        return (np.arange(T) % G).astype(np.int32)
    if rule == "years":                                  # several years concatenated: ids rise, fall back, rise again
        return ((np.arange(T) + 3 * G // 4) % G).astype(np.int32)
    if rule == "gaps":                                   # every third group owns no timestep
        ids = np.array([g for g in range(G) if g % 3 != 2] or [0])
        return ids[np.arange(T) % len(ids)].astype(np.int32)
    if rule == "shuffled":
        return rng.permutation(np.arange(T) % G).astype(np.int32)
    raise KeyError(rule)
