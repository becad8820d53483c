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


# ---------------------------------------------------------------------------------------------------------------------------
# the plan of ctk_percentile_groups_* restated (ctk_pctl_form, ctk_pctl_refusal in contrack_amd/csrc/ctk_forms.h);
# tests/test_percentile_groups_host.py compares it with the library's own answer (ctk_debug_percentile_groups_plan)
# ---------------------------------------------------------------------------------------------------------------------------
PCTL_BITS = 11                   # widest digit
PCTL_LDS_SLOTS = 4               # histograms a sweep workgroup keeps in LDS: a day's fifth distinct prefix counts in HBM
PCTL_MAX_WINDOW = 1024
PCTL_MAX_SLOTS = 1 << 19
PCTL_CHUNK = 16384


def pctl_form(keybits, nband, G, W):
    levels = -(-keybits // PCTL_BITS)
    base, extra = divmod(keybits, levels)
    bits = [base + (1 if l < extra else 0) for l in range(levels)]
    shift = [keybits - sum(bits[:l + 1]) for l in range(levels)]
    return dict(levels=levels, sweeps=levels + 1, stride=1 if W >= G else W, chunk=PCTL_CHUNK, chunks=-(-nband // PCTL_CHUNK), shift=shift, bits=bits)


def pctl_refusal(nband, G, W, max_steps_of_a_group):
    """what the entry refuses by size, the first reason met"""
    if W < G and W > PCTL_MAX_WINDOW:
        return "window"
    if G * (1 if W >= G else W) > PCTL_MAX_SLOTS:
        return "slots"
    if -(-nband // PCTL_CHUNK) > 65535:
        return "band"
    if max_steps_of_a_group * nband > 0xffffffff:
        return "day"
    return "fine"


# ---------------------------------------------------------------------------------------------------------------------------
# a model of the selection's intermediate values, from the order statistics of the yardstick's pools
# ---------------------------------------------------------------------------------------------------------------------------
def key_of(v):
    """the order-preserving unsigned key of a float32 / float64 array: every bit flipped for a negative value, the sign bit set
    otherwise (-0.0 sorts below 0.0)"""
    v = np.ascontiguousarray(v)
    ut = {4: np.uint32, 8: np.uint64}[v.dtype.itemsize]
    u = v.view(ut)
    top = ut(1) << ut(8 * v.dtype.itemsize - 1)
    return np.where(u & top, ~u, u | top)


def day_targets(d, G, W):
    """the groups whose window holds day d"""
    return [(d - (W - 1) // 2 + j) % G for j in range(W)] if W < G else list(range(G))


def selection_model(x, rows, group, G, W, q):
    """what a radix selection on key_of must hold for every group after its last digit, from sorted pools alone:
    n[g] the pool size (NaNs dropped); key[g] the key of rank k0 = floor((n - 1) q) (0 for an empty pool, which selects nothing);
    need[g]: rank k0 + 1 exists, holds a larger key, and that key differs from key[g] above the last digit, so no histogram under
    key[g]'s prefix has counted it; nu[l][d]: the distinct level-l prefixes key >> shift[l] among the targets of day d (1 where the
    window covers every group).  nu[levels - 1] counts the distinct selected keys.  Also shift, bits, levels."""
    y0, y1 = rows
    x = np.asarray(x)
    group = np.asarray(group)
    keybits = 8 * x.dtype.itemsize
    form = pctl_form(keybits, (y1 - y0) * x.shape[2], G, W)
    per = []
    for g in range(G):
        v = x[group == g, y0:y1].ravel()
        per.append(key_of(v[~np.isnan(v)]).astype(np.uint64))
    n = np.zeros(G, np.uint64)
    key = np.zeros(G, np.uint64)
    need = np.zeros(G, np.uint32)
    last = np.uint64(form["bits"][-1])
    for g in range(G):
        pool = np.sort(np.concatenate([per[m] for m in window_members(g, G, W)]))
        n[g] = pool.size
        if not pool.size:
            continue
        k0 = int(np.floor((pool.size - 1.0) * q))
        key[g] = pool[k0]
        le = int(np.searchsorted(pool, pool[k0], side="right"))
        need[g] = le == k0 + 1 and k0 + 1 < pool.size and (pool[k0 + 1] >> last) != (pool[k0] >> last)
    nu = []
    for l in range(form["levels"]):
        pre = key >> np.uint64(form["shift"][l])
        if W >= G:
            nu.append(np.ones(G, np.uint32))
        else:
            nu.append(np.array([np.unique(pre[day_targets(d, G, W)]).size for d in range(G)], np.uint32))
    return dict(n=n, key=key, need=need, nu=nu, shift=form["shift"], bits=form["bits"], levels=form["levels"])


def odd_plane_for(nband):
    """(ny, nx), rows: a band of nband values inside a plane of an odd number of values, so that the band's first element takes
    every alignment residue over consecutive timesteps: nx the largest odd divisor of nband, a row above and one or two below"""
    nx = nband
    while nx % 2 == 0:
        nx //= 2
    nrows = nband // nx
    ny = nrows + (2 if nrows % 2 else 3)
    return (ny, nx), (1, 1 + nrows)
