"""Shared by tests/test_std_field_host.py, tests/test_gpu_std_field.py and tests/test_gpu_std_class.py: the statement of
ctk_std_field_* (include/contrack_hip.h) as a loop over time -- the project's yardstick, which numpy confirms on planes of two or more
points (tests/test_std_field_host.py) -- and ctk_std_plan (contrack_amd/csrc/ctk_forms.h) restated.  The window rule is
pctl_util.window_members; the pool of a group is x[np.isin(group, members)]: IN TIME ORDER."""
import numpy as np

import pctl_util


def moments(x, rows, group, G, W, skipna):
    """(q, mean, n) of every (group, grid point) pool, each (G, rows, nx): n the values counted (uint32), mean = s / n with s summed in
    time order, q the sum of (v - mean) ** 2 in time order, product and sum rounded separately.  Vectorised over the pixels, a Python
    loop over time; groups whose member sets are identical share one accumulator."""
    y0, y1 = rows
    x = np.asarray(x)
    group = np.asarray(group)
    sets, plane_of = {}, []
    for g in range(G):
        plane_of.append(sets.setdefault(tuple(pctl_util.window_members(g, G, W)), len(sets)))
    feeds = [np.array([u for members, u in sets.items() if m in members], dtype=np.intp) for m in range(G)]     # (distinct planes per step)
    shape = (len(sets), y1 - y0, x.shape[2])
    s, q, c = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for t in range(x.shape[0]):
            v = x[t, y0:y1].astype(np.float64)
            idx = feeds[group[t]]
            if skipna:
                nan = np.isnan(v)
                c[idx] += ~nan
                s[idx] = s[idx] + np.where(nan, 0.0, v)
            else:
                c[idx] += 1
                s[idx] = s[idx] + v
        m = s / c.astype(np.float64)
        for t in range(x.shape[0]):
            v = x[t, y0:y1].astype(np.float64)
            idx = feeds[group[t]]
            d = v - m[idx]
            dd = d * d
            q[idx] = q[idx] + (np.where(np.isnan(v), 0.0, dd) if skipna else dd)
    plane_of = np.array(plane_of)
    return q[plane_of], m[plane_of], c[plane_of]


def finish(q, n, ddof):
    """std = sqrt(q / (n - ddof)) where n - ddof > 0, else NaN"""
    den = n.astype(np.int64) - int(ddof)
    with np.errstate(all="ignore"):
        return np.where(den > 0, np.sqrt(q / np.where(den > 0, den, 1).astype(np.float64)), np.nan)


def want_std(x, rows, group, G, W, ddof, skipna):
    """(std, mean, n) of ctk_std_field_*: float64, float64, uint32, each (G, rows, nx)"""
    q, m, n = moments(x, rows, group, G, W, skipna)
    return finish(q, n, ddof), m, n


def numpy_std(x, rows, group, G, W, ddof, skipna):
    """np.nanstd / np.std of every pool x[np.isin(group, members)] in float64 along time, under the statement's NaN rule: NaN where
    count - ddof <= 0 (np.nanstd's; plain np.std gives inf there when q > 0) and for an empty pool"""
    import warnings
    y0, y1 = rows
    x = np.asarray(x)
    out = np.full((G, y1 - y0, x.shape[2]), np.nan)
    for g in range(G):
        pool = np.ascontiguousarray(x[np.isin(group, pctl_util.window_members(g, G, W)), y0:y1].astype(np.float64))
        if pool.shape[0] == 0:
            continue
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            r = (np.nanstd if skipna else np.std)(pool, axis=0, ddof=ddof)
        n = (~np.isnan(pool)).sum(axis=0) if skipna else np.full(pool.shape[1:], pool.shape[0])
        out[g] = np.where(n - ddof > 0, r, np.nan)
    return out


LDS_BYTES, THREADS, STAGE = 163840, 512, 64


def planes_max(tile, skipna):
    return (LDS_BYTES - STAGE * tile * 8) // (tile * (20 if skipna else 16))


def plan_py(G, W, skipna):
    """ctk_std_plan (contrack_amd/csrc/ctk_forms.h) restated"""
    planes = 1 if W >= G else G
    for tile in (32, 16, 8):
        if planes <= planes_max(tile, skipna):
            return dict(tile=tile, planes=planes, lds_bytes=planes * tile * (20 if skipna else 16) + STAGE * tile * 8, max_groups=planes_max(8, skipna))
    return dict(tile=0, planes=planes, lds_bytes=0, max_groups=planes_max(8, skipna))
