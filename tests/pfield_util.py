"""Shared by tests/test_percentile_field_host.py and tests/test_gpu_percentile_field.py: the numpy yardstick of ctk_percentile_field_*
(include/contrack_hip.h).  The window rule is pctl_util.window_members."""
import warnings

import numpy as np

import pctl_util


def want_field(x, rows, group, G, W, q):
    """out[g] = np.nanquantile(pool(g).astype(np.float64), q, axis=0) over the timesteps of g's member groups, NaN where a pool is
    empty or all NaN: (G, rows, nx) -- with a sequence of q: (len(q), G, rows, nx), every q from the same pools (what numpy gives for
    each q alone, tests/test_percentile_field_host.py)"""
    y0, y1 = rows
    x = np.asarray(x)
    group = np.asarray(group)
    per = [x[group == g, y0:y1].astype(np.float64) for g in range(G)]
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    out = np.full((len(qs), G, y1 - y0, x.shape[2]), np.nan)
    done = {}
    for g in range(G):
        members = tuple(pctl_util.window_members(g, G, W))
        if members not in done:
            pool = np.concatenate([per[m] for m in members], axis=0)
            done[members] = g
            if pool.shape[0]:
                with warnings.catch_warnings(), np.errstate(invalid="ignore"):
                    warnings.simplefilter("ignore")
                    out[:, g] = np.nanquantile(pool, qs, axis=0)
        else:
            out[:, g] = out[:, done[members]]
    return out if np.ndim(q) else out[0]


def plan_py(keybytes, max_pool_steps, G, W):
    """ctk_pfield_plan (contrack_amd/csrc/ctk_forms.h) restated"""
    lds, ring_threads = 163840, 512

    def ring_steps(tile):
        return (lds - (tile * 257 * 4 + ring_threads * 4 + tile * 64)) // (tile * keybytes)
    cap = ring_steps(8)
    if max_pool_steps > cap:
        return dict(form=0, cap=cap, tile=64, ring_bytes=0)
    tile = 32
    while tile > 8 and ring_steps(tile) < max_pool_steps:
        tile //= 2
    return dict(form=1, cap=cap, tile=tile, ring_bytes=ring_steps(tile) * tile * keybytes)
