"""Expected results of segmented tracking (ctk_set_segments) from the committed C oracle: every segment tracked alone, its ids
shifted by the number of 3-D components of the filtered mask in the segments before it (the raster numbering of the whole slab
when no connectivity crosses a break)."""
import numpy as np

import oracle


def bounds(starts, T):
    st = [int(s) for s in starts] + [int(T)]
    return list(zip(st[:-1], st[1:]))


def n3d_filtered(anom, thr, gorl, wrow, overlap, twosided):
    """3-D components of the overlap-filtered mask of one segment: the oracle with persistence=1 removes nothing more"""
    full, _ = oracle.run_contrack(anom, thr, gorl, wrow, overlap, 1, twosided)
    _, n = oracle.label((full > 0).astype(np.uint8), 1)
    return n


def expected(anom, thr, gorl, wrow, overlap, persistence, twosided, starts):
    """(flag, n_tracked) that a segmented call must return"""
    anom = np.asarray(anom, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float64)
    out = np.zeros(anom.shape, dtype=np.int32)
    off = 0
    for a, b in bounds(starts, anom.shape[0]):
        f, _ = oracle.run_contrack(anom[a:b], thr[a:b], gorl, wrow, overlap, persistence, twosided)
        out[a:b] = np.where(f > 0, f + off, 0)
        off += n3d_filtered(anom[a:b], thr[a:b], gorl, wrow, overlap, twosided)
    return out, len(np.unique(out)) - 1


def segmentations(T, seed=0):
    """named segment starts for a slab of T steps: one segment, random cuts, length-1 and length-2 segments, a break before
    every step"""
    rng = np.random.default_rng(seed + T)
    out = {"one": np.array([0])}
    if T >= 3:
        k = min(4, T - 1)
        out["random"] = np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), size=k, replace=False))])
    short = [0, 1, 3]
    if T >= 6:
        short += [T - 2, T - 1]
    out["short"] = np.array(sorted(set(s for s in short if s < T)))
    out["every"] = np.arange(T)
    return out
