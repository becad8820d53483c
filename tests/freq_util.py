"""numpy statements of the blocking frequency (README.rst:159-160 of the reference) for the frequency tests:
    np.where(flag > above, 1, 0).sum(axis=0) / T * 100       and its per-group version"""
import numpy as np


def counts(flag, ids=None, G=1, above=0):
    m = np.where(flag > above, 1, 0)
    if ids is None:
        return m.sum(axis=0)[None]
    return np.stack([m[ids == g].sum(axis=0) for g in range(G)])


def percent(flag, ids=None, G=1, above=0):
    m = np.where(flag > above, 1, 0)
    if ids is None:
        return m.sum(axis=0) / flag.shape[0] * 100
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([m[ids == g].sum(axis=0) / np.count_nonzero(ids == g) * 100 for g in range(G)])


def same_bits(a, b):
    """equal float64 arrays bit for bit (NaN included)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def groupings(T):
    """(name, ids or None, G): no grouping, t % 3, a DJF-style grouping that wraps around the year (months of 10-step blocks
    starting in November, seasons DJF / MAM / JJA / SON -> ids not sorted in time), and t % 3 spread over 5 ids (two empty groups)"""
    t = np.arange(T)
    month = (t // 10 + 10) % 12 + 1
    season = np.array([0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 0])[month - 1]
    return [("none", None, 1), ("mod3", (t % 3).astype(np.int32), 3), ("djf", season.astype(np.int32), 4),
            ("empty", ((t % 3) * 2).astype(np.int32), 5)]
