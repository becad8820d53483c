"""Shared by the segmented streaming and time-shard tests: every golden and its expected segmented results (tests/segment_util.py:
the C oracle per segment + id offset), computed once per (golden, segmentation) and handed out read-only."""
import functools

import numpy as np

import golden_util
import segment_util as su
from contrack_amd import _native


@functools.lru_cache(maxsize=None)
def golden(name):
    g = golden_util.load(name)
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def args(g):
    return (g["thr"], _native.CMP_OPS[g["gorl"]], g["wrow"], g["overlap"], g["persistence"], g["twosided"])


@functools.lru_cache(maxsize=None)
def _expected(name, starts):
    g = golden(name)
    flag, n = su.expected(g["anom"], g["thr"], g["gorl"], g["wrow"], g["overlap"], g["persistence"], g["twosided"], list(starts))
    flag.setflags(write=False)
    return flag, n


def expected(name, starts):
    """(flag, n_tracked) of golden `name` tracked as the segments `starts`"""
    return _expected(name, tuple(int(s) for s in starts))
