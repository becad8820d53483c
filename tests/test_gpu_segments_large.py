"""Segment breaks at full size, no oracle needed: identical members must get identical ids up to a per-member shift, and a
segmented call must equal per-segment calls on the same device buffer up to per-segment shifts."""
import ctypes as C

import numpy as np
import pytest

from contrack_amd import _native, synth
from contrack_amd.contrack import row_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def shift_of(seg, alone):
    """the constant seg - alone over the foreground (the masks must agree)"""
    fg = alone > 0
    assert np.array_equal(seg > 0, fg)
    if not fg.any():
        return None
    d = np.unique(seg[fg].astype(np.int64) - alone[fg])
    assert d.size == 1, "ids are not a constant shift: {}".format(d[:5])
    return int(d[0])


def test_identical_members(trk):
    M, T, ny, nx = 40, 200, 181, 360
    lat, _ = synth.grid(ny, nx)
    w = row_weights(lat, np.float32(1.0), np.float32(1.0))
    plane = ny * nx
    d_in = trk.malloc(M * T * plane * 4)
    d_out = trk.malloc(M * T * plane * 4)
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=3)
        one = np.empty((T, ny, nx), dtype=np.float32)
        trk.d2h(one, d_in)
        for m in range(1, M):
            trk.h2d(C.c_void_p(d_in.value + m * T * plane * 4), one)
        thr = np.full(M * T, np.float64(np.float32(160.0)))
        trk.set_segments(np.arange(M) * T)
        try:
            n = trk.track_dev(d_in, M * T, ny, nx, thr, 0, w, 0.5, 5, True, d_out)
        finally:
            trk.clear_segments()
        flag = np.empty((M, T, ny, nx), dtype=np.int32)
        trk.d2h(flag, d_out)
        n0 = trk.track_dev(d_in, T, ny, nx, thr[:T], 0, w, 0.5, 5, True, d_out)
        alone = np.empty((T, ny, nx), dtype=np.int32)
        trk.d2h(alone, d_out)
    finally:
        trk.free(d_in)
        trk.free(d_out)
    assert np.array_equal(flag[0], alone) and n0 > 0
    n3d = shift_of(flag[1], alone)
    assert n3d is not None and n3d >= alone.max()
    for m in range(2, M):
        assert shift_of(flag[m], alone) == m * n3d
    assert n == len(np.unique(flag)) - 1 == M * n0


def test_winters_match_per_segment_calls(trk):
    T, ny, nx = 2707, 181, 360
    starts = np.array([0] + [int(round(k * T / 30)) for k in range(1, 30)])
    lat, _ = synth.grid(ny, nx)
    w = row_weights(lat, np.float32(1.0), np.float32(1.0))
    plane = ny * nx
    thr = np.full(T, np.float64(np.float32(160.0)))
    d_in = trk.malloc(T * plane * 4)
    d_out = trk.malloc(T * plane * 4)
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        trk.set_segments(starts)
        try:
            n = trk.track_dev(d_in, T, ny, nx, thr, 0, w, 0.5, 5, True, d_out)
        finally:
            trk.clear_segments()
        seg = np.empty((T, ny, nx), dtype=np.int32)
        trk.d2h(seg, d_out)
        bounds = list(zip(starts, list(starts[1:]) + [T]))
        for a, b in bounds:
            trk.track_dev(C.c_void_p(d_in.value + int(a) * plane * 4), int(b - a), ny, nx, thr[a:b], 0, w, 0.5, 5, True,
                          C.c_void_p(d_out.value + int(a) * plane * 4))
        alone = np.empty((T, ny, nx), dtype=np.int32)
        trk.d2h(alone, d_out)
    finally:
        trk.free(d_in)
        trk.free(d_out)
    top = 0
    for a, b in bounds:
        s = shift_of(seg[a:b], alone[a:b])
        if s is None:
            continue
        assert s >= top, "segment [{}, {}) overlaps the ids of the segments before it".format(a, b)
        top = s + int(alone[a:b].max())
    assert n == len(np.unique(seg)) - 1
