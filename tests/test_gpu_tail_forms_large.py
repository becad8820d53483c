"""The back-half forms only long slabs reach, exactly against the C oracle, with the statistics of tests/tail_forms.py asserted after
every call: k_rs_pass_blk_2pc (more k_rs_pass_blk workgroups than compute units), the 64-thread k_run_values and k_extent_blk of
shards beyond 65 536 steps, the 128-thread k_extent of wide grids beyond 2048 steps, and a streamed pass whose write launches split
at the tab_batched edge, k_relabel_v5 with two and more LDS images a chunk at each budget, and the generic k_relabel at 2^24
workgroups.  Each step's memory and time are in its docstring."""
import ctypes

import numpy as np
import pytest

import tail_forms as tf
from test_gpu_tail_forms import Calls, device_cus, inputs, _want
from contrack_amd import _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cus():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    return device_cus()


def _bars(T, ny, nx, period=7):
    """a bar that grows and shrinks over `period` steps in every plane, one more per 32 steps: ids that live several steps, ids
    that persistence removes, planes without foreground"""
    m = np.zeros((T, ny, nx), dtype=np.uint8)
    t = np.arange(T)
    length = np.minimum((t % period) * max(1, nx // (2 * period)), nx - 2)
    y = 1 + (t // 32) % (ny - 2)
    for k in range(T):
        if length[k]:
            m[k, y[k], 1:1 + length[k]] = 1
    return m


@pytest.mark.parametrize("T", [4097, 4098])
def test_two_workgroups_per_cu(T, oracle_lib, n_cus):
    """ceil((T - 1) / 16) against the CU count: k_rs_pass_blk at 4097 steps on 256 CUs, k_rs_pass_blk_2pc at 4098 (and both SEG
    builds).  4098 x 8 x 64: 8 MB, seconds."""
    anom, thr, w = inputs(_bars(T, 8, 64), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, 2)
    nb = (T - 1 + tf.PB_G - 1) // tf.PB_G
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, 2, want)
        sts = c.track_dev()
        assert all(s["fused_pass"] == 1 for s in sts)
        want_bit = tf.F_2PC if nb > n_cus else tf.F_BLK
        assert sts[0]["filter_forms"] & want_bit
        st = c.segmented(np.array([0, T // 2, T - 5]))
        assert st["filter_forms"] & (want_bit << 1)


def test_long_shard_run_values(oracle_lib, n_cus):
    """65 537 steps of 8 x 64 with few runs a plane: the 64-thread k_run_values and k_extent_blk (its last workgroup partial:
    65 537 = 4096 x 16 + 1); 65 536 steps: 256 threads.  130 MB, under a minute with the oracle."""
    for T in (65537, 65536):
        anom, thr, w = inputs(_bars(T, 8, 64), oracle_lib)
        want = _want(oracle_lib, anom, thr, w, 2)
        with _native.Tracker(0) as trk:
            c = Calls(trk, n_cus, anom, thr, w, 2, want)
            sts = c.track_dev()
            assert all(s["fused_pass"] == 1 and s["extent_form"] == tf.EXTENT_BLK for s in sts)
            assert sts[0]["runval_form"] // 10 == (64 if T > 65536 else 256)


def test_wide_extent(oracle_lib, n_cus):
    """2049 steps of 4 x 1024: the 128-thread k_extent.  33 MB, seconds."""
    anom, thr, w = inputs(_bars(2049, 4, 1024), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, 2)
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, 2, want)
        assert all(s["extent_form"] == 128 for s in c.track_dev())


def test_stream_splits_tab_batched(oracle_lib, n_cus):
    """262 144 steps of 4 x 4 streamed in blocks of 200 000: the first write launch (200 000 one-chunk workgroups) loads its
    tables in three loops, the second (62 144) in one batch.  33 MB, under a minute with the oracle."""
    T = 262144
    anom, thr, w = inputs(_bars(T, 4, 4, period=3), oracle_lib)
    want = _want(oracle_lib, anom, thr, w, 2)
    with _native.Tracker(0) as trk:
        c = Calls(trk, n_cus, anom, thr, w, 2, want)
        st = c.track_stream(200000)
        assert st["relabel_shape"] & (tf.R_BATCHED | tf.R_LOOPS) == tf.R_BATCHED | tf.R_LOOPS


def _static_plane(ny, nx):
    """diagonal three-pixel bars on the rows between the poles, background in every word, nothing at x = 0 / nx - 1"""
    y, x = np.mgrid[0:ny, 0:nx]
    m = ((x // 3 + y) % 4 == 0) & (y > 0) & (y < ny - 1) & (x > 0) & (x < nx - 1)
    return m.astype(np.uint8)


def _static_slab(trk, oracle, plane, T, xcds=()):
    """T identical planes on the device (built in blocks of at most 64 MB), tracked by track_dev: every component lives through the
    slab and every step's flags are those of the interior step of the same planes over three steps (oracle), n_tracked too.  The
    flags come back in blocks and are compared there.  xcds: the write kernel again with these chunk -> XCD remaps
    (ctk_debug_time_relabel), each compared the same way."""
    ny, nx = plane.shape
    a3, thr3, w = inputs(np.repeat(plane[None], 3, axis=0), oracle)
    want3, n3 = _want(oracle, a3, thr3, w, 2)
    assert np.array_equal(want3[0], want3[1]) and np.array_equal(want3[1], want3[2])
    ref = want3[1]
    step = ny * nx * 4
    blk = max(1, min(T, (64 << 20) // step))
    block = np.repeat(a3[:1], blk, axis=0)
    thr = oracle.prepare_thresholds(0.0, T)
    d_in, d_out = trk.malloc(T * step), trk.malloc(T * step)

    def compare():
        out = np.empty((blk, ny, nx), dtype=np.int32)
        for t0 in range(0, T, blk):
            nt = min(blk, T - t0)
            trk.d2h(out[:nt], ctypes.c_void_p(d_out.value + t0 * step))
            assert (out[:nt] == ref).all(), t0
    try:
        for t0 in range(0, T, blk):
            trk.h2d(ctypes.c_void_p(d_in.value + t0 * step), block[:min(blk, T - t0)])
        n = trk.track_dev(d_in, T, ny, nx, thr, _native.CMP_OPS[">="], w, 0.5, 2, True, d_out)
        assert n == n3
        st = trk.stats()
        compare()
        for xcd in xcds:
            trk.memset(d_out, 0xff, T * step)
            trk.time_relabel(d_out, 2, 0, xcd=xcd, reps=1)
            compare()
    finally:
        trk.free(d_in)
        trk.free(d_out)
    return st


@pytest.mark.parametrize("name", ["img2_kb20", "img2_kb24", "img2_kb28", "img3_kb20"])
def test_multi_image_write(name, oracle_lib):
    """k_relabel_v5 with chunks taller than one LDS image: two images at 20, 24 and 28 KB, three or more at 20 KB.  The rule grows the
    chunk only beyond 130 000 workgroups a launch, so these are long slabs: 65 500 x 31 x 140 (284 M pixels, 2.3 GB of device memory
    for the slab and the flags), 65 500 x 5 x 1440 (472 M, 3.8 GB), 65 500 x 5 x 1760 (576 M, 4.6 GB), 65 536 x 96 x 128 (805 M,
    6.4 GB); seconds each, most of it the block-wise copies and comparisons.  The two-image 20 KB case also writes its flags with the
    chunk -> XCD remaps 0, 1 and 16 (31 chunk rows in one chunk a step: 65 500 chunks, no multiple of 8 or 128)."""
    T, ny, nx, reach = tf.LARGE[name]
    f = tf.write_form(T, ny, nx)
    assert f["kernel"] == 5 and f["sub"] < f["rb"]
    with _native.Tracker(0) as trk:
        st = _static_slab(trk, oracle_lib, _static_plane(ny, nx), T, xcds=(0, 1, 16) if name == "img2_kb20" else ())
    assert st["relabel_kernel"] == 5 and st["relabel_shape"] == tf.relabel_shape([f])
    assert st["extent_form"] == tf.extent_form(T, nx)


def test_2p24_write_workgroups_is_beyond_the_shard_limit():
    """The generic k_relabel's third condition, 2^24 workgroups a launch or more (ctk_write_plan in ctk_forms.h), needs one chunk a step (the rows
    rule grows the chunk until the launch fits or the chunk is the plane) and so 2^24 steps: beyond the 4 000 000 steps a shard may
    hold.  The call is refused before anything is written.  2 GB of device memory, a second."""
    T, ny, nx = 1 << 24, 4, 4
    assert tf.write_form(T, ny, nx)["kernel"] == 0 and tf.write_form(tf.MAX_SHARD_T, ny, nx)["kernel"] == 5
    thr = np.zeros(T)
    w = np.ones(ny, dtype=np.float32)
    with _native.Tracker(0) as trk:
        d_in, d_out = trk.malloc(T * ny * nx * 4), trk.malloc(T * ny * nx * 4)
        try:
            with pytest.raises(ValueError, match="more than 4 000 000 timesteps"):
                trk.track_dev(d_in, T, ny, nx, thr, _native.CMP_OPS[">="], w, 0.5, 2, True, d_out)
        finally:
            trk.free(d_in)
            trk.free(d_out)
