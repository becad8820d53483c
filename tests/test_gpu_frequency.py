"""The blocking frequency on the device (ctk_frequency*, k_freq): counts exactly, percent bit for bit against the numpy statement of
README.rst:159-160 of the reference (np.where(flag > above, 1, 0).sum(axis=0) / T * 100, per group)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import freq_util
import golden_util
from contrack_amd import _native, synth

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def _on_device(trk, flag, offset=0):
    """flag copied into a fresh device buffer, `offset` bytes into it; returns (allocation, pointer to the flag)"""
    flag = np.ascontiguousarray(flag, dtype=np.int32)
    base = trk.malloc(flag.nbytes + offset + 16)
    ptr = C.c_void_p(base.value + offset)
    trk.h2d(ptr, flag)
    return base, ptr


def _check(flag, ids, G, above, got_counts, tag):
    want = freq_util.counts(flag, ids, G, above)
    assert got_counts.dtype == np.uint32 and got_counts.shape == want.shape, tag
    assert np.array_equal(got_counts.astype(np.int64), want), tag


@pytest.mark.parametrize("name", golden_util.case_names())
def test_golden_flags_every_grouping_and_threshold(trk, name):
    flag = golden_util.load(name)["flag"]
    T = flag.shape[0]
    aboves = (-1, 0, 1, int(flag.max()) + 1)
    for gname, ids, G in freq_util.groupings(T):
        for above in aboves:
            _check(flag, ids, G, above, trk.frequency(flag, ids, G, above), (name, gname, above))
            Gn = 1 if ids is None else int(ids.max()) + 1                 # (frequency_numpy: G = the largest id + 1)
            got = cm.frequency_numpy(flag, ids, above=above)
            assert freq_util.same_bits(got, freq_util.percent(flag, ids, Gn, above)), (name, gname, above)
            cnt = cm.frequency_numpy(flag, ids, above=above, percent=False)
            want = freq_util.counts(flag, ids, Gn, above)
            assert cnt.dtype == np.int64 and np.array_equal(cnt, want[0] if ids is None else want)


def test_readme_expression(trk):
    """above=1: xr.where(block['flag'] > 1, 1, 0).sum(dim='time') / block.ntime * 100, as a (ny, nx) float64 array"""
    flag = golden_util.load("syn2deg_s0")["flag"]
    got = cm.frequency_numpy(flag, above=1)
    assert got.shape == flag.shape[1:] and got.dtype == np.float64
    assert freq_util.same_bits(got, np.where(flag > 1, 1, 0).sum(axis=0) / flag.shape[0] * 100)


def _random_flag(T, ny, nx, seed, density=0.05):
    rng = np.random.default_rng(seed)
    return ((rng.random((T, ny, nx)) < density) * rng.integers(1, 1000, (T, ny, nx))).astype(np.int32)


@pytest.mark.parametrize("shape", [(1, 31, 60), (57, 1, 130), (57, 33, 1), (1, 1, 1), (203, 9, 65), (67, 17, 64), (131, 20, 36)])
def test_shapes(trk, shape):
    flag = _random_flag(*shape, seed=sum(shape), density=0.3)
    for gname, ids, G in freq_util.groupings(shape[0]):
        for above in (0, 500):
            _check(flag, ids, G, above, trk.frequency(flag, ids, G, above), (shape, gname, above))
            _check(flag, ids, G, above, trk.frequency(flag, ids, G, above, chunk_steps=5), (shape, gname, above, "chunks"))


def test_slice_lengths_and_load_flavours(trk):
    """T not a multiple of the slice (nor of the unrolled step group), every kernel variant: 16-byte loads (plain / nontemporal) and
    the general path (an unaligned pointer, a plane of ny * nx % 4 != 0)"""
    try:
        for shape in ((203, 24, 40), (203, 9, 65)):
            flag = _random_flag(*shape, seed=7)
            for off in (0, 4):
                base, ptr = _on_device(trk, flag, off)
                try:
                    for sl in (0, 1, 3, 8, 13, 64, 1000):
                        for nt in (False, True, None):
                            trk.debug_set_freq(sl, nt)
                            for gname, ids, G in freq_util.groupings(shape[0]):
                                _check(flag, ids, G, 0, trk.frequency_dev(ptr, *shape, group=ids, ngroups=G), (shape, off, sl, nt, gname))
                finally:
                    trk.free(base)
    finally:
        trk.debug_set_freq(0)


@pytest.mark.parametrize("chunk_steps", [0, 1, 7])
def test_entries_agree(trk, chunk_steps):
    flag = _random_flag(150, 46, 90, seed=11)
    T, ny, nx = flag.shape
    base, ptr = _on_device(trk, flag)
    try:
        for gname, ids, G in freq_util.groupings(T):
            dev = trk.frequency_dev(ptr, T, ny, nx, group=ids, ngroups=G, above=3)
            host = trk.frequency(flag, ids, G, 3, chunk_steps=chunk_steps)
            calls = []

            def reader(t0, nt, out):
                calls.append((t0, nt))
                out[...] = flag[t0:t0 + nt]
            cb = trk.frequency_cb(reader, flag.shape, ids, G, 3, chunk_steps=chunk_steps)
            assert np.array_equal(dev, host) and np.array_equal(dev, cb), (gname, chunk_steps)
            _check(flag, ids, G, 3, dev, gname)
            step = chunk_steps or T
            assert calls == [(t0, min(step, T - t0)) for t0 in range(0, T, step)]
    finally:
        trk.free(base)


def test_accumulate_two_halves(trk):
    flag = _random_flag(121, 31, 60, seed=13)
    T, ny, nx = flag.shape
    base, ptr = _on_device(trk, flag)
    cdev = trk.malloc(3 * ny * nx * 4)
    try:
        ids = (np.arange(T) % 3).astype(np.int32)
        h = 60
        trk.memset(cdev, 0xff, 3 * ny * nx * 4)                    # overwritten by accumulate=0
        trk.frequency_dev(ptr, h, ny, nx, group=ids[:h], ngroups=3, counts_dev=cdev, accumulate=False)
        trk.frequency_dev(C.c_void_p(ptr.value + h * ny * nx * 4), T - h, ny, nx, group=ids[h:], ngroups=3, counts_dev=cdev, accumulate=True)
        got = np.empty((3, ny, nx), dtype=np.uint32)
        trk.d2h(got, cdev)
        _check(flag, ids, 3, 0, got, "halves")
        assert np.array_equal(got, trk.frequency_dev(ptr, T, ny, nx, group=ids, ngroups=3))
    finally:
        trk.free(cdev)
        trk.free(base)


def test_end_to_end_after_track(trk):
    T, ny, nx = 96, 91, 180
    a = synth.smooth_field(T, ny, nx, seed=21)
    lat, _ = synth.grid(ny, nx)
    w = cm.row_weights(lat, np.float32(2.0), np.float32(2.0))
    thr = np.full(T, np.float64(np.quantile(a, 0.9)))
    flag, n = trk.track(a, thr, 0, w, 0.5, 3, True)
    flag = flag.copy()
    assert n > 0 and (flag > 0).any()
    ids = ((np.arange(T) // 8) % 12).astype(np.int32)
    for above in (0, 1):
        assert freq_util.same_bits(cm.frequency_numpy(flag, above=above), freq_util.percent(flag, None, 1, above))
        assert freq_util.same_bits(cm.frequency_numpy(flag, ids, above=above), freq_util.percent(flag, ids, 12, above))


def test_wide_integer_flags(trk):
    flag = _random_flag(40, 13, 21, seed=17)
    for dt in (np.int64, np.uint32, np.int16, np.uint8, np.bool_):
        f = flag.astype(dt)
        assert freq_util.same_bits(cm.frequency_numpy(f, above=0), freq_util.percent(f, None, 1, 0)), dt
    big = flag.astype(np.int64)
    big[20, 3, 4] = 2 ** 31
    with pytest.raises(ValueError, match="int32"):
        cm.frequency_numpy(big)


def test_errors(trk):
    flag = _random_flag(10, 5, 6, seed=1)
    T, ny, nx = flag.shape
    with pytest.raises(ValueError):
        trk.frequency(flag, np.arange(T) % 3, 2)                            # id 2 out of range
    with pytest.raises(ValueError):
        trk.frequency(flag, np.full(T, -1), 2)
    with pytest.raises(ValueError):
        trk.frequency(flag, np.zeros(T, np.int32), 0)                       # ngroups = 0
    with pytest.raises(ValueError):
        trk.frequency(flag[:0])                                             # T = 0
    with pytest.raises(ValueError):
        trk.frequency(flag, np.zeros(T - 1, np.int32), 1)                   # mismatched shape
    with pytest.raises(ValueError):
        trk.frequency(flag[0])
    base, ptr = _on_device(trk, flag)
    try:
        with pytest.raises(ValueError):
            trk.frequency_dev(ptr, T, ny, nx, group=np.arange(T) % 3, ngroups=2)
        with pytest.raises(ValueError):
            trk.frequency_dev(ptr, 0, ny, nx)
        with pytest.raises(ValueError):
            trk.frequency_dev(ptr, T, ny, nx, group=np.zeros(T, np.int32), ngroups=0)
        with pytest.raises(ValueError):
            trk.frequency_dev(ptr, T, ny, nx, counts_dev=C.c_void_p(0))       # NULL buffer
        with pytest.raises(ValueError):
            trk.frequency_cb(lambda t0, nt, out: None, (T, ny, 0))
        with pytest.raises(ValueError):
            cm.frequency_numpy(flag, np.zeros(T + 1, np.int32))
        # the handle still works after the refusals
        _check(flag, None, 1, 0, trk.frequency_dev(ptr, T, ny, nx), "after errors")
    finally:
        trk.free(base)
