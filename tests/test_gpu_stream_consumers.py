"""The streamed map consumers after a reader that gives up, and the four kernel-timing hooks.

A reader that raises on its second call leaves one chunk in flight; every read-only streaming entry goes through one driver
(stream_consume, ctk_api.hip) that waits for it before the error returns.  So the call raises the reader's own exception, and the
next call on the same Tracker gives exactly what a fresh Tracker gives.  (centred_cb and track_stream have their own loops: their
tests are in test_gpu_centred.py and test_gpu_stream.py.)

The timing hooks (time_freq, time_spells, time_composite, time_centred) run the kernel reps + 1 times on accumulators zeroed once:
what is left in the buffers says that the shared loop launched that often."""
import math

import numpy as np
import pytest

import life_forms
from contrack_amd import _native

pytestmark = pytest.mark.gpu

T, NY, CHUNK, G = 5, 3, 2, 2                    # three chunks: [0, 2), [2, 4), [4, 5)
GROUP = np.array([0, 1, 0, 1, 1], dtype=np.int32)
ENTRIES = ["frequency_cb", "spells_cb", "composite_cb:flag", "composite_cb:field", "anomalies_stream", "lifecycle_stream"]


def _tracker():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    return _native.Tracker(0)


def _slabs(nx):
    rng = np.random.default_rng(nx)
    flag = rng.integers(0, 4, size=(T, NY, nx)).astype(np.int32)
    field = rng.integers(-8, 9, size=(T, NY, nx)).astype(np.float32)
    return flag, field


def _reader(slab, fail):
    """reader of `slab`; fail: it raises on its second call, the chunk at t0 = 2"""
    calls = []

    def rd(t0, nt, out):
        calls.append(t0)
        if fail and len(calls) == 2:
            assert t0 == CHUNK
            raise OSError("no such chunk: %d" % t0)
        out[...] = slab[t0:t0 + nt]
    return rd


def _call(trk, entry, flag, field, fail):
    """the entry's result as a tuple of arrays; fail: the reader the entry names gives up"""
    shape = flag.shape
    if entry == "frequency_cb":
        return (trk.frequency_cb(_reader(flag, fail), shape, GROUP, G, chunk_steps=CHUNK),)
    if entry == "spells_cb":
        return trk.spells_cb(_reader(flag, fail), shape, GROUP, G, chunk_steps=CHUNK)
    if entry.startswith("composite_cb"):
        which = entry.split(":")[1]
        return trk.composite_cb(_reader(flag, fail and which == "flag"), _reader(field, fail and which == "field"), shape, np.float32, GROUP, G,
                                chunk_steps=CHUNK)
    if entry == "anomalies_stream":
        return trk.anomalies_stream(_reader(field, fail), GROUP, G, shape=shape, dtype=np.float32, chunk_steps=CHUNK, want_clim=True)
    assert entry == "lifecycle_stream"
    wrow = life_forms.grid(shape[1], shape[2])[2]
    return trk.lifecycle_stream(_reader(flag, fail), _reader(field, False), wrow, shape=shape, dtype=np.float32, chunk_steps=CHUNK)


@pytest.mark.parametrize("nx", [8, 7])           # planes of a multiple of 16 bytes (the 16-byte loads) and not (the scalar path)
@pytest.mark.parametrize("entry", ENTRIES)
def test_reader_gives_up_on_its_second_chunk(entry, nx):
    flag, field = _slabs(nx)
    with _tracker() as fresh:
        want = _call(fresh, entry, flag, field, False)
    with _tracker() as trk:
        with pytest.raises(OSError, match="no such chunk: 2"):
            _call(trk, entry, flag, field, True)
        got = _call(trk, entry, flag, field, False)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), entry
    assert any(np.asarray(a).view(np.uint8).any() for a in want)       # (not a comparison of nothing with nothing)


# ---- the timing hooks ---------------------------------------------------------------------------------------------------------
HT, HNY, HNX, REPS = 6, 4, 8, 3
HGROUP = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)


class Dev:
    """host arrays in fresh device buffers of one Tracker; zeros(shape, dtype): a buffer to read back"""
    def __init__(self, trk):
        self.trk, self.ptrs = trk, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.trk.free(p)

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.trk.malloc(max(a.nbytes, 8))
        self.ptrs.append(p)
        self.trk.h2d(p, a)
        return p

    def get(self, p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self.trk.d2h(out, p)
        return out


def _times_ok(ms):
    best, mean = ms
    assert math.isfinite(best) and math.isfinite(mean) and best > 0 and mean > 0


def _hook_slabs():
    rng = np.random.default_rng(11)
    flag = rng.integers(0, 3, size=(HT, HNY, HNX)).astype(np.int32)
    field = rng.integers(-8, 9, size=(HT, HNY, HNX)).astype(np.float32)       # integers of |x| <= 8: the float64 sums are exact
    return flag, field


def test_time_freq_counts_every_launch():
    flag, _ = _hook_slabs()
    with _tracker() as trk, Dev(trk) as dev:
        fp, cp = dev.put(flag), dev.put(np.zeros((G, HNY, HNX), np.uint32))
        one = trk.frequency_dev(fp, HT, HNY, HNX, HGROUP, G)
        _times_ok(trk.time_freq(fp, HT, HNY, HNX, cp, HGROUP, G, reps=REPS))
        got = dev.get(cp, one.shape, np.uint32)
    assert one.any() and np.array_equal(got, (REPS + 1) * one)


def test_time_composite_continues_every_launch():
    flag, field = _hook_slabs()
    with _tracker() as trk, Dev(trk) as dev:
        fp, xp = dev.put(flag), dev.put(field)
        sp, npt = dev.put(np.zeros((G, HNY, HNX), np.float64)), dev.put(np.zeros((G, HNY, HNX), np.uint32))
        s1, n1 = trk.composite_dev(fp, xp, HT, HNY, HNX, HGROUP, G)
        _times_ok(trk.time_composite(fp, xp, HT, HNY, HNX, sp, npt, HGROUP, G, reps=REPS))
        s, n = dev.get(sp, s1.shape, np.float64), dev.get(npt, n1.shape, np.uint32)
    assert n1.any() and s1.any()
    assert np.array_equal(n, (REPS + 1) * n1) and np.array_equal(s, (REPS + 1) * s1)


def test_time_centred_continues_every_launch():
    _, field = _hook_slabs()
    t, row, col, bins = [0, 2, 2, 3, 5], [1, 0, 3, 2, 1], [0, 7, 3, 4, 6], [0, 1, 0, 1, 0]          # five stamps, two of them on step 2
    nbins, hy, hx = 2, 1, 1
    with _tracker() as trk, Dev(trk) as dev:
        xp = dev.put(field)
        sp, npt = dev.put(np.zeros((nbins, 3, 3), np.float64)), dev.put(np.zeros((nbins, 3, 3), np.uint32))
        s1, n1 = trk.centred_dev(xp, HT, HNY, HNX, t, row, col, bins, nbins, hy, hx)
        _times_ok(trk.time_centred(xp, HT, HNY, HNX, t, row, col, bins, nbins, hy, hx, sp, npt, reps=REPS))
        s, n = dev.get(sp, s1.shape, np.float64), dev.get(npt, n1.shape, np.uint32)
    assert n1.any() and s1.any()
    assert np.array_equal(n, (REPS + 1) * n1) and np.array_equal(s, (REPS + 1) * s1)


def test_time_spells_publishes_every_launch():
    """k_spell alone, every launch from the same empty carry and without k_spell_close: a launch publishes the spells that end inside
    the slab -- events and steps add up over the launches, longest is a maximum.  With the last step unflagged every spell ends inside,
    so one launch publishes what spells_dev returns."""
    flag, _ = _hook_slabs()
    flag[-1] = 0
    with _tracker() as trk, Dev(trk) as dev:
        fp, mp = dev.put(flag), dev.put(np.zeros((3, G, HNY, HNX), np.uint32))
        e0, s0, l0 = trk.spells_dev(fp, HT, HNY, HNX, HGROUP, G)
        _times_ok(trk.time_spells(fp, HT, HNY, HNX, mp, HGROUP, G, reps=REPS))
        e3, s3, l3 = dev.get(mp, (3, G, HNY, HNX), np.uint32)
        _times_ok(trk.time_spells(fp, HT, HNY, HNX, mp, HGROUP, G, reps=1))
        e1, s1, l1 = dev.get(mp, (3, G, HNY, HNX), np.uint32)
    assert e1.any() and s1.any() and l1.any()
    assert np.array_equal(e3, 2 * e1) and np.array_equal(s3, 2 * s1) and np.array_equal(l3, l1)
    assert np.array_equal(e1, 2 * e0) and np.array_equal(s1, 2 * s0) and np.array_equal(l1, l0)
