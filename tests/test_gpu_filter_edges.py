"""The streamed entries of the time filter (ctk_filter_f32 / _f64 with chunk_steps, ctk_filter_stream_cb) and its resident chain: the
chunks pass through windows that keep the last K - 1 steps of the chunk before on the device, so a wrong halo shows as wrong bits in the
first outputs of a chunk and a reader asked twice shows in the callback's own count.  Everything is compared bit for bit with the numpy
statement (tests/filter_util.py) and with the entry on slabs in device memory."""
import numpy as np
import pytest

from contrack_amd import _native

import filter_util as fu
from filter_util import same_bits
from test_gpu_filter import _dev, _weights, steer, trk      # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu

RING, PLAIN = 1, 0
NY, NX = 3, 85


def _chunks(K, T):
    """chunk_steps at the edges: the minimum K - 1, K, one that leaves a last chunk of one step, and one chunk for everything"""
    one_left = next(c for c in range(K + 1, T) if T % c == 1)
    return (K - 1, K, one_left, T + 5)


class Reader:
    """serves x and records what it was asked for"""

    def __init__(self, x):
        self.x, self.asked = x, []

    def __call__(self, t0, nt, out):
        self.asked.append((t0, nt))
        out[...] = self.x[t0:t0 + nt]

    def check(self, chunk):
        """every step once, in rising order, in chunks of `chunk` steps"""
        T = self.x.shape[0]
        c = min(chunk, T)
        assert self.asked == [(t0, min(c, T - t0)) for t0 in range(0, T, c)], (chunk, self.asked[:6])


class Writer:
    def __init__(self, out):
        self.out, self.got = out, []

    def __call__(self, t0, nt, values):
        self.got.append((t0, nt))
        self.out[t0:t0 + nt] = values

    def check(self, T_out):
        """every output once, in rising order"""
        assert [t0 for t0, _ in self.got] == list(np.cumsum([0] + [nt for _, nt in self.got[:-1]])) and sum(nt for _, nt in self.got) == T_out, self.got[:6]


CASES = [
    dict(K=9, stride=1),                                                    # the centred filter: every chunk needs its halo
    dict(K=9, stride=1, edges="renorm", segments=[0, 40, 41, 77]),          # breaks inside chunks and on chunk edges
    dict(K=8, stride=3, offset=-2),                                         # windows over both ends of the axis
    dict(K=4, stride=4),                                                    # block means: no tap shared, the plain form
    dict(K=5, stride=7, offset=1, segments=[0, 33]),                        # steps between the windows that no output uses
    dict(K=2, stride=1, skipna=True),                                       # the shortest halo
]


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "K%d_s%d" % (c["K"], c["stride"]))
def test_streamed_entries_at_the_chunk_edges(trk, steer, dtype, case):
    kw = dict(case)
    K, T = kw.pop("K"), 97
    x = fu.edge_field(T, NY, NX, dtype, seed=K)
    positive = kw.get("edges") == "renorm" or kw.get("skipna", False)
    for weights in (_weights(K, K, positive=positive), K):
        want = fu.time_filter(x, weights, **kw)
        T_out = want.shape[0]
        assert same_bits(_dev(trk, x, weights, **kw), want)
        for forced in (-1, PLAIN) if kw["stride"] < K else (-1, RING):
            steer(0, 0, forced)
            for chunk in _chunks(K, T):
                got = trk.time_filter(x, weights, chunk_steps=chunk, **kw)
                assert same_bits(got, want), ("array", dtype.__name__, case, forced, chunk)
                nchunks = -(-T // min(max(chunk, K - 1, 1), T))
                assert 1 <= trk.debug_filter_launch()["launches"] <= nchunks
                rd, out = Reader(x), np.full_like(want, 7)
                wr = Writer(out)
                assert trk.time_filter_cb(rd, x.shape, dtype, weights, sink=wr, chunk_steps=chunk, **kw) is None
                rd.check(max(chunk, K - 1, 1))
                wr.check(T_out)
                assert same_bits(out, want), ("callbacks", dtype.__name__, case, forced, chunk)
        rd = Reader(x)                                                        # a reader into an array the entry makes; kept in HBM too
        got = trk.time_filter_cb(rd, x.shape, dtype, weights, chunk_steps=K, keep_resident=True, **kw)
        rd.check(K)
        assert same_bits(got, want) and trk.resident_level_mean() == (T_out, NY, NX, dtype == np.float64)


def test_streamed_halo_is_what_the_bits_depend_on(trk, steer):
    """the first outputs after a chunk edge read K - 1 steps of the chunk before: with those steps changed the statement changes there,
    so a halo that is missing, short or stale cannot give these bits (checked on the CPU, then the entry is held against both)"""
    K, T, chunk = 9, 60, 10
    x = fu.edge_field(T, NY, NX, np.float64, seed=4)
    x = np.where(np.isfinite(x), x, 1.0)
    w = _weights(K, 1)
    want = fu.time_filter(x, w)
    for c0 in range(chunk, T, chunk):
        y = x.copy()
        y[c0 - (K - 1):c0] += 1.0                                             # what the halo of the chunk at c0 must hold
        other = fu.time_filter(y, w)
        first = slice(c0 - K // 2, c0 + K // 2)                               # outputs whose window straddles the chunk edge
        ok = np.isfinite(want[first])
        assert ok.any() and np.all(other[first][ok] != want[first][ok])
    assert same_bits(trk.time_filter(x, w, chunk_steps=chunk), want)
    steer(0, 0, PLAIN)
    assert same_bits(trk.time_filter(x, w, chunk_steps=chunk), want)


# ---- the resident chain on a shared handle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=lambda v: v.__name__)
def test_resident_chain(trk, dtype):
    T, K, G = 90, 7, 5
    rng = np.random.default_rng(8)
    x4 = (rng.standard_normal((T, 3, NY, NX)) * 50).astype(dtype)
    lw = np.array([1.0, 2.0, 0.5])
    w = _weights(K, 2, positive=True)
    group = (np.arange(T) % G).astype(np.int32)
    # time_filter(keep_resident) -> anomalies_resident: the bits of anomalies on the filtered host array
    x = x4[:, 0].copy()
    filt = trk.time_filter(x, w, edges="renorm", segments=[0, 50], keep_resident=True)
    assert same_bits(filt, fu.time_filter(x, w, edges="renorm", segments=[0, 50]))
    assert trk.resident_level_mean() == (T, NY, NX, dtype == np.float64)
    want_a, want_c = trk.anomalies(filt, group, G, window=3, smooth=4, want_clim=True, segments=[0, 50])
    gen = trk.resident_level_mean_generation()
    got_a, got_c = trk.anomalies_resident(group, G, window=3, smooth=4, want_clim=True, segments=[0, 50])
    assert same_bits(got_a, want_a) and same_bits(got_c, want_c) and trk.resident_level_mean_generation() == gen
    # level_mean(keep_resident) -> time_filter_resident: the bits of time_filter on the host mean; the slot is not filtered in place
    mean = trk.level_mean(x4, lw, keep_resident=True)
    assert trk.resident_level_mean_generation() != gen                       # (a level_mean call: a filter result recorded before is stale)
    gen = trk.resident_level_mean_generation()
    want = fu.time_filter(mean, w)
    assert same_bits(trk.time_filter_resident(w), want) and trk.resident_level_mean_generation() == gen
    assert same_bits(trk.time_filter_resident(w), want)                      # (again: the mean is still the mean)
    daily = trk.time_filter_resident(4, stride=4, keep_resident=True)        # ... and now the slot holds the block means
    assert same_bits(daily, fu.time_filter(mean, 4, stride=4))
    assert trk.resident_level_mean() == (daily.shape[0], NY, NX, dtype == np.float64) and trk.resident_level_mean_generation() != gen
    g2 = (np.arange(daily.shape[0]) % 3).astype(np.int32)
    assert same_bits(trk.anomalies_resident(g2, 3, smooth=2)[0], trk.anomalies(daily, g2, 3, smooth=2, segments=[0])[0])
    assert same_bits(trk.time_filter_resident(w, want_out=True), fu.time_filter(daily, w))
    with pytest.raises(ValueError):
        trk.time_filter_resident(w, want_out=False)
    # without keep_resident a host call leaves the slot alone
    before = trk.resident_level_mean_generation()
    trk.time_filter(x, w)
    assert trk.resident_level_mean_generation() == before and trk.resident_level_mean() == (daily.shape[0], NY, NX, dtype == np.float64)
    trk.release_io()
    assert trk.resident_level_mean() is None
    with pytest.raises(_native.ContrackHipError, match="no vertical mean is resident"):
        trk.time_filter_resident(w)
