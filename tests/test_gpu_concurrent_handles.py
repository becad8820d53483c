"""Several handles in one process, one host thread each, all at work at once (tests/concurrent_util.py): what include/contrack_hip.h
and INTEGRATION.md promise of independent handles, and what bench.py's concurrent_members measures, with every answer compared --
exactly, with the references and the io model of tests/handle_sequences.py, which are per handle and must hold unchanged.

What two handles can share is process-wide or device-wide: the HIP runtime's per-function attributes (k_std_field's dynamic LDS
limit, test_std_field_launches_of_different_lds_at_once), the null stream of the synchronous copies, the hardware queues (the HIP runtime
gives a process four by default: test_more_handles_than_hardware_queues uses eight handles), the thread-local message behind
ctk_last_error, and the counters of csrc/ctk_own.h.  Every case asserts the overlap condition: each handle had an operation under way
together with an operation of another handle -- a run that never overlapped has tested nothing.  Never more than eight handles, and
threads only.  Each case prints its wall time and the number of overlapping pairs of operations (measured values, no thresholds)."""
import gc
import threading
import time

import numpy as np
import pytest

import concurrent_util as cu
import freq_util
import handle_sequences as hs
import std_util
from contrack_amd import _native

pytestmark = pytest.mark.gpu

S, O, L = hs.S, hs.O, hs.L


@pytest.fixture(scope="module", autouse=True)
def oracle_built(oracle_lib):
    return oracle_lib


def _trackers(n):
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    assert n <= 8
    return [_native.Tracker(0) for _ in range(n)]


def _overlapped(name, intervals, t0):
    """the overlap condition, and the case's figures on stdout"""
    span = [t for v in intervals for a, b, _ in v for t in (a, b)]
    print("\nconcurrent case %s: %d handles, wall %.2f s (operations %.2f s), %d overlapping pairs of operations"
          % (name, len(intervals), time.perf_counter() - t0, max(span) - min(span) if span else 0.0, cu.overlapping_pairs(intervals)))
    assert cu.every_handle_overlapped(intervals), "no overlap: nothing was tested (handles %s ran alone)" % cu.handles_without_overlap(intervals)


def _together(name, sequences, also=(), more_intervals=()):
    t0 = time.perf_counter()
    trks = _trackers(len(sequences))
    try:
        bad, intervals = cu.run_together(trks, sequences, also=also)
    finally:
        for t in trks:
            t.close()
    assert not bad, "\n".join(repr(b) for b in bad)                  # (one failure per line, none cut short)
    _overlapped(name, intervals + [list(v) for v in more_intervals], t0)
    return intervals


# ---- 1. the seeded sequences, four at a time ------------------------------------------------------------------------------------
def _rounds(n, size=4):
    """range(n) in rounds of `size`; a last round of one takes a seed from the round before it (never fewer than two handles)"""
    r = [list(range(a, min(a + size, n))) for a in range(0, n, size)]
    if len(r) > 1 and len(r[-1]) == 1:
        r[-1].insert(0, r[-2].pop())
    return r


ROUNDS = _rounds(hs.N_SEEDS)


def test_the_rounds_cover_every_seed():
    assert sorted(s for r in ROUNDS for s in r) == list(range(hs.N_SEEDS)) and all(2 <= len(r) <= 4 for r in ROUNDS)
    assert _rounds(9) == [[0, 1, 2, 3], [4, 5, 6], [7, 8]] and _rounds(8) == [[0, 1, 2, 3], [4, 5, 6, 7]] and _rounds(6) == [[0, 1, 2, 3], [4, 5]]


@pytest.mark.parametrize("seeds", ROUNDS, ids=["seeds%d-%d" % (r[0], r[-1]) for r in ROUNDS])
def test_seeded_sequences_four_at_a_time(seeds):
    _together("seeded %s" % seeds, [hs.seeded(s) for s in seeds])


# ---- 2. one family on every handle: bench.py's concurrent_members, with the answers checked -----------------------------------
def _same_family(family, i):
    """three calls of `family` for handle i: every handle its own data (seed) and its own order of the shapes"""
    keys = [(S, O, L)[(i + j) % 3] for j in range(3)]
    dt = ("f4", "f8")[i % 2]
    make = {
        "track": lambda j, k: hs.track(k, dt, thr=(100.0, 130.0)[j % 2], seed=1 + i),
        "track_dev": lambda j, k: hs.track_dev(k, dt, seed=1 + i),
        "anomalies_stream": lambda j, k: hs.anomalies_stream(k, dt, chunk_steps=5 + 2 * j + i, callbacks=bool((i + j) % 2), seed=3 + i),
        "std_field": lambda j, k: hs.std_field(k, dt, seed=3 + i),
        "percentile_field": lambda j, k: hs.percentile_field(k, dt, seed=3 + i),
        "spells": lambda j, k: hs.spells(k, "array", (0, 4, 7)[j], by_id=bool(j % 2), seed=2 + i),
        "lifecycle": lambda j, k: hs.lifecycle(k, dt, seed=1 + i),
        "centred": lambda j, k: hs.centred(k, "array", dt, (0, 5, 9)[j], seed=i),
        "reversal": lambda j, k: hs.reversal(k, dt, "array", (0, 6, 11)[j], keep=j == 1, mask=j == 2, second=bool((i + j) % 2), seed=i),
    }[family]
    return [make(j, k) for j, k in enumerate(keys)]


@pytest.mark.parametrize("family", ["track", "track_dev", "anomalies_stream", "std_field", "percentile_field", "spells", "lifecycle", "centred", "reversal"])
def test_same_family_on_every_handle(family):
    seqs = [_same_family(family, i) for i in range(4)]
    assert all(op.family == family for q in seqs for op in q) and all(len(q) == 3 for q in seqs)
    _together("same family %s" % family, seqs)


# ---- 3. k_std_field: one template instance, launches of different dynamic LDS at the same time ---------------------------------
STD_CALLS = 20                         # a fixed count, not a loop until something happens


def _std_case(G, window, rows, nx, seed):
    """x, group and the reference of a float32 slab of 2 G steps: every group twice, NaNs among the values"""
    T = 2 * G
    rng = np.random.default_rng(seed)
    x = (50.0 * rng.standard_normal((T, rows + 2, nx)) + 5500.0).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    group = (np.arange(T) % G).astype(np.int32)
    return x, group, std_util.want_std(x, (1, rows + 1), group, G, window, 1, True)


def _std_op(case, G, window, tile, lds):
    x, group, want = case
    assert std_util.plan_py(G, window, True)["tile"] == tile and std_util.plan_py(G, window, True)["lds_bytes"] == lds

    def run(trk, env):
        got = trk.std_field(x, 1, x.shape[1] - 1, group, G, window, 1, True, want_mean=True, want_n=True)
        return got, trk.debug_std_field_form()[0]
    return hs.Op("std_field", None, run, lambda: want, lambda got, w: hs.same_std(got[0], w) and got[1] == tile, dict(hs.NO_IO, io_in=x.nbytes), note="G=%d window=%d: %d bytes of LDS" % (G, window, lds))


@pytest.mark.parametrize("tile,window,small", [(32, 3, 5), (16, 31, 366)], ids=["tile32", "tile16"])
def test_std_field_launches_of_different_lds_at_once(tile, window, small):
    """float32, skipna, a window at most as wide as the owners of a pixel: k_std_field<float, tile, true, true> on both handles, one
    with few planes, one with as many as the tile holds.  The dynamic LDS limit of that function is one per process"""
    large = std_util.planes_max(tile, True)
    assert large == {32: 230, 16: 486}[tile] and window <= 512 // tile and (tile == 32 or small > std_util.planes_max(32, True))
    lds = [std_util.plan_py(G, window, True)["lds_bytes"] for G in (small, large)]
    assert lds[0] < lds[1] <= std_util.LDS_BYTES and lds[1] > 65536 and lds[1] > std_util.LDS_BYTES - tile * 20
    if tile == 32:
        assert lds[0] < 20 * 1024 and lds[1] > 159 * 1024                     # about 19 KB against about 160 KB
    cases = [_std_case(G, window, 3, 40, 10 + k) for k, G in enumerate((small, large))]
    ops = [_std_op(c, G, window, tile, b) for c, G, b in zip(cases, (small, large), lds)]
    _together("std_field tile %d, %d and %d bytes of LDS" % (tile, lds[0], lds[1]), [[op] * STD_CALLS for op in ops])


# ---- 4. more handles than hardware queues ----------------------------------------------------------------------------------------
def test_more_handles_than_hardware_queues():
    written = [hs.io_grows_and_shrinks, hs.tracking_caches, hs.resident_anomaly_survives, hs.reversal_between_the_others]
    _together("eight handles, written sequences", [written[k % 4]() for k in range(8)])


# ---- 5. the message behind ctk_last_error is the calling thread's --------------------------------------------------------------
N_REFUSALS = 50


def test_error_messages_stay_with_their_thread():
    """four threads, each on its own handle, each refused 50 times for an argument of its own with a value nobody else uses.  An
    operation here is the refused call AND the reading of its message; the threads meet at a barrier between the two, so in every
    iteration all four have been refused before any of them reads -- a message kept per process would be somebody else's for three
    of them.  (The refusals take microseconds under the interpreter's lock: left to chance, the four would seldom interleave.)
    Host-side refusals: nothing is launched"""
    t_case = time.perf_counter()
    Lb = _native.lib()
    T, ny, nx = 4, 3, 8
    flag = np.ones((T, ny, nx), dtype=np.int32)
    x = np.ones((T, ny, nx), dtype=np.float32)
    group = np.zeros(T, dtype=np.int32)
    maps = [np.zeros((1, ny, nx), dtype=np.uint32) for _ in range(3)]
    out = np.zeros((1, 1, nx), dtype=np.float64)
    p = lambda a: a.ctypes.data                                                # noqa: E731
    calls = [
        ("min_duration=%d ", lambda h, v: Lb.ctk_spells(h, p(flag), T, ny, nx, None, 1, None, 0, 0, 1, v, p(maps[0]), p(maps[1]), p(maps[2]), 0)),
        ("by_id=%d ", lambda h, v: Lb.ctk_spells(h, p(flag), T, ny, nx, None, 1, None, 0, 0, v, 1, p(maps[0]), p(maps[1]), p(maps[2]), 0)),
        ("ngroups=%d ", lambda h, v: Lb.ctk_frequency(h, p(flag), T, ny, nx, None, v, 0, p(maps[0]), 0)),
        ("window=%d ", lambda h, v: Lb.ctk_std_field_f32(h, p(x), T, ny, nx, 1, 2, p(group), 1, v, 0, 1, p(out), None, None)),
    ]
    trks = _trackers(4)
    step = threading.Barrier(4)
    wrong, intervals, raised = [[] for _ in range(4)], [[] for _ in range(4)], [None] * 4

    def work(k):
        try:
            h = trks[k].handle
            step.wait(60.0)
            for it in range(N_REFUSALS):
                v = -(1000 * (k + 1) + it)                                    # negative: refused by every one of the four checks
                t0 = time.perf_counter()
                rc = calls[k][1](h, v)
                step.wait(60.0)                                               # every thread has been refused by now
                msg = Lb.ctk_last_error().decode("utf-8", "replace")
                t1 = time.perf_counter()
                intervals[k].append((t0, t1, it))
                own = calls[k][0] % v
                if rc != -1 or own not in msg:
                    wrong[k].append((it, rc, own, msg))
        except BaseException as e:                                              # noqa: BLE001
            step.abort()
            raised[k] = e
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(120.0)
        assert not any(t.is_alive() for t in threads)
        for e in raised:
            if e is not None and not isinstance(e, threading.BrokenBarrierError):
                raise e
        assert raised == [None] * 4
        assert wrong == [[], [], [], []], wrong
        assert [len(v) for v in intervals] == [N_REFUSALS] * 4
        # the handles are usable afterwards
        for k, t in enumerate(trks):
            assert hs.same_ints(t.frequency(hs.flags(S)), freq_util.counts(hs.flags(S), None, 1, 0)), k
    finally:
        for t in trks:
            t.close()
    _overlapped("error messages", intervals, t_case)


# ---- 6. handles come and go while others work ------------------------------------------------------------------------------------
def test_handles_closed_while_others_work():
    t_case = time.perf_counter()
    gc.collect()                                                              # (no forgotten handle of an earlier test goes meanwhile)
    before = _native.debug_live()
    want = freq_util.counts(hs.flags(O), hs.groups(O, 3), 3, 0)
    short_lived, wrong = [], []

    def come_and_go(stop):
        for k in range(6):
            if stop.is_set():
                return
            t0 = time.perf_counter()
            with _native.Tracker(0) as t:
                got = t.frequency(hs.flags(O), hs.groups(O, 3), 3, 0, 5)
            short_lived.append((t0, time.perf_counter(), k))
            if not hs.same_ints(got, want):
                wrong.append(k)
    trks = _trackers(2)
    try:
        bad, intervals = cu.run_together(trks, [hs.seeded(0), hs.seeded(1)], also=[come_and_go])
    finally:
        for t in trks:
            t.close()
    assert not bad, "\n".join(repr(b) for b in bad)
    assert wrong == [] and len(short_lived) == 6
    gc.collect()
    assert _native.debug_live() == before
    _overlapped("handles closed meanwhile", intervals + [short_lived], t_case)
