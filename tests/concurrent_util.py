"""Several handles at once, one host thread each (include/contrack_hip.h and INTEGRATION.md name this as a supported use; bench.py's
concurrent_members measures it): the runner of tests/test_gpu_concurrent_handles.py, and what tests/test_concurrent_host.py checks
about it without a GPU.

run_together(trackers, sequences) runs sequence k on tracker k through handle_sequences.run_sequence, every comparison as exact as
there.  What the threads share is kept out of their way beforehand: every reference is computed in the calling thread (the
lru_caches of handle_sequences fill there, and the C oracle runs single-threaded), and the threads only start -- together, from a
barrier -- once all of them are there.  A thread whose operation raises sets `stop`; every thread looks at `stop` before each
operation and starts nothing more once it is set; what was raised is raised again in the caller after all threads have joined.

A run in which no two operations of different handles were under way at the same time has tested nothing: overlapping_pairs counts
them from the intervals run_together returns, and every_handle_overlapped is the condition the GPU cases assert."""
import copy
import threading
import time

import handle_sequences as hs

JOIN_SECONDS = 600.0                   # (a thread that has not come back by then is reported, not waited for)


class Stopped(Exception):
    """raised instead of starting an operation after another thread gave up"""


def _guarded(op, stop):
    """the same operation, which does not start once `stop` is set and sets it when it raises (the families' expected refusals and
    readers that give up are caught inside Op.run: whatever escapes it is unexpected)"""
    g = copy.copy(op)

    def run(trk, env):
        if stop.is_set():
            raise Stopped(repr(op))
        try:
            return op.run(trk, env)
        except BaseException:
            stop.set()
            raise
    g.run = run
    return g


def run_together(trackers, sequences, stop=None, also=(), barrier_seconds=60.0):
    """-> (failures, intervals): failures as run_sequence reports them, each prefixed with the index of its handle; intervals[k] the
    (t_start, t_end, position) of every operation handle k ran, time.perf_counter() around Op.run.  An exception of a thread is
    raised again here after all threads have joined (the first by handle index; Stopped only if nothing else was raised).
    also: callables fn(stop) that run in threads of their own from the same barrier on (work that is no sequence on a handle); what
    they raise is treated like a sequence's."""
    assert len(trackers) == len(sequences) and len(trackers) >= 1
    n = len(trackers)
    wants = [[op.want() for op in seq] for seq in sequences]                  # here, in the calling thread
    stop = stop or threading.Event()
    barrier = threading.Barrier(n + len(also))
    failures, intervals, raised = [[] for _ in range(n)], [[] for _ in range(n)], [None] * (n + len(also))

    def work(k):
        try:
            barrier.wait(barrier_seconds)
            if k >= n:
                also[k - n](stop)
                return
            ops = [_guarded(op, stop) for op in sequences[k]]
            bad = hs.run_sequence(trackers[k], ops, hs.Env(), wants=wants[k], on_op=lambda i, op, t0, t1: intervals[k].append((t0, t1, i)))
            failures[k] = [(k,) + tuple(b) for b in bad]
        except BaseException as e:                                          # noqa: BLE001  (kept for the caller)
            stop.set()
            raised[k] = e
    threads = [threading.Thread(target=work, args=(k,), name="handle-%d" % k) for k in range(n + len(also))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_SECONDS
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    hung = [t.name for t in threads if t.is_alive()]
    if hung:
        stop.set()
        raise RuntimeError("threads still running after %.0f s: %s" % (JOIN_SECONDS, ", ".join(hung)))
    real = [e for e in raised if e is not None and not isinstance(e, (Stopped, threading.BrokenBarrierError))]
    other = [e for e in raised if e is not None]
    if real or other:
        raise (real or other)[0]
    return [b for f in failures for b in f], intervals


def intersect(a, b):
    """two intervals (t_start, t_end, ...) share more than an instant"""
    return a[0] < b[1] and b[0] < a[1]


def overlapping_pairs(intervals):
    """the number of pairs (operation of handle i, operation of handle j > i) whose intervals intersect"""
    return sum(1 for i in range(len(intervals)) for j in range(i + 1, len(intervals)) for a in intervals[i] for b in intervals[j] if intersect(a, b))


def handles_without_overlap(intervals):
    """the handles none of whose operations was under way together with an operation of another handle"""
    return [i for i in range(len(intervals))
            if not any(intersect(a, b) for j in range(len(intervals)) if j != i for a in intervals[i] for b in intervals[j])]


def every_handle_overlapped(intervals):
    return len(intervals) >= 2 and not handles_without_overlap(intervals)
