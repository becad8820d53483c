"""tests/concurrent_util.py without a GPU: fake trackers and operations that sleep a few milliseconds.  The barrier starts the threads
together, `stop` keeps a thread from starting its next operation, what a thread raises surfaces in the caller, failures carry the
index of their handle, the references are computed in the calling thread, and the overlap condition is right on hand-made
intervals."""
import threading
import time

import pytest

import concurrent_util as cu
import handle_sequences as hs


class FakeTracker:
    def debug_io_bytes(self):
        return dict(hs.NO_IO)

    def stats(self):
        return dict(ambiguous_decisions=0)


def _op(name, seconds=0.0, value=1, want=1, raises=None, log=None, want_threads=None):
    def run(trk, env):
        if log is not None:
            log.append((name, time.perf_counter()))
        if seconds:
            time.sleep(seconds)
        if raises is not None:
            raise raises
        return value

    def reference():
        if want_threads is not None:
            want_threads.append(threading.current_thread())
        return want
    return hs.Op(name, None, run, reference, lambda got, w: got == w)


def test_the_overlap_condition_on_hand_made_intervals():
    disjoint = [[(0.0, 1.0, 0), (2.0, 3.0, 1)], [(1.5, 1.9, 0), (3.5, 4.0, 1)]]
    assert cu.overlapping_pairs(disjoint) == 0 and cu.handles_without_overlap(disjoint) == [0, 1] and not cu.every_handle_overlapped(disjoint)
    touching = [[(0.0, 1.0, 0)], [(1.0, 2.0, 0)]]                               # the end of one is the start of the other: no overlap
    assert not cu.intersect(*[h[0] for h in touching]) and cu.overlapping_pairs(touching) == 0 and not cu.every_handle_overlapped(touching)
    nested = [[(0.0, 10.0, 0)], [(2.0, 3.0, 0), (4.0, 5.0, 1)]]
    assert cu.overlapping_pairs(nested) == 2 and cu.every_handle_overlapped(nested)
    partly = [[(0.0, 2.0, 0)], [(1.0, 3.0, 0)], [(5.0, 6.0, 0)]]                # the third handle ran alone
    assert cu.overlapping_pairs(partly) == 1 and cu.handles_without_overlap(partly) == [2] and not cu.every_handle_overlapped(partly)
    chain = [[(0.0, 2.0, 0)], [(1.0, 4.0, 0)], [(3.0, 6.0, 0)]]                 # 0-1 and 1-2 overlap, 0-2 do not: every handle overlapped
    assert cu.overlapping_pairs(chain) == 2 and cu.every_handle_overlapped(chain)
    assert not cu.every_handle_overlapped([[(0.0, 1.0, 0)]]) and not cu.every_handle_overlapped([])            # one handle overlaps nobody
    assert cu.overlapping_pairs([[(0.0, 1.0, 0), (0.5, 1.5, 1)], []]) == 0      # (operations of ONE handle do not count)


def test_the_barrier_starts_the_threads_together(monkeypatch):
    """the threads are started 50 ms apart (a Thread whose start() lingers): without the barrier the first operations would begin
    100 ms apart, with it they begin when the last thread has arrived"""
    gap = 0.05

    class Slow(threading.Thread):
        def start(self):
            super().start()
            time.sleep(gap)
    monkeypatch.setattr(cu.threading, "Thread", Slow)
    log = []
    t0 = time.perf_counter()
    bad, intervals = cu.run_together([FakeTracker() for _ in range(3)], [[_op("h%d" % k, 0.02, log=log), _op("second%d" % k)] for k in range(3)])
    assert bad == [] and [len(v) for v in intervals] == [2, 2, 2]
    first = [t for name, t in log if name.startswith("h")]
    assert len(first) == 3 and min(first) - t0 >= 2 * gap * 0.9                 # nobody began before the last thread was started
    assert max(first) - min(first) < gap                                       # ... and then all of them did
    assert cu.every_handle_overlapped(intervals) and cu.overlapping_pairs([[v[0]] for v in intervals]) == 3
    assert [[i for _, _, i in v] for v in intervals] == [[0, 1]] * 3 and all(a <= b for v in intervals for a, b, _ in v)


def test_references_are_computed_in_the_calling_thread_before_any_operation_runs():
    who, log = [], []
    seqs = [[_op("a%d" % k, 0.005, log=log, want_threads=who), _op("b%d" % k, log=log, want_threads=who)] for k in range(2)]
    t_before = time.perf_counter()
    bad, _ = cu.run_together([FakeTracker(), FakeTracker()], seqs)
    assert bad == [] and len(who) == 4 and all(t is threading.current_thread() for t in who)
    assert len(log) == 4 and min(t for _, t in log) >= t_before


def test_stop_keeps_a_thread_from_starting_its_next_operation():
    log = []
    boom = ValueError("handle 0 gives up")
    seqs = [[_op("boom", raises=boom, log=log), _op("never0", log=log)],
            [_op("slow", 0.05, log=log), _op("never1", log=log), _op("never1b", log=log)]]
    with pytest.raises(ValueError, match="handle 0 gives up") as e:
        cu.run_together([FakeTracker(), FakeTracker()], seqs)
    assert e.value is boom
    assert sorted(name for name, _ in log) == ["boom", "slow"]                  # the operation under way ends; nothing starts after it
    # an event that is already set: no operation starts at all, and that is what the caller hears
    log.clear()
    stop = threading.Event()
    stop.set()
    with pytest.raises(cu.Stopped):
        cu.run_together([FakeTracker(), FakeTracker()], [[_op("x", log=log)], [_op("y", log=log)]], stop=stop)
    assert log == []


def test_an_exception_in_one_thread_surfaces_after_all_threads_have_joined():
    class Odd(Exception):
        pass
    log = []
    seqs = [[_op("fine", 0.03, log=log)], [_op("first", 0.01, log=log), _op("bad", raises=Odd("in handle 1"), log=log)], [_op("also fine", 0.03, log=log)]]
    before = threading.active_count()
    with pytest.raises(Odd, match="in handle 1"):
        cu.run_together([FakeTracker() for _ in range(3)], seqs)
    assert threading.active_count() == before                                  # every thread has joined
    assert {"fine", "also fine", "first", "bad"} == {name for name, _ in log}
    # BaseException too (a KeyboardInterrupt delivered to a thread, SystemExit): it is kept and raised here
    with pytest.raises(SystemExit):
        cu.run_together([FakeTracker(), FakeTracker()], [[_op("exit", raises=SystemExit(3))], [_op("other", 0.01)]])


def test_failures_carry_the_index_of_their_handle():
    seqs = [[_op("right"), _op("right too")], [_op("right"), _op("wrong", value=2)], [_op("wrong first", value=0)]]
    bad, intervals = cu.run_together([FakeTracker() for _ in range(3)], seqs)
    assert [(b[0], b[1], b[3]) for b in bad] == [(1, 1, "differs from its reference"), (2, 0, "differs from its reference")]
    assert "wrong" in bad[0][2] and [len(v) for v in intervals] == [2, 2, 1]


def test_run_sequence_alone_is_what_it_was():
    """without wants= and on_op= the references come from Op.want, and nothing is timed for anybody"""
    who = []
    ops = [_op("a", want_threads=who), _op("b", value=3, want_threads=who)]
    assert [b[:3] for b in hs.run_sequence(FakeTracker(), ops)] == [(1, repr(ops[1]), "differs from its reference")] and len(who) == 2
    seen = []
    assert hs.run_sequence(FakeTracker(), ops, wants=[1, 3], on_op=lambda i, op, t0, t1: seen.append((i, op, t0 <= t1))) == []
    assert seen == [(0, ops[0], True), (1, ops[1], True)] and len(who) == 2     # Op.want was not asked again
