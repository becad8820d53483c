"""Segment breaks given with a time-shard call (ctk_track_sharded_seg_*_dev, Tracker.track_sharded_dev(..., segments=)): N handles on
one GPU play N ranks (tests/shard_inproc.py), the starts are global step indices, the same on every rank.  Breaks fall on shard
cuts, next to them, inside shards; shards lie inside segments and segments inside shards.  The result is what the one-call entries
give with ctk_set_segments: the C oracle on every segment alone, ids shifted (tests/segment_util.py)."""
import numpy as np
import pytest

import segment_cases as sc
import segment_util as su
from contrack_amd import _native
from shard_inproc import sharded_threads

pytestmark = pytest.mark.gpu

GOLDENS = ("T3", "syn2deg_s0", "chain_a", "chain_b", "busy_s2", "noise", "nan_planes", "refslab_two")
WORLDS = (2, 3, 5)


@pytest.fixture(scope="module")
def handles():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    hs = [_native.Tracker(0) for _ in range(5)]
    yield hs
    for h in hs:
        h.close()


class WithSegments:
    """a Tracker whose track_sharded_dev passes segments= (what shard_inproc.sharded_threads does not know about)"""

    def __init__(self, trk, starts):
        self._trk, self._starts = trk, starts

    def __getattr__(self, name):
        return getattr(self._trk, name)

    def track_sharded_dev(self, *a, **k):
        return self._trk.track_sharded_dev(*a, segments=self._starts, **k)


def seg_sharded(handles, g, cuts, starts, f64=False):
    trks = [WithSegments(h, starts) for h in handles[:len(cuts) - 1]]
    return sharded_threads(trks, g["anom"], *sc.args(g), cuts, f64=f64)


def cuts_of(T, n):
    c = sorted(set(int(round(T * k / n)) for k in range(n + 1)))
    return c if len(c) == n + 1 else None


def uniq(starts, T):
    return np.array(sorted(set(int(s) for s in starts if 0 <= s < T) | {0}), dtype=np.int64)


def segmentations(T, cuts):
    """segment_util's (one segment: every shard inside it; random; short segments inside shard 0 and the last; a break before every
    step) and, relative to the interior cuts C: a break exactly on every cut; breaks one step before and one after every cut (none
    on it: a two-step segment spans the cut); single-step segments on both sides of every cut; a break on the first cut only (the
    shards behind it lie inside one segment)"""
    C = cuts[1:-1]
    out = dict(su.segmentations(T))
    out["on_cuts"] = uniq(C, T)
    out["beside_cuts"] = uniq([c - 1 for c in C if c - 1 not in C] + [c + 1 for c in C if c + 1 not in C], T)
    out["single_steps_at_cuts"] = uniq([c - 1 for c in C] + list(C) + [c + 1 for c in C], T)
    out["first_cut_only"] = uniq(C[:1], T)
    return out


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens_segmented_sharded(handles, name, world):
    g = sc.golden(name)
    T = g["anom"].shape[0]
    cuts = cuts_of(T, world)
    if cuts is None:                                   # (T3 in five shards: fewer steps than ranks; its 2- and 3-shard cases run)
        assert name == "T3" and world == 5
        cuts = [0, 1, 2, 3]
    for sname, starts in segmentations(T, cuts).items():
        want, nw = sc.expected(name, starts)
        got, ng, _ = seg_sharded(handles, g, cuts, starts)          # (n_tracked equal on all ranks: sharded_threads asserts it)
        where = "{} / {} {} / cuts {}".format(name, sname, starts.tolist(), cuts)
        assert np.array_equal(got, want), "{}: flag differs at {} pixels".format(where, int((got != want).sum()))
        assert ng == nw, "{}: n_tracked {} != {}".format(where, ng, nw)


def test_uneven_cuts_and_float64(handles):
    """one-step shards between longer ones, breaks on, before and after them; a float64 slab"""
    g = sc.golden("syn2deg_s1")
    T = g["anom"].shape[0]
    cuts = [0, 20, 21, 22, 50, T]
    for starts in ([0, 21], [0, 20, 21, 22], [0, 22, 51], [0, 19, 23, 49], [0, 21, 22, 50]):
        want, nw = sc.expected("syn2deg_s1", starts)
        for f64 in (False, True):
            got, ng, _ = seg_sharded(handles, g, cuts, np.array(starts), f64=f64)
            assert np.array_equal(got, want) and ng == nw, (starts, f64)


def test_world_of_one_is_the_one_call_result(handles):
    g = sc.golden("busy_s2")
    T = g["anom"].shape[0]
    for starts in su.segmentations(T).values():
        trk = handles[1]
        trk.set_segments(starts)
        try:
            one, n1 = trk.track(g["anom"], *sc.args(g))
            one = one.copy()
        finally:
            trk.clear_segments()
        got, ng, _ = seg_sharded(handles, g, [0, T], starts)
        assert np.array_equal(got, one) and ng == n1
        want, nw = sc.expected("busy_s2", starts)
        assert np.array_equal(got, want) and ng == nw


def test_one_segment_is_the_unsegmented_call(handles):
    """segments=[0] (and none): the unsegmented sharded result from the unsegmented kernel builds; breaks: the SEG builds on the
    shards they touch, the unsegmented ones on a shard inside one segment (CTK_S_OVERLAP_FORM carries the SEG offset; the time-shard
    path reports no filter forms)"""
    g = sc.golden("syn2deg_s0")
    T = g["anom"].shape[0]
    cuts = cuts_of(T, 3)
    ref, nref, st_ref = sharded_threads(handles[:3], g["anom"], *sc.args(g), cuts)
    assert np.array_equal(ref, g["flag"])
    for starts in ([0], []):
        got, n, st = seg_sharded(handles, g, cuts, np.array(starts, dtype=np.int64))
        assert np.array_equal(got, ref) and n == nref
        for a, b in zip(st, st_ref):
            assert a["overlap_form"] == b["overlap_form"] < 1000000
    got, n, st = seg_sharded(handles, g, cuts, np.array([0, 5]))          # a break inside shard 0 only
    assert st[0]["overlap_form"] == st_ref[0]["overlap_form"] + 1000000
    assert st[1]["overlap_form"] == st_ref[1]["overlap_form"] and st[2]["overlap_form"] == st_ref[2]["overlap_form"]
    want, nw = sc.expected("syn2deg_s0", [0, 5])
    assert np.array_equal(got, want) and n == nw


@pytest.mark.parametrize("mode", ["host_seam_driver", "per_pass_filter"])
def test_fallbacks(handles, mode):
    """the host-driven seam form on every rank and the filter with one launch per pass"""
    hs = [_native.Tracker(0) for _ in range(3)]
    try:
        for h in hs:
            if mode == "host_seam_driver":
                h.debug_set_seam_caps(1, 1)
            else:
                h.set_fused(False)
        for name in ("syn2deg_s0", "chain_a", "busy_s2"):
            g = sc.golden(name)
            T = g["anom"].shape[0]
            cuts = cuts_of(T, 3)
            for sname, starts in segmentations(T, cuts).items():
                want, nw = sc.expected(name, starts)
                got, ng, _ = seg_sharded(hs, g, cuts, starts)
                assert np.array_equal(got, want) and ng == nw, (mode, name, sname)
    finally:
        for h in hs:
            h.close()


def one_rank_call(trk, g, starts, T_total=None):
    """a world of one through the C entry; every refusal retires the communicator, so each call gets its own"""
    a = g["anom"]
    T, ny, nx = a.shape
    grp = _native.CommGroup(1)
    comm = _native.Comm.local(trk, grp, 0)
    d_in, d_out = trk.malloc(a.nbytes), trk.malloc(a.size * 4)
    try:
        trk.h2d(d_in, a)
        n = trk.track_sharded_dev(comm, d_in, T, 0, T if T_total is None else T_total, ny, nx, *sc.args(g), d_out, segments=starts)
        f = np.empty(a.shape, np.int32)
        trk.d2h(f, d_out)
        return f, n
    finally:
        comm.close()
        grp.close()
        trk.free(d_in)
        trk.free(d_out)


def test_refusals(handles):
    g = sc.golden("T3")
    T = g["anom"].shape[0]
    trk = handles[0]
    for bad in ([1, 2], [0, 2, 2], [0, 2, 1], [0, -1], [0, T], [0, 1, T + 4]):
        with pytest.raises(ValueError, match="segment"):
            one_rank_call(trk, g, bad)
    trk.set_segments([0, 1])                               # sticky segments and the call's own: refused
    try:
        with pytest.raises(ValueError, match="segments"):
            one_rank_call(trk, g, [0, 2])
    finally:
        trk.clear_segments()
    f, n = one_rank_call(trk, g, [0, 2])                   # the handle is fine afterwards
    want, nw = sc.expected("T3", [0, 2])
    assert np.array_equal(f, want) and n == nw
