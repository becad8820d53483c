"""Segment breaks given with a streaming call (ctk_track_stream_seg_*, Tracker.track_stream(..., segments=)): the slab passes through
chunk-sized device buffers, the breaks fall inside chunks, on chunk edges and between chunks shorter than a segment.  The result is
what the one-call entries give with ctk_set_segments: the C oracle on every segment alone, ids shifted (tests/segment_util.py)."""
import importlib

import numpy as np
import pytest

import golden_util
import segment_cases as sc
import segment_util as su
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

CASES = golden_util.case_names()
CHUNKS = (1, 3, 0)                      # one step per chunk, breaks inside and on chunk edges, the default chunk (the whole golden)


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.close()


def stream_array(trk, g, starts, chunk, f64=False, thr="golden"):
    a = g["anom"].astype(np.float64) if f64 else g["anom"]
    ar = sc.args(g)
    return trk.track_stream(a, g["thr"] if thr == "golden" else thr, *ar[1:], chunk_steps=chunk, segments=starts)


def stream_callbacks(trk, g, starts, chunk):
    a = g["anom"]
    out = np.full(a.shape, -7, dtype=np.int32)
    seen = []

    def reader(t0, nt, dst):
        dst[...] = a[t0:t0 + nt]

    def writer(t0, nt, src):
        seen.append((t0, nt))
        out[t0:t0 + nt] = src
    _, n = trk.track_stream(reader, *sc.args(g), sink=writer, shape=a.shape, dtype=a.dtype, chunk_steps=chunk, segments=starts)
    assert [t0 for t0, _ in seen] == sorted(t0 for t0, _ in seen) and sum(nt for _, nt in seen) == a.shape[0]
    return out, n


def check_case(trk, name, chunks=CHUNKS, sinks=("array", "callbacks"), f64=False):
    g = sc.golden(name)
    T = g["anom"].shape[0]
    for sname, starts in su.segmentations(T).items():
        want, nw = sc.expected(name, starts)
        if sname == "one":
            assert np.array_equal(want, g["flag"])
        for chunk in chunks:
            for sink in sinks:
                got, ng = stream_array(trk, g, starts, chunk, f64=f64) if sink == "array" else stream_callbacks(trk, g, starts, chunk)
                where = "{} / {} / chunk {} / {}".format(name, sname, chunk, sink)
                assert np.array_equal(got, want), "{}: flag differs at {} pixels".format(where, int((got != want).sum()))
                assert ng == nw, "{}: n_tracked {} != {}".format(where, ng, nw)


@pytest.mark.parametrize("name", CASES)
def test_goldens_segmented_streaming(trk, name):
    check_case(trk, name)


def test_float64_slab(trk):
    check_case(trk, "f64pole_syn", f64=True)


@pytest.mark.parametrize("mode", ["host_resolver", "dense_rerun", "sync", "seam_caps"])
def test_fallbacks_see_the_same_table(mode):
    """the host resolver, the second pass after the run-table result was refused (the table is built again for it), the synchronous
    device resolver and the host seam driver give what the fused pass gives"""
    t = _native.Tracker(0)
    try:
        if mode == "host_resolver":
            t.set_device_resolve(False)
        elif mode == "dense_rerun":
            t.set_result_transfer(2)
        elif mode == "sync":
            t.set_fused(False)
        else:
            t.debug_set_seam_caps(1, 1)
        for name in ("syn2deg_s0", "chain_b", "busy_s1", "T3"):
            check_case(t, name, chunks=(3,), sinks=("array",) if mode == "dense_rerun" else ("array", "callbacks"))
        if mode == "host_resolver":
            assert t.stats()["host_path"] == 1
        if mode == "dense_rerun":
            assert t.stats()["result_as_runs"] == 0
    finally:
        t.close()


def test_ambiguous_decisions_route(trk):
    """decisions on rounding boundaries send the one-call pass through the time-shard path with a world of one: it sees the call's
    segments too (the f64pole goldens hold such decisions; with breaks some of them may disappear -- the results decide)"""
    for name in ("f64pole_blocky", "f64pole_blocky5"):
        check_case(trk, name, chunks=(3,), sinks=("array",))


def test_threshold_field_with_segments(trk):
    """thr=None (the handle's threshold field) composes with the call's segments, as in the one-call entries"""
    g = sc.golden("syn2deg_s1")
    T, ny, nx = g["anom"].shape
    assert np.all(g["thr"] == g["thr"][0])
    planes = np.broadcast_to(np.float32(g["thr"][0]), (1, ny, nx)).copy()
    starts = np.array([0, 7, 30, 31, 60])
    want, nw = sc.expected("syn2deg_s1", starts)
    trk.set_threshold_field(planes, np.zeros(T, dtype=np.int32))
    try:
        for chunk in (5, 0):
            got, ng = stream_array(trk, g, starts, chunk, thr=None)
            assert np.array_equal(got, want) and ng == nw
    finally:
        trk.clear_threshold_field()


def test_one_segment_is_the_unsegmented_call(trk):
    """segments=[0] and no segments at all: the unsegmented result from the unsegmented kernel builds"""
    g = sc.golden("syn2deg_s0")
    ref, nref = trk.track_stream(g["anom"], *sc.args(g), chunk_steps=7)
    st_ref = trk.stats()
    for starts in ([0], []):
        got, n = trk.track_stream(g["anom"], *sc.args(g), chunk_steps=7, segments=starts)
        st = trk.stats()
        assert np.array_equal(got, ref) and n == nref and np.array_equal(got, g["flag"])
        assert st["overlap_form"] == st_ref["overlap_form"] < 1000000 and st["filter_forms"] == st_ref["filter_forms"]
    got, n = trk.track_stream(g["anom"], *sc.args(g), chunk_steps=7, segments=[0, 20])
    st = trk.stats()
    assert st["overlap_form"] == st_ref["overlap_form"] + 1000000 and st["filter_forms"] != st_ref["filter_forms"]
    got, n = trk.track_stream(g["anom"], *sc.args(g), chunk_steps=7)          # nothing of the call's segments stays on the handle
    assert np.array_equal(got, g["flag"]) and trk.stats()["overlap_form"] == st_ref["overlap_form"]


def test_track_numpy_chunk_steps_with_segments():
    g = sc.golden("chain_a")
    starts = np.array([0, 17, 18, 90])
    want, nw = sc.expected("chain_a", starts)
    got, n = cm.track_numpy(g["anom"], g["wrow"], g["thr"], g["gorl"], g["overlap"], g["persistence"], g["twosided"], segments=starts, chunk_steps=16)
    assert np.array_equal(got, want) and n == nw
    got, n = cm.track_numpy(g["anom"], g["wrow"], g["thr"], g["gorl"], g["overlap"], g["persistence"], g["twosided"], chunk_steps=16)
    assert np.array_equal(got, g["flag"])


def test_refusals(trk):
    g = sc.golden("T3")
    a = g["anom"]
    T = a.shape[0]
    for bad in ([1, 2], [0, 2, 2], [0, 2, 1], [0, -1], [0, T], [0, 1, T + 4]):
        with pytest.raises(ValueError, match="segment"):
            trk.track_stream(a, *sc.args(g), segments=bad)
    with pytest.raises(ValueError):
        trk.track_stream(a, *sc.args(g), segments=[[0, 1]])
    trk.set_segments([0, 1])                               # sticky segments and the call's own: refused
    try:
        with pytest.raises(ValueError, match="segments"):
            trk.track_stream(a, *sc.args(g), segments=[0, 2])
        with pytest.raises(ValueError, match="segments"):
            trk.track_stream(a, *sc.args(g), segments=[0])
    finally:
        trk.clear_segments()
    flag, n = trk.track_stream(a, *sc.args(g), segments=[0, 2])          # the handle is fine afterwards
    want, nw = sc.expected("T3", [0, 2])
    assert np.array_equal(flag, want) and n == nw
