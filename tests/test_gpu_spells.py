"""Blocked spells per grid point on the device (ctk_spells*, k_spell): events, steps and longest exactly equal to the numpy statement
of the definition (spell_util), whatever the slice length, the chunk length and the place of the segment breaks."""
import ctypes as C
import importlib

import numpy as np
import pytest

import freq_util
import golden_util
import spell_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 31, 60), (57, 1, 130), (57, 33, 1), (67, 17, 64), (203, 9, 65), (131, 20, 36)]
SERIES = (0, 3, 3, 0, 3, 5, 5, 0)
KNOWN = (((1, 1, None), (3, 5, 2)),
         ((0, 1, None), (2, 5, 3)),
         ((1, 2, None), (2, 4, 2)),
         ((1, 1, (0, 2)), (4, 5, 2)))


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


_flags, _lists = {}, {}


def _flag(shape):
    """the generated slab of a shape (made once)"""
    if shape not in _flags:
        _flags[shape] = spell_util.spell_flags(*shape, seed=sum(shape))
        _flags[shape].setflags(write=False)
    return _flags[shape]


def _want(key, flag, ids, G, above, by_id, min_duration, segments=None):
    """spell_util's maps; the walk over the slab is shared by the calls that differ only in grouping and min_duration"""
    k = (key, above, bool(by_id), None if segments is None else tuple(int(s) for s in segments))
    if k not in _lists:
        _lists[k] = spell_util.spell_list(flag, above, bool(by_id), segments)
    return spell_util.maps_of(_lists[k], flag.shape, ids, G, min_duration)


def _same(got, want, tag):
    assert len(got) == 3
    for g, w, what in zip(got, want, ("events", "steps", "longest")):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, tag)
        assert np.array_equal(g.astype(np.int64), w), (what, tag)


@pytest.mark.parametrize("args,want", KNOWN)
def test_known_answers(trk, args, want):
    by_id, min_duration, segments = args
    flag = np.array(SERIES, dtype=np.int32).reshape(8, 1, 1)
    _same(trk.spells(flag, by_id=by_id, min_duration=min_duration, segments=segments),
          spell_util.spells(flag, None, 1, 0, by_id, min_duration, segments), args)
    base, ptr = _on_device(trk, flag)
    try:
        for got in (trk.spells(flag, by_id=by_id, min_duration=min_duration, segments=segments),
                    trk.spells(flag, by_id=by_id, min_duration=min_duration, segments=segments, chunk_steps=3),
                    trk.spells_dev(ptr, 8, 1, 1, by_id=by_id, min_duration=min_duration, segments=segments)):
            assert tuple(int(a[0, 0, 0]) for a in got) == want, args
    finally:
        trk.free(base)


@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(trk, shape):
    flag = _flag(shape)
    for gname, ids, G in freq_util.groupings(shape[0]):
        for by_id in (True, False):
            for min_duration in (1, 2, 5):
                for above in (0, 2):
                    tag = (shape, gname, by_id, min_duration, above)
                    _same(trk.spells(flag, ids, G, above, by_id, min_duration), _want(shape, flag, ids, G, above, by_id, min_duration), tag)


@pytest.mark.parametrize("shape", [(67, 17, 64), (57, 1, 130)])
def test_slice_and_chunk_lengths(trk, shape):
    """every forced slice length and the rule, crossed with every chunk length: the same arrays (slice 1 with chunk 1 makes every
    spell cross every kind of edge); the resident entry under the same slices"""
    flag = _flag(shape)
    T, ny, nx = shape
    _, ids, G = freq_util.groupings(T)[2]
    segments = [0, 20, 21, 40]
    base, ptr = _on_device(trk, flag)
    try:
        for by_id in (True, False):
            want = _want(shape, flag, ids, G, 0, by_id, 2, segments)
            for sl in (1, 2, 7, 8, 64, 0):
                trk.set_spell_debug(sl)
                for chunk in (0, 1, 5, T):
                    _same(trk.spells(flag, ids, G, 0, by_id, 2, segments, chunk_steps=chunk), want, (shape, by_id, sl, chunk))
                _same(trk.spells_dev(ptr, T, ny, nx, ids, G, 0, by_id, 2, segments), want, (shape, by_id, sl, "dev"))
    finally:
        trk.set_spell_debug(0)
        trk.free(base)


def test_segment_starts_on_and_beside_the_edges(trk):
    """slices of 8 steps in chunks of 20: a segment start exactly on a slice edge (16, 28), on a chunk edge (20, 40), one step on
    either side of each, and at the last step; on generated flags and on an all-flagged slab, where the breaks alone make the spells"""
    shape = (67, 17, 64)
    T = shape[0]
    flag = _flag(shape)
    solid = np.full(shape, 4, dtype=np.int32)
    _, ids, G = freq_util.groupings(T)[1]
    sets = [[0, e + d] for e in (16, 20, 28, 40) for d in (-1, 0, 1)] + [[0, T - 1], [0, 15, 16, 17, 19, 20, 21, 27, 28, 29, 39, 40, 41, T - 1]]
    try:
        trk.set_spell_debug(8)
        for segments in sets:
            for by_id in (True, False):
                want = spell_util.spells(flag, ids, G, 0, by_id, 1, segments)
                _same(trk.spells(flag, ids, G, 0, by_id, 1, segments, chunk_steps=20), want, (segments, by_id))
            ev, st, lg = trk.spells(solid, segments=segments, chunk_steps=20)
            lens = np.diff(np.array(list(segments) + [T]))
            assert (ev == len(segments)).all() and (st == T).all() and (lg == lens.max()).all(), segments
            ev, st, lg = trk.spells(solid, segments=segments, chunk_steps=20, min_duration=3)
            assert (ev == (lens >= 3).sum()).all() and (st == lens[lens >= 3].sum()).all(), segments
    finally:
        trk.set_spell_debug(0)


def test_one_spell_through_every_slice_and_chunk(trk):
    T, ny, nx = 203, 9, 65
    solid = np.full((T, ny, nx), 7, dtype=np.int32)
    _, ids, G = freq_util.groupings(T)[2]
    try:
        for sl in (0, 8):
            trk.set_spell_debug(sl)
            for chunk in (0, 5, 64):
                ev, st, lg = trk.spells(solid, chunk_steps=chunk)
                assert ev.shape == (1, ny, nx) and (ev == 1).all() and (st == T).all() and (lg == T).all(), (sl, chunk)
                ev, st, lg = trk.spells(solid, ids, G, chunk_steps=chunk)                     # the whole spell in the group of step 0
                g0 = int(ids[0])
                assert (ev[g0] == 1).all() and (st[g0] == T).all() and (lg[g0] == T).all() and ev.sum() == ny * nx and st.sum() == T * ny * nx, (sl, chunk)
                for maps in (trk.spells(solid, above=7, chunk_steps=chunk), trk.spells(solid, min_duration=T + 1, chunk_steps=chunk)):
                    assert all(not m.any() for m in maps), (sl, chunk)
                ev, st, lg = trk.spells(solid, min_duration=T, chunk_steps=chunk)
                assert (ev == 1).all() and (lg == T).all(), (sl, chunk)
    finally:
        trk.set_spell_debug(0)


@pytest.mark.parametrize("shape", [(67, 17, 64), (203, 9, 65)])
def test_misaligned_device_pointer(trk, shape):
    """4 bytes into the allocation: the general-load path on a plane the 16-byte loads would otherwise take"""
    flag = _flag(shape)
    T, ny, nx = shape
    _, ids, G = freq_util.groupings(T)[2]
    for off in (4, 0):
        base, ptr = _on_device(trk, flag, off)
        try:
            for by_id in (True, False):
                _same(trk.spells_dev(ptr, T, ny, nx, ids, G, 0, by_id, 2), _want(shape, flag, ids, G, 0, by_id, 2), (shape, off, by_id))
        finally:
            trk.free(base)


@pytest.mark.parametrize("name", golden_util.case_names())
def test_golden_flags(trk, name):
    """on tracked flags: with min_duration = 1 the steps summed over the groups are the frequency counts of the existing entry;
    spells_numpy equals spell_util grouped, ungrouped and from a reader"""
    flag = golden_util.load(name)["flag"]
    T = flag.shape[0]
    _, ids, G = freq_util.groupings(T)[2]
    G = int(ids.max()) + 1                                                  # (spells_numpy: G = the largest id + 1)
    for by_id in (True, False):
        for above in (0, 1):
            ev, st, lg = trk.spells(flag, ids, G, above, by_id, 1)
            assert np.array_equal(st.sum(axis=0, dtype=np.int64), trk.frequency(flag, None, 1, above)[0]), (name, by_id, above)
        want = _want(name, flag, ids, G, 0, by_id, 2)
        got = cm.spells_numpy(flag, ids, by_id=by_id, min_duration=2)
        flat = cm.spells_numpy(flag, by_id=by_id, min_duration=2)
        calls = []

        def reader(t0, nt, out):
            calls.append((t0, nt))
            out[...] = flag[t0:t0 + nt]
        read = cm.spells_numpy(reader, ids, by_id=by_id, min_duration=2, chunk_steps=7, shape=flag.shape)
        assert calls == [(t0, min(7, T - t0)) for t0 in range(0, T, 7)]
        want_flat = _want(name, flag, None, 1, 0, by_id, 2)
        for k in range(3):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (name, by_id, k)
            assert read[k].dtype == np.int64 and np.array_equal(read[k], want[k]), (name, by_id, k)
            assert flat[k].shape == flag.shape[1:] and np.array_equal(flat[k], want_flat[k][0]), (name, by_id, k)


def test_wide_integer_flags(trk):
    flag = _flag((57, 1, 130))
    want = spell_util.spells(flag)
    for dt in (np.int64, np.uint32, np.int16, np.uint8):
        got = cm.spells_numpy(flag.astype(dt))
        assert all(np.array_equal(g, w[0]) for g, w in zip(got, want)), dt
    big = flag.astype(np.int64)
    big[20, 0, 4] = 2 ** 31
    with pytest.raises(ValueError, match="int32"):
        cm.spells_numpy(big)


def test_library_refusals_name_the_value(trk):
    """the C entries check for themselves what the Python wrappers check before them: CTK_E_INVALID and a message with the value"""
    L = _native.lib()
    flag = np.zeros((8, 2, 3), dtype=np.int32)
    out = np.zeros((3, 2, 2, 3), dtype=np.uint32)
    ids = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int32)

    def call(h=None, T=8, ny=2, nx=3, group=ids, G=2, seg=None, by_id=1, md=1, ev=out[0].ctypes.data, chunk=0):
        st = None if seg is None else np.array(seg, dtype=np.int64)
        rc = L.ctk_spells(trk._h if h is None else h, flag.ctypes.data, T, ny, nx, None if group is None else group.ctypes.data, G,
                          None if st is None else st.ctypes.data, 0 if st is None else len(st), 0, by_id, md, ev, out[1].ctypes.data, out[2].ctypes.data, chunk)
        return rc, L.ctk_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(md=0), "min_duration=0"), (dict(by_id=2), "by_id=2"), (dict(T=0), "T=0"), (dict(nx=0), "nx=0"), (dict(T=2 ** 32), "T=4294967296"),
                     (dict(G=1), "group[1] = 1"), (dict(group=None), "ngroups=2"), (dict(G=0), "ngroups=0"), (dict(seg=[1, 3]), "starts[0] = 1"),
                     (dict(seg=[0, 3, 3]), "starts[2] = 3"), (dict(seg=[0, 8]), "starts at step 8, the slab has 8 steps"), (dict(ev=None), "null buffer"), (dict(chunk=-2), "chunk_steps=-2")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert L.ctk_spells(None, flag.ctypes.data, 8, 2, 3, None, 1, None, 0, 0, 1, 1, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 0) == -1
    assert "null handle" in L.ctk_last_error().decode()
    base, ptr = _on_device(trk, flag)
    try:
        with pytest.raises(ValueError):
            trk.spells_dev(ptr, 8, 2, 3, min_duration=0)
        with pytest.raises(ValueError):
            trk.spells_dev(ptr, 8, 2, 3, segments=[0, 9])
        assert L.ctk_spells_dev(trk._h, ptr, 8, 2, 3, None, 1, None, 0, 0, 1, 1, None, None, None) == -1
        assert L.ctk_spells_cb(trk._h, 8, 2, 3, _native.READ_CHUNK_FN(), None, None, 1, None, 0, 0, 1, 1, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 0) == -1
        # the handle still works after the refusals
        assert all(not m.any() for m in trk.spells_dev(ptr, 8, 2, 3))
    finally:
        trk.free(base)
