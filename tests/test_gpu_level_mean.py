"""The vertical mean over the selected levels on the GPU (ctk_level_mean_*: README.rst:235-240 of the reference, "vertically averaged
between 500-150 hPa") against its numpy statement tests/level_util.py, by bit pattern, NaN positions included (level_util.same_bits:
equal dtype and shape, NaN at the same places, equal uint32 / uint64 views everywhere else).  That is looser than a plain integer view
in one respect only: the sign and payload of a NaN are not compared, because IEEE 754 leaves them open and the host and the device
differ there (0 / 0 is 0xfff8... on an x86 host, 0x7ff8... on the device).
The float64 cases pin the order of the sum and the separate multiply and add (tests/test_level_mean_host.py shows that the oracle
sees both), the float32 cases indexing, conversion and NaN handling."""
import ctypes as C

import numpy as np
import pytest

import level_util as lu
from contrack_amd import _native
from contrack_amd.contrack import level_mean_numpy

pytestmark = pytest.mark.gpu

VECTOR, SCALAR = 1, 0              # Tracker.debug_level_form


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


@pytest.fixture(scope="module")
def cases():
    """the 7 x 15 x 9 x 65 fields with the pinned trapezoid weights and random weights on the same levels, some NaNs on selected
    levels, NaN on every unselected one; the oracle's answers, computed once: {(dtype name, weights, skipna): (x, w, want)}"""
    out = {}
    for dtype in (np.float32, np.float64):
        x = lu.field(dtype, seed=11)
        x[:, lu.PINNED_WEIGHTS == 0] = np.nan
        x[2, 5, 3, 7] = np.nan
        x[4, 3:13, 8, 64] = np.nan
        for wname, w in (("pinned", lu.PINNED_WEIGHTS), ("random", lu.random_weights_on(lu.PINNED_WEIGHTS))):
            for skipna in (0, 1):
                x.flags.writeable = False
                out[(np.dtype(dtype).name, wname, skipna)] = (x, w, lu.level_mean(x, w, skipna=bool(skipna)))
    return out


# ---- forms ------------------------------------------------------------------------------------------------------------------------
def test_forms(trk):
    seen = set()
    for (ny, nx), dtype, skipna in [(g, d, s) for g in ((1, 1), (2, 2), (2, 3), (8, 8), (9, 65)) for d in (np.float32, np.float64) for s in (0, 1)]:
        x = lu.field(dtype, steps=5, nlev=6, ny=ny, nx=nx, seed=ny * nx)
        x[1, 2].flat[0] = np.nan
        w = np.array([0.0, 1.5, 2.0, 0.25, 0.0, 3.0])
        got = trk.level_mean(x, w, skipna=bool(skipna))
        form = trk.debug_level_form()
        assert form == lu.plan(x.itemsize, 4, ny * nx, 5, True)["vec"], (ny, nx, dtype, form)
        seen.add((np.dtype(dtype).name, form))
        assert lu.same_bits(got, lu.level_mean(x, w, skipna=bool(skipna))), (ny, nx, dtype, skipna)
    assert seen == {(d, f) for d in ("float32", "float64") for f in (VECTOR, SCALAR)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dev_entry_and_offset_pointers(trk, dtype):
    """x_dev and out_dev each one element past a 16-byte boundary: the scalar form, the same bits; unselected levels skipped in place"""
    steps, nlev, ny, nx = 5, 6, 8, 8
    x = lu.field(dtype, steps=steps, nlev=nlev, ny=ny, nx=nx, seed=3)
    w = np.array([0.0, 1.5, 2.0, 0.25, 0.0, 3.0])
    want = lu.level_mean(x, w)
    es = x.itemsize
    d_x, d_o = trk.malloc(x.nbytes + 16), trk.malloc(want.nbytes + 16)
    try:
        for off, form in ((0, VECTOR), (es, SCALAR)):
            px, po = C.c_void_p(d_x.value + off), C.c_void_p(d_o.value + off)
            trk.h2d(px, x)
            trk.level_mean_dev(px, steps, nlev, ny, nx, w, po, f64=dtype == np.float64)
            assert trk.debug_level_form() == form
            got = np.empty_like(want)
            trk.d2h(got, po)
            assert lu.same_bits(got, want), off
    finally:
        trk.free(d_x)
        trk.free(d_o)


# ---- level loop: every remainder of the unrolled batches -----------------------------------------------------------------------------
def test_every_number_of_selected_levels(trk):
    rng = np.random.default_rng(5)
    x = lu.field(np.float64, steps=3, nlev=17, ny=3, nx=5, seed=17)
    for K in range(1, 18):
        w = np.zeros(17)
        w[np.sort(rng.choice(17, K, replace=False))] = rng.random(K) + 0.5
        assert lu.same_bits(trk.level_mean(x, w), lu.level_mean(x, w)), K


# ---- selection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(d, w, s) for d in ("float32", "float64") for w in ("pinned", "random") for s in (0, 1)], ids=str)
def test_selection_and_nan(trk, cases, key):
    """unselected levels on both sides, filled with NaN, do not show; a NaN on one and on ten selected levels with both skipna"""
    x, w, want = cases[key]
    assert np.isnan(want[2, 3, 7]) == (key[2] == 0) and np.isnan(want[4, 8, 64])
    assert np.count_nonzero(np.isnan(want)) == (2 if key[2] == 0 else 1)
    assert lu.same_bits(trk.level_mean(x, w, skipna=bool(key[2])), want)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hole_in_the_selected_run_and_infinities(trk, dtype):
    x = lu.field(dtype, steps=4, nlev=15, ny=9, nx=65, seed=2)
    w = lu.PINNED_WEIGHTS.copy()
    w[6] = 0.0                                          # two runs: levels 3-5 and 7-12
    assert lu.runs_of(w) == [(3, 3), (7, 6)]
    x[:, w == 0] = np.nan
    x[0, 4, 0, 0] = np.inf
    x[0, 4, 0, 1], x[0, 8, 0, 1] = np.inf, -np.inf      # inf - inf
    x[1, 9, 2, 2] = -np.inf
    x[1, 9, 2, 3], x[1, 10, 2, 3] = -np.inf, np.nan
    for skipna in (False, True):
        want = lu.level_mean(x, w, skipna=skipna)
        assert want[0, 0, 0] == np.inf and np.isnan(want[0, 0, 1]) and want[1, 2, 2] == -np.inf
        assert np.isnan(want[1, 2, 3]) != skipna
        assert lu.same_bits(trk.level_mean(x, w, skipna=skipna), want), skipna
        assert lu.same_bits(trk.level_mean(x, w, skipna=skipna, chunk_steps=3), want), skipna


# ---- steps ----------------------------------------------------------------------------------------------------------------------------
def test_one_step_and_more_steps_than_a_grid_dimension(trk):
    w = np.array([0.0, 2.0, 0.0, 1.0])
    for steps in (1, 65537):
        x = lu.field(np.float32, steps=steps, nlev=4, ny=3, nx=5, seed=steps)
        want = lu.level_mean(x, w)
        assert lu.same_bits(trk.level_mean(x, w), want), steps
    d_x, d_o = trk.malloc(x.nbytes), trk.malloc(want.nbytes)           # all 65 537 steps in one launch
    try:
        trk.h2d(d_x, x)
        trk.level_mean_dev(d_x, 65537, 4, 3, 5, w, d_o)
        got = np.empty_like(want)
        trk.d2h(got, d_o)
        assert lu.same_bits(got, want)
    finally:
        trk.free(d_x)
        trk.free(d_o)


def test_workgroup_to_xcd_mappings_give_the_same_bits(trk, cases):
    """launch order, eighths and tiles (the remainders that stay where they are included: 65 537 workgroups, 3 per step x 7)"""
    x, w, want = cases[("float64", "random", 1)]
    big = lu.field(np.float32, steps=65537, nlev=2, ny=3, nx=5, seed=4)
    want_big = lu.level_mean(big, [1.0, 3.0])
    assert _native.level_plan(4, 2, 15, 65537, 1)["xcd"] == 1 and _native.level_plan(8, 9, 585, 7, 1)["blocks"] == 21
    try:
        for mode in (0, 1, 2, 16):
            trk.debug_set_level(mode)
            assert lu.same_bits(trk.level_mean(x, w, skipna=True), want), mode
            assert lu.same_bits(trk.level_mean(big, [1.0, 3.0]), want_big), mode
    finally:
        trk.debug_set_level()


def test_stride_loop_with_fewer_workgroups_than_work(trk, cases):
    """a launch of fewer workgroups than (step, part of the plane) pairs, in launch order and with every XCD mapping, the library's rule
    included: 21 pairs on 1, 5, 8 and 20 workgroups, 65 537 pairs on 1000 and 4099"""
    x, w, want = cases[("float64", "random", 1)]
    big = lu.field(np.float32, steps=65537, nlev=2, ny=3, nx=5, seed=4)
    want_big = lu.level_mean(big, [1.0, 3.0])
    try:
        for mode in (-1, 0, 1, 2):
            for cap in (1, 5, 8, 20):
                trk.debug_set_level(mode, cap)
                assert lu.same_bits(trk.level_mean(x, w, skipna=True), want), (mode, cap)
                assert trk.debug_level_launch() == (0, cap)
            for cap in (1000, 4099):
                trk.debug_set_level(mode, cap)
                assert lu.same_bits(trk.level_mean(big, [1.0, 3.0]), want_big), (mode, cap)
                assert trk.debug_level_launch() == (0, cap)
    finally:
        trk.debug_set_level()


def test_more_work_than_a_launch_may_have_workgroups(trk):
    """2^24 + 1 steps of one pixel: one workgroup each, 2^24 - 1 of them launched (a launch stays below 2^32 work-items), the last two
    pairs are reached by the stride; 67 MB in, one chunk, one launch"""
    steps = (1 << 24) + 1
    x = np.random.default_rng(3).standard_normal((steps, 1, 1, 1), dtype=np.float32)
    assert _native.level_plan(4, 1, 1, steps, 1)["grid"] == (1 << 24) - 1
    got = trk.level_mean(x, [2.0])
    assert trk.debug_level_launch() == (0, (1 << 24) - 1)
    assert lu.same_bits(got, lu.level_mean(x, [2.0])) and lu.same_bits(got[-3:], x[-3:, 0])


# ---- streaming ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(d, w, s) for d in ("float32", "float64") for w in ("pinned", "random") for s in (0, 1)], ids=str)
def test_streamed_equals_resident(trk, cases, key, tmp_path):
    x, w, want = cases[key]
    skipna = bool(key[2])
    resident = trk.level_mean(x, w, skipna=skipna)
    assert lu.same_bits(resident, want)
    mm = np.memmap(str(tmp_path / "x.bin"), dtype=x.dtype, mode="w+", shape=x.shape)
    mm[...] = x
    mm.flush()
    sel = np.flatnonzero(w)
    for cs in (1, 2, 3, 7, 8, 0):
        assert lu.same_bits(trk.level_mean(x, w, skipna=skipna, chunk_steps=cs), resident), cs
        assert lu.same_bits(level_mean_numpy(mm, weights=w, skipna=skipna, chunk_steps=cs), resident), cs
        asked, got_chunks = [], []

        def reader(t0, nt, out):
            asked.append((t0, nt, out.shape))
            out[...] = x[t0:t0 + nt][:, sel]

        def writer(t0, nt, values):
            got_chunks.append((t0, values.copy()))
        assert trk.level_mean_cb(reader, (7, len(sel), 9, 65), x.dtype, w[sel], skipna=skipna, sink=writer, chunk_steps=cs) is None
        n = 7 if cs in (0, 8) else cs
        assert asked == [(t0, min(n, 7 - t0), (min(n, 7 - t0), len(sel), 9, 65)) for t0 in range(0, 7, n)], cs      # only ever (nt, K, ny, nx)
        assert [t0 for t0, _ in got_chunks] == [a[0] for a in asked]
        assert lu.same_bits(np.concatenate([v for _, v in got_chunks]), resident), cs
        out = level_mean_numpy(reader, weights=w[sel], skipna=skipna, chunk_steps=cs, shape=(7, len(sel), 9, 65), dtype=x.dtype)
        assert lu.same_bits(out, resident), cs


def test_reader_that_gives_up_and_argument_errors_leave_the_handle_usable(trk, cases):
    x, w, want = cases[("float32", "pinned", 0)]
    sel = np.flatnonzero(w)
    calls = []

    def reader(t0, nt, out):
        calls.append(t0)
        if len(calls) == 2:
            raise RuntimeError("no more data")
        out[...] = x[t0:t0 + nt][:, sel]
    with pytest.raises(RuntimeError, match="no more data"):
        trk.level_mean_cb(reader, (7, len(sel), 9, 65), np.float32, w[sel], chunk_steps=2)
    assert calls == [0, 2]
    L, h = _native.lib(), trk.handle
    give_up = _native.READ_CHUNK_FN(lambda user, t0, nt, dst: 1 if t0 else 0)
    wv, out = w[sel].copy(), np.empty((7, 9, 65), dtype=np.float32)
    no_writer = C.cast(None, _native.WRITE_CHUNK_FN)
    assert L.ctk_level_mean_stream_cb(h, 4, 7, len(sel), 9, 65, give_up, None, wv.ctypes.data, 0, no_writer, None, 2, 1) == -1      # CTK_E_INVALID
    assert b"reader returned 1" in L.ctk_last_error()
    assert trk.resident_level_mean() is None
    bad = w.copy()
    bad[4] = -1.0
    for args in ((None, 7, 15, 9, 65, w.ctypes.data, 0, out.ctypes.data, 0), (x.ctypes.data, 0, 15, 9, 65, w.ctypes.data, 0, out.ctypes.data, 0),
                 (x.ctypes.data, 7, 15, 9, 65, None, 0, out.ctypes.data, 0), (x.ctypes.data, 7, 15, 9, 65, bad.ctypes.data, 0, out.ctypes.data, 0),
                 (x.ctypes.data, 7, 15, 9, 65, np.zeros(15).ctypes.data, 0, out.ctypes.data, 0), (x.ctypes.data, 7, 15, 9, 65, w.ctypes.data, 0, None, 0)):
        assert L.ctk_level_mean_f32(h, *args) == -1 and L.ctk_last_error()
    assert L.ctk_level_mean_stream_f32(h, x.ctypes.data, 7, 15, 9, 65, w.ctypes.data, 0, out.ctypes.data, -1, 0) == -1
    many = np.ones(4097)
    assert L.ctk_level_mean_f32(h, x.ctypes.data, 1, 4097, 1, 1, many.ctypes.data, 0, out.ctypes.data, 0) == -1 and b"4097 selected" in L.ctk_last_error()
    assert lu.same_bits(trk.level_mean(x, w), want)                           # the handle works


def test_writer_that_gives_up_leaves_nothing_resident_and_the_handle_usable(trk, cases):
    """four chunks of 2, 2, 2 and 1 steps (both buffers reused once); the writer fails on the second"""
    x, w, want = cases[("float32", "pinned", 0)]
    sel = np.flatnonzero(w)

    def reader(t0, nt, out):
        out[...] = x[t0:t0 + nt][:, sel]
    for keep in (False, True):
        seen = []

        def writer(t0, nt, values):
            seen.append(t0)
            if len(seen) == 2:
                raise RuntimeError("disk full")
        with pytest.raises(RuntimeError, match="disk full"):
            trk.level_mean_cb(reader, (7, len(sel), 9, 65), np.float32, w[sel], sink=writer, chunk_steps=2, keep_resident=keep)
        assert seen == [0, 2], keep
        assert trk.resident_level_mean() is None
    L, h = _native.lib(), trk.handle
    tr = _native._Trampolines()
    fill = tr.reader(reader, C.c_float, (len(sel), 9, 65))
    give_up = _native.WRITE_CHUNK_FN(lambda user, t0, nt, src: 1 if t0 else 0)
    wv = w[sel].copy()
    for keep in (0, 1):
        assert L.ctk_level_mean_stream_cb(h, 4, 7, len(sel), 9, 65, fill, None, wv.ctypes.data, 0, give_up, None, 2, keep) == -1      # CTK_E_INVALID
        err = L.ctk_last_error()
        assert b"ctk_level_mean_stream_cb" in err and b"writer returned 1" in err, err
        assert trk.resident_level_mean() is None
    assert not tr.errors
    assert lu.same_bits(trk.level_mean(x, w), want)                           # the handle works


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_writer_together_with_keep_resident(trk, cases, dtype):
    """the kernel writes the resident mean, and the writer gets every chunk from there through the pinned output chunks"""
    x, w, want = cases[(dtype, "pinned", 1)]
    sel = np.flatnonzero(w)
    asked, chunks = [], []

    def reader(t0, nt, out):
        asked.append(t0)
        out[...] = x[t0:t0 + nt][:, sel]

    def writer(t0, nt, values):
        chunks.append((t0, values.copy()))
    assert trk.level_mean_cb(reader, (7, len(sel), 9, 65), x.dtype, w[sel], skipna=True, sink=writer, chunk_steps=2, keep_resident=True) is None
    assert asked == [0, 2, 4, 6] and [t0 for t0, _ in chunks] == asked
    assert lu.same_bits(np.concatenate([v for _, v in chunks]), want)
    assert trk.resident_level_mean() == (7, 9, 65, dtype == "float64")
    group = np.arange(7, dtype=np.int32)                                      # own group per step, climatology 0: the anomaly is the mean itself
    zero = np.zeros((7, 9, 65), dtype=x.dtype)
    assert lu.same_bits(trk.anomalies_resident(group, 7, clim=zero)[0], trk.anomalies(want, group, 7, clim=zero)[0])
    assert lu.same_bits(trk.anomalies_resident(group, 7, clim=zero)[0], want - zero)
    group, G = (np.arange(7) % 3).astype(np.int32), 3
    ref = trk.anomalies(want, group, G, window=1, smooth=2, want_clim=True, segments=[0, 3])
    got = trk.anomalies_resident(group, G, window=1, smooth=2, want_clim=True, segments=[0, 3])
    assert lu.same_bits(got[0], ref[0]) and lu.same_bits(got[1], ref[1])


def test_1024_selected_levels(trk):
    x = lu.field(np.float64, steps=2, nlev=1030, ny=2, nx=3, seed=9)
    w = np.random.default_rng(1).random(1030) + 0.5
    w[[0, 500, 501, 777, 1000, 1029]] = 0.0
    assert lu.same_bits(trk.level_mean(x, w), lu.level_mean(x, w))


# ---- the resident chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_resident_chain(trk, cases, dtype):
    x, w, want = cases[(dtype, "pinned", 1)]
    group, G = (np.arange(7) % 3).astype(np.int32), 3
    g0 = trk.resident_level_mean_generation()
    assert trk.level_mean(x, w, skipna=True, keep_resident=True, want_out=False) is None
    assert trk.resident_level_mean() == (7, 9, 65, dtype == "float64")
    g1 = trk.resident_level_mean_generation()
    assert g1 != g0
    for smooth in (1, 2):
        for segments in (None, [0, 3]):
            ref = trk.anomalies(want, group, G, window=1, smooth=smooth, want_clim=True, segments=segments)
            got = trk.anomalies_resident(group, G, window=1, smooth=smooth, want_clim=True, segments=segments)
            assert lu.same_bits(got[0], ref[0]) and lu.same_bits(got[1], ref[1]), (smooth, segments)
    assert trk.resident_level_mean_generation() == g1                          # anomalies leave the mean alone
    host = trk.level_mean(x, w, skipna=True, keep_resident=True)              # a second call: another slab
    assert lu.same_bits(host, want) and trk.resident_level_mean_generation() != g1
    trk.release_io()
    assert trk.resident_level_mean() is None and trk.resident_level_mean_generation() != g1
    with pytest.raises(ValueError, match="no vertical mean is resident"):
        _native.check(_native.lib().ctk_anom_seg_resident(trk.handle, group.ctypes.data, G, 1, 1, None, host.ctypes.data, None, 0, None, 0))
    with pytest.raises(_native.ContrackHipError):
        trk.anomalies_resident(group, G)
