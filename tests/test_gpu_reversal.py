"""The gradient-reversal blocking index on the GPU (ctk_reversal_*) against its numpy statement tests/reversal_util.py, by bit pattern
(level_util.same_bits: equal dtype and shape, NaN at the same places, equal integer views everywhere else -- the index itself is never
NaN).  Every comparison on a fixture field first asserts that between 5 % and 50 % of the statement's active band is blocked: an
all-zero output cannot pass.  tests/test_reversal_host.py shows that the statement sees a float32 subtraction and a division by delta."""
import ctypes as C

import numpy as np
import pytest

import reversal_util as ru
from contrack_amd import _native
from contrack_amd.contrack import reversal_numpy, row_weights, track_numpy

pytestmark = pytest.mark.gpu

VECTOR, SCALAR = 1, 0              # Tracker.debug_reversal_form
STEP = {25: 7.5, 37: 5.0, 73: 2.5}


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def blocked(want, tab):
    return 0.05 <= ru.blocked_share(want, tab["eq"]) <= 0.5


def on_device(trk, z, tab, mask=False, off=0):
    """the _dev entry on a copy of z that starts `off` bytes past a 16-byte boundary (the output too)"""
    d_x, d_o = trk.malloc(z.nbytes + 16), trk.malloc(z.nbytes + 16)
    try:
        px, po = C.c_void_p(d_x.value + off), C.c_void_p(d_o.value + off)
        trk.h2d(px, z)
        trk.reversal_dev(px, z.shape[0], z.shape[1], z.shape[2], tab, po, mask=mask, f64=z.dtype == np.float64)
        got = np.empty_like(z)
        trk.d2h(got, po)
        return got
    finally:
        trk.free(d_x)
        trk.free(d_o)


# ---- forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_forms(trk, dtype):
    seen = set()
    for ny, nx in ((25, 1), (25, 3), (25, 8), (37, 65), (73, 8)):
        lat = ru.grid(STEP[ny])
        z = ru.field(lat, nx, steps=6, seed=ny + nx, dtype=dtype)
        for ghgs2 in (None, -5.0):
            tab = ru.table(lat, ghgs2=ghgs2)
            for stat in ("gradient", "mask"):
                want = ru.from_table(z, tab, mask=stat == "mask")
                assert blocked(want, tab), (ny, nx, ghgs2, stat)
                got = trk.reversal(z, tab, mask=stat == "mask")
                form = trk.debug_reversal_form()
                assert form == ru.plan(z.itemsize, ny, nx, 6, True)["vec"], (ny, nx, form)
                seen.add(form)
                assert ru.same_bits(got, want), (ny, nx, ghgs2, stat)
                assert ru.same_bits(reversal_numpy(z, lat, ghgs2=ghgs2, stat=stat), want), (ny, nx, ghgs2, stat)
    assert seen == {VECTOR, SCALAR}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_dev_entry_and_offset_pointers(trk, dtype):
    """x_dev and out_dev each one element past a 16-byte boundary: the scalar form, the same bits"""
    lat = ru.grid(2.5)
    z = ru.field(lat, 8, steps=5, seed=4, dtype=dtype)
    for ghgs2 in (None, -5.0):
        tab = ru.table(lat, ghgs2=ghgs2)
        want = ru.from_table(z, tab)
        assert blocked(want, tab)
        for off, form in ((0, VECTOR), (z.itemsize, SCALAR)):
            got = on_device(trk, z, tab, off=off)
            assert trk.debug_reversal_form() == form
            assert ru.same_bits(got, want), (ghgs2, off)


def test_stride_loop_and_workgroup_to_xcd_mappings(trk):
    """fewer workgroups than (step, part of the plane) pairs and every XCD mapping: 60 pairs of the scalar form, 18 of the vector form,
    and 4099 one-workgroup steps of a regional grid, where the library's own rule maps eighths (3 workgroups stay where they are)"""
    lat = ru.grid(5.0)
    cases = [(ru.field(lat, 65, steps=6, seed=1), ru.table(lat, ghgs2=-5.0)), (ru.field(ru.grid(2.5), 24, steps=9, seed=2), ru.table(ru.grid(2.5)))]
    reg = np.arange(60.0, 29.0, -7.5)                                            # 60N .. 30N: only 45N has both partners
    cases.append((ru.field(reg, 4, steps=4099, seed=3), ru.table(reg)))
    wants = [ru.from_table(z, tab) for z, tab in cases]
    assert _native.reversal_plan(4, 37, 65, 6)["blocks"] == 60 and _native.reversal_plan(4, 73, 24, 9)["blocks"] == 18
    assert _native.reversal_plan(4, 5, 4, 4099) == dict(vec=1, vpt=4, bps=1, blocks=4099, grid=4099, xcd=1)
    assert np.count_nonzero(wants[2]) > 100
    try:
        for mode in (-1, 0, 1, 2):
            for cap in (0, 1, 5, 1000):
                trk.debug_set_reversal(mode, cap)
                for (z, tab), want in zip(cases, wants):
                    assert ru.same_bits(trk.reversal(z, tab), want), (mode, cap, z.shape)
                if cap:
                    assert trk.debug_reversal_launch() == (VECTOR, min(cap, 4099))
    finally:
        trk.debug_set_reversal()


# ---- rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hemisphere", ["both", "north", "south"])
def test_rising_and_falling_latitude_and_hemispheres(trk, hemisphere):
    for rising in (False, True):
        lat = ru.grid(5.0, rising=rising)
        z = ru.field(lat, 8, steps=5, seed=7 + rising)
        tab = ru.table(lat, ghgs2=-5.0, hemisphere=hemisphere)
        want = ru.from_table(z, tab)
        act = np.flatnonzero(tab["eq"] >= 0)
        assert blocked(want, tab) and len(act) == (20 if hemisphere == "both" else 10)
        assert np.count_nonzero(want[:, act[0]]) and np.count_nonzero(want[:, act[-1]])          # the first and the last active row
        assert not np.count_nonzero(np.delete(want, act, axis=1))
        assert ru.same_bits(trk.reversal(z, tab), want), rising
        assert ru.same_bits(reversal_numpy(z, lat, ghgs2=-5.0, hemisphere=hemisphere), want), rising


def test_one_active_row_no_active_row_and_an_irregular_grid(trk):
    one = np.arange(60.0, 29.0, -7.5)                                            # ny = 2 k + 1 with k = 2: only the middle row has both partners
    tab = ru.table(one)
    assert tab["eq"].tolist() == [-1, -1, 4, -1, -1] and tab["po"].tolist() == [-1, -1, 0, -1, -1]
    for nx in (3, 8):
        z = ru.field(one, nx, steps=40, seed=nx)
        want = ru.from_table(z, tab)
        assert blocked(want, tab)
        assert ru.same_bits(trk.reversal(z, tab), want) and ru.same_bits(on_device(trk, z, tab), want)
    none = np.arange(60.0, 44.0, -7.5)
    tab = ru.table(none)
    assert np.all(tab["eq"] == -1)
    z = ru.field(none, 8, steps=3)
    for got in (trk.reversal(z, tab), on_device(trk, z, tab), trk.reversal(z, tab, chunk_steps=2)):
        assert got.dtype == np.float32 and got.shape == z.shape and not got.any() and not np.signbit(got).any()
    lat = ru.gaussian()
    for dtype in (np.float32, np.float64):
        z = ru.field(lat, 8, steps=5, seed=9, dtype=dtype)
        for ghgs2 in (None, -5.0):
            tab = ru.table(lat, ghgs2=ghgs2)
            want = ru.from_table(z, tab)
            assert blocked(want, tab)
            assert ru.differing(want, ru.from_table(z, tab, div=15.0)) == np.count_nonzero(want)      # dE is not delta here
            assert ru.same_bits(trk.reversal(z, tab), want) and ru.same_bits(reversal_numpy(z, lat, ghgs2=ghgs2), want)


# ---- values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_nan_inf_limits_and_negative_zero(trk, dtype):
    lat = ru.grid(7.5)                                           # row 4 (60N): eq 6, po 2, eq2 8; row 13 (7.5S) is read by no northern row
    tab = ru.table(lat, ghgs2=-5.0, hemisphere="north")
    assert (tab["eq"][4], tab["po"][4], tab["eq2"][4]) == (6, 2, 8) and 13 not in set(tab["eq"]) | set(tab["po"]) | set(tab["eq2"]) | set(np.flatnonzero(tab["eq"] >= 0))
    z = ru.field(lat, 8, steps=4, seed=5, dtype=dtype)
    z[0, 2, :], z[0, 8, :] = 4000.0, 6000.0                                     # step 0, row 4: every pixel blocked (5000, 6000, 4000 going north from the partner: a reversal; 6000 again further south) ...
    z[0, 4, :], z[0, 6, :] = 6000.0, 5000.0
    plain = ru.from_table(z, tab)
    assert np.all(plain[0, 4] == dtype(1000.0 / 15.0))
    for k, row in enumerate((4, 6, 2, 8)):                       # ... but for a NaN in the own row and in each partner row
        z[0, row, k] = np.nan
    z[:, 13, :] = np.nan                                         # the unread row
    z[0, 4, 4], z[0, 6, 5], z[0, 2, 6] = np.inf, -np.inf, -np.inf
    z[0, 4, 7], z[0, 6, 7] = np.inf, np.inf                      # inf - inf
    z[1, 4, :], z[1, 6, :], z[1, 2, :], z[1, 8, :] = 5500.0, 5000.0, 5000.0, 6000.0
    z[1, 6, 0] = 5500.0                                          # dS == tS == 0: not blocked
    z[1, 6, 1] = np.nextafter(dtype(5500.0), dtype(0))           # the smallest dS > 0
    z[1, 2, 2] = 5350.0                                          # dN == tN == -150: not blocked
    z[1, 2, 3] = np.nextafter(dtype(5350.0), dtype(0))
    z[1, 8, 4] = 5075.0                                          # dS2 == tS2 == -75: not blocked
    z[1, 8, 5] = np.nextafter(dtype(5075.0), dtype(9000))
    want = ru.from_table(z, tab)
    assert not np.isnan(want).any()
    assert want[0, 4, :4].tolist() == [0, 0, 0, 0] and want[0, 4, 4] == np.inf and want[0, 4, 5] == np.inf and want[0, 4, 6] == plain[0, 4, 6] and want[0, 4, 7] == 0
    assert want[1, 4, 0] == 0 and 0 < want[1, 4, 1] < 1e-3 and want[1, 4, 2] == 0 and want[1, 4, 3] > 0 and want[1, 4, 4] == 0 and want[1, 4, 5] > 0
    assert blocked(want, tab)
    for got in (trk.reversal(z, tab), on_device(trk, z, tab), on_device(trk, z, tab, off=z.itemsize)):
        assert ru.same_bits(got, want)
    assert ru.same_bits(trk.reversal(z, tab, mask=True), ru.from_table(z, tab, mask=True))
    neg = ru.table(lat, ghgs=-1.0)                               # a limit below 0 lets dS = -0.0 pass: the gradient is -0.0, an unblocked pixel +0.0
    z[2, 4, :], z[2, 6, :], z[2, 2, :] = -0.0, 0.0, -1000.0
    want = ru.from_table(z, neg)
    assert np.all(want[2, 4] == 0) and np.signbit(want[2, 4]).all() and not np.signbit(want[2, 0]).any()
    assert ru.same_bits(trk.reversal(z, neg), want) and ru.same_bits(on_device(trk, z, neg), want)


# ---- copies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hemisphere", ["both", "north"])
def test_chunks_row_ranges_and_the_reader(trk, hemisphere):
    lat = ru.grid(5.0)
    steps = 7
    z = ru.field(lat, 8, steps=steps, seed=12)
    tab = ru.table(lat, hemisphere=hemisphere)
    act = np.flatnonzero(tab["eq"] >= 0)
    read = np.unique(np.concatenate([act, tab["eq"][act], tab["po"][act]]))
    r0, r1 = int(read.min()), int(read.max()) + 1
    assert (r0, r1) == ((0, 37) if hemisphere == "both" else (0, 16))
    z[:, :r0], z[:, r1:] = np.float32(-7e30), np.float32(7e30)                  # rows no active row reads: a sentinel that would block or unblock
    want = ru.from_table(z, tab)
    assert blocked(want, tab)
    dev = on_device(trk, z, tab)
    assert ru.same_bits(dev, want)
    ptrs, keep = _native._reversal_rows(tab, 37)
    for cs in (1, 3, steps, steps + 1, 0):
        assert ru.same_bits(trk.reversal(z, tab, chunk_steps=cs), dev), cs
        out = np.full_like(z, 3e33)                                              # what the call does not download it zeroes
        _native.check(_native.lib().ctk_reversal_f32(trk.handle, z.ctypes.data, steps, 37, 8, *ptrs, 0, out.ctypes.data, cs, 0))
        assert ru.same_bits(out, dev), cs
        asked, chunks = [], []

        def reader(t0, nt, view):
            asked.append((t0, nt, view.shape))
            view[...] = z[t0:t0 + nt]

        def writer(t0, nt, values):
            chunks.append((t0, values.copy()))
        assert trk.reversal_cb(reader, z.shape, z.dtype, tab, sink=writer, chunk_steps=cs) is None
        n = steps if cs in (0, steps + 1) else cs
        assert asked == [(t0, min(n, steps - t0), (min(n, steps - t0), 37, 8)) for t0 in range(0, steps, n)], cs
        assert [t0 for t0, _ in chunks] == [a[0] for a in asked] and ru.same_bits(np.concatenate([v for _, v in chunks]), dev), cs
        assert ru.same_bits(reversal_numpy(reader, lat, hemisphere=hemisphere, chunk_steps=cs, shape=z.shape, dtype=z.dtype), dev), cs


def test_argument_errors_leave_the_handle_usable(trk):
    lat = ru.grid(7.5)
    z = ru.field(lat, 8, steps=3)
    tab = ru.table(lat, ghgs2=-5.0)
    want = ru.from_table(z, tab)
    L, h, out = _native.lib(), trk.handle, np.empty_like(z)

    def call(steps=3, chunk_steps=0, out_ptr=out.ctypes.data, keep=0, **changed):
        t = dict(tab)
        for key, (j, v) in changed.items():
            t[key] = t[key].copy()
            t[key][j] = v
        ptrs, _keep = _native._reversal_rows(t, 25)
        return L.ctk_reversal_f32(h, z.ctypes.data, steps, 25, 8, *ptrs, 0, out_ptr, chunk_steps, keep)
    assert call() == 0 and ru.same_bits(out, want)
    for bad in (dict(eq=(4, 25)), dict(po=(4, -2)), dict(eq2=(4, 99)), dict(po=(4, -1)), dict(eq2=(4, -1)), dict(dE=(4, 0.0)), dict(dE=(4, np.inf)), dict(dE=(4, np.nan)),
                dict(tS=(4, np.nan)), dict(tN=(4, -np.inf)), dict(tS2=(4, np.inf)), dict(steps=0), dict(chunk_steps=-1), dict(out_ptr=None)):
        assert call(**bad) == -1 and L.ctk_last_error(), bad
    assert call(eq=(0, -1), dE=(0, np.nan), tS=(0, np.inf)) == 0                 # what an inactive row carries is not looked at
    give_up = _native.READ_CHUNK_FN(lambda user, t0, nt, dst: 1 if t0 else 0)
    ptrs, _keep = _native._reversal_rows(tab, 25)
    assert L.ctk_reversal_stream_cb(h, 4, 3, 25, 8, give_up, None, *ptrs, 0, C.cast(None, _native.WRITE_CHUNK_FN), None, 2, 1) == -1
    assert b"reader returned 1" in L.ctk_last_error() and trk.resident_anom() is None
    assert ru.same_bits(trk.reversal(z, tab), want)                              # the handle works


@pytest.mark.parametrize("cs", [2, 3])
def test_writer_that_gives_up_leaves_nothing_resident_and_the_handle_usable(trk, cs):
    """four chunks of 2, 2, 2, 1 or three of 3, 3, 1 steps (both buffers reused once); the writer fails on the second"""
    lat = ru.grid(5.0)
    z = ru.field(lat, 8, steps=7, seed=12)
    tab = ru.table(lat)
    want = ru.from_table(z, tab)
    assert blocked(want, tab)

    def reader(t0, nt, view):
        view[...] = z[t0:t0 + nt]
    for keep in (False, True):
        seen = []

        def writer(t0, nt, values):
            seen.append(t0)
            if len(seen) == 2:
                raise RuntimeError("disk full")
        with pytest.raises(RuntimeError, match="disk full"):
            trk.reversal_cb(reader, z.shape, z.dtype, tab, sink=writer, chunk_steps=cs, keep_resident=keep)
        assert seen == [0, cs], keep
        if keep:
            assert trk.resident_anom() is None
    L, h = _native.lib(), trk.handle
    tr = _native._Trampolines()
    fill = tr.reader(reader, C.c_float, (37, 8))
    give_up = _native.WRITE_CHUNK_FN(lambda user, t0, nt, src: 1 if t0 else 0)
    ptrs, _keep = _native._reversal_rows(tab, 37)
    for keep in (0, 1):
        assert L.ctk_reversal_stream_cb(h, 4, 7, 37, 8, fill, None, *ptrs, 0, give_up, None, cs, keep) == -1      # CTK_E_INVALID
        err = L.ctk_last_error()
        assert b"ctk_reversal_stream_cb" in err and b"writer returned 1" in err, err
        if keep:
            assert trk.resident_anom() is None
    assert not tr.errors
    assert ru.same_bits(trk.reversal(z, tab), want)                              # the handle works


@pytest.mark.parametrize("cs", [2, 3])
def test_writer_together_with_keep_resident(trk, cs):
    """the kernel writes the resident slot, and the writer gets every chunk from there through the pinned output chunks"""
    lat = ru.grid(5.0)
    z = ru.field(lat, 8, steps=7, seed=12)
    tab = ru.table(lat)
    want = ru.from_table(z, tab)
    assert blocked(want, tab)
    asked, chunks = [], []

    def reader(t0, nt, view):
        asked.append(t0)
        view[...] = z[t0:t0 + nt]

    def writer(t0, nt, values):
        chunks.append((t0, values.copy()))
    g0 = trk.resident_generation()
    assert trk.reversal_cb(reader, z.shape, z.dtype, tab, sink=writer, chunk_steps=cs, keep_resident=True) is None
    assert asked == list(range(0, 7, cs)) and [t0 for t0, _ in chunks] == asked
    assert ru.same_bits(np.concatenate([v for _, v in chunks]), want)
    assert trk.resident_anom() == (7, 37, 8, False) and trk.resident_generation() != g0
    assert trk.percentile(None, 3, 12, 0.9) == trk.percentile(want, 3, 12, 0.9)
    wrow = row_weights(lat.astype(np.float32), np.float32(5.0), np.float32(5.0))
    ids, n_ids = track_numpy(want, wrow, 0, ">", 0.0, 1)
    flag, n = trk.track_resident(np.zeros(7), _native.CMP_OPS[">"], wrow, 0.0, 1)
    assert n_ids > 0 and n == n_ids and np.array_equal(np.array(flag), ids)


# ---- the resident slot ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_resident_slot(trk, dtype):
    lat = ru.grid(5.0)
    z = ru.field(lat, 65, steps=6, seed=21, dtype=dtype)
    tab = ru.table(lat)
    want = ru.from_table(z, tab)
    assert blocked(want, tab)
    wrow = row_weights(lat.astype(np.float32), np.float32(5.0), np.float32(5.0))
    ids, n_ids = track_numpy(want, wrow, 0, ">", 0.0, 1)
    assert n_ids > 10
    g0 = trk.resident_generation()
    assert trk.reversal(z, tab, keep_resident=True, want_out=False, chunk_steps=4) is None
    g1 = trk.resident_generation()
    assert g1 != g0 and trk.resident_anom() == (6, 37, 65, dtype == np.float64)
    thr = np.zeros(6)

    def tracked():
        flag, n = trk.track_resident(thr, _native.CMP_OPS[">"], wrow, 0.0, 1)
        return np.array(flag), n
    flag, n = tracked()
    assert n == n_ids and np.array_equal(flag, ids)
    assert trk.percentile(None, 3, 12, 0.9) == trk.percentile(want, 3, 12, 0.9)
    assert trk.resident_generation() == g1
    bad = dict(tab)                                                              # a failing call: the slab stays what it was, or is dropped
    bad["po"] = tab["po"].copy()
    bad["po"][5] = 37
    with pytest.raises(ValueError, match="partner"):
        trk.reversal(z, bad, keep_resident=True)
    assert trk.resident_anom() in (None, (6, 37, 65, dtype == np.float64))
    if trk.resident_anom() is not None:
        assert trk.resident_generation() == g1
        flag, n = tracked()
        assert n == n_ids and np.array_equal(flag, ids)
    host = trk.reversal(z, tab, keep_resident=True)                              # with the host copy too; another generation
    g2 = trk.resident_generation()
    assert ru.same_bits(host, want) and g2 != g1
    assert ru.same_bits(trk.reversal(z, tab), want) and trk.resident_generation() == g2       # a call that keeps nothing leaves the slot alone
    group = (np.arange(6) % 2).astype(np.int32)
    anom, _ = trk.anomalies(z, group, 2, keep_resident=True)                     # the other producer replaces it
    assert trk.resident_generation() != g2 and trk.resident_anom() == (6, 37, 65, dtype == np.float64)
    assert trk.percentile(None, 3, 12, 0.9) == trk.percentile(anom, 3, 12, 0.9)
    trk.release_io()
    assert trk.resident_anom() is None
