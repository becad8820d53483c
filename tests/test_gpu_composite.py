"""The composite over flagged time steps on the device (ctk_composite_*, k_composite): the float64 sums bit for bit and the counts
exactly against the numpy statement (tests/composite_util.py), through the device, host-array and reader entries, with the rule's
batch of time steps and with shorter forced ones.  The cases are the smallest at which the kernel can still go wrong; the wide-
magnitude input is the one tests/test_composite_host.py shows to discriminate a reversed order, a float32 accumulator and a split
of T."""
import ctypes as C

import numpy as np
import pytest

import composite_util as cu
from contrack_amd import _native

pytestmark = pytest.mark.gpu

PLANES = [(5, 13), (4, 16), (3, 1), (17, 61)]


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.debug_set_composite(-1)
    t.close()


def _case(dtype, T, ny, nx, seed=0, frac=0.3):
    return cu.wide_case(dtype, T, ny, nx, seed=seed, frac=frac)


class OnDevice:
    """flag and x in fresh device buffers, `offset` bytes past a 16-byte boundary"""
    def __init__(self, trk, flag, x, offset=0):
        self.trk, self.flag, self.x = trk, np.ascontiguousarray(flag, dtype=np.int32), np.ascontiguousarray(x)
        self.bases = [trk.malloc(a.nbytes + offset + 16) for a in (self.flag, self.x)]
        self.fp, self.xp = (C.c_void_p(b.value + offset) for b in self.bases)
        trk.h2d(self.fp, self.flag)
        trk.h2d(self.xp, self.x)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bases:
            self.trk.free(b)

    def run(self, ids=None, G=1, above=0, skipna=False, T=None, t0=0, **kw):
        T = self.flag.shape[0] if T is None else T
        ny, nx = self.flag.shape[1:]
        fp = C.c_void_p(self.fp.value + t0 * ny * nx * 4)
        xp = C.c_void_p(self.xp.value + t0 * ny * nx * self.x.dtype.itemsize)
        return self.trk.composite_dev(fp, xp, T, ny, nx, group=ids, ngroups=G, above=above, skipna=skipna, f64=self.x.dtype == np.float64, **kw)


def _same(got, want, tag):
    (gs, gn), (ws, wn) = got, want
    assert gs.dtype == np.float64 and gn.dtype == np.uint32 and gs.shape == ws.shape and gn.shape == wn.shape, tag
    assert np.array_equal(gn, wn), tag
    assert cu.same_bits(gs, ws), (tag, cu.differing(gs, ws))


def _run(trk, flag, x, ids=None, G=1, above=0, skipna=False, offset=0, unrolls=(-1,), tag=None):
    """the device entry against the statement, under every listed batch (-1: the rule's); returns the statement's (sum, n)"""
    want = cu.composite(flag, x, ids, G, above=above, skipna=skipna)
    with OnDevice(trk, flag, x, offset) as d:
        for unroll in unrolls:
            trk.debug_set_composite(unroll)
            try:
                got = d.run(ids, G, above, skipna)
            finally:
                trk.debug_set_composite(-1)
            assert trk.debug_composite_launch()[0] == (16 if unroll < 0 else unroll), (tag, unroll)
            _same(got, want, (tag, unroll))
    return want


# ---- planes, T against the batch, both dtypes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("plane", PLANES)
def test_planes_and_lengths(trk, plane, dtype):
    """T = 1, U - 1, U, U + 1, 2U + 3 for the batch U the rule gives these planes (16) and for a forced batch of 4"""
    ny, nx = plane
    assert _native.composite_plan(np.dtype(dtype).itemsize, ny * nx)["unroll"] == 16
    for u in (16, 4):
        for T in (1, u - 1, u, u + 1, 2 * u + 3):
            flag, x = _case(dtype, T, ny, nx, seed=T)
            _run(trk, flag, x, unrolls=(-1, 4), tag=(plane, T))
    if plane == (17, 61):                                          # 1037 pixels: five workgroups, the last one 13 pixels
        assert _native.composite_plan(4, 17 * 61)["blocks"] == 5 and trk.debug_composite_launch() == (4, 5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_wide_magnitudes(trk, dtype):
    """the discriminating input (T = 61, 5 x 13): rising order, float64 sums, no split of T -- whatever the batch"""
    flag, x = cu.wide_case(dtype)
    for kw in (dict(order="falling"), dict(acc="float32"), dict(slice=8)):
        assert cu.differing(cu.composite(flag, x, None, 1)[0], cu.composite(flag, x, None, 1, **kw)[0]) >= 1, kw
    _run(trk, flag, x, unrolls=(-1, 1, 2, 4, 8, 16), tag="wide")
    flag4, x4 = cu.wide_case(dtype, ny=4, nx=16, seed=9)
    want4 = _run(trk, flag4, x4, tag="wide 4x16")
    assert cu.differing(want4[0], cu.composite(flag4, x4, None, 1, order="falling")[0]) >= 1


def test_pointer_offset_by_4_bytes(trk):
    flag, x = _case(np.float32, 37, 4, 16, seed=2)
    _run(trk, flag, x, offset=4, unrolls=(-1, 4), tag="offset")


# ---- groups ---------------------------------------------------------------------------------------------------------------------------
def _groupings(T):
    rng = np.random.default_rng(T)
    yield "none", None, 1
    yield "cycling", (np.arange(T) % 4).astype(np.int32), 4                        # the accumulator is reloaded at every step
    wrap = ((np.arange(T) + 5) // 6 % 3).astype(np.int32)                          # runs of 6, unsorted: 0 1 2 0 1 2 ... starting inside a run
    yield "wrap", wrap, 3
    yield "empty group", np.where(wrap == 1, 3, wrap).astype(np.int32), 5           # groups 1 and 4 have no step: sum 0, n 0
    yield "random", rng.integers(0, 7, T).astype(np.int32), 7


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("plane", [(5, 13), (4, 16)])
def test_groups(trk, plane, dtype):
    T = 61
    flag, x = _case(dtype, T, *plane, seed=3)
    for name, ids, G in _groupings(T):
        want = _run(trk, flag, x, ids, G, tag=(plane, name))
        if name == "empty group":
            assert not want[1][1].any() and not want[1][4].any() and not want[0][4].any() and not np.signbit(want[0][4]).any()


# ---- chunks, entries, accumulate --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("chunk_steps", [1, 7, 61, 100, 0])
def test_chunks_and_entries_agree(trk, chunk_steps, dtype):
    """the same bits as one launch whatever the chunking; with chunks of 7, runs of equal ids that end exactly at a chunk boundary
    (runs of 7 from step 0) and runs that span one (runs of 6, the first one cut short)"""
    T, ny, nx = 61, 5, 13
    flag, x = cu.wide_case(dtype)
    groupings = list(_groupings(T)) + [("runs of 7", (np.arange(T) // 7 % 3).astype(np.int32), 3)]
    with OnDevice(trk, flag, x) as d:
        for name, ids, G in groupings:
            want = cu.composite(flag, x, ids, G)
            _same(d.run(ids, G), want, (name, "dev"))
            _same(trk.composite(flag, x, ids, G, chunk_steps=chunk_steps), want, (name, "host", chunk_steps))
            calls = []

            def fread(t0, nt, out):
                calls.append(("flag", t0, nt))
                out[...] = flag[t0:t0 + nt]

            def xread(t0, nt, out):
                calls.append(("x", t0, nt))
                out[...] = x[t0:t0 + nt]
            _same(trk.composite_cb(fread, xread, flag.shape, dtype, ids, G, chunk_steps=chunk_steps), want, (name, "cb", chunk_steps))
            step = min(chunk_steps or T, T)
            assert calls == [(w, t0, min(step, T - t0)) for t0 in range(0, T, step) for w in ("flag", "x")]


def test_chunks_with_a_short_batch(trk):
    """chunks of 7 steps against a forced batch of 4: every launch ends in batches of 2 and 1"""
    flag, x = cu.wide_case(np.float32, ny=4, nx=16, seed=4)
    ids = (np.arange(61) // 7 % 3).astype(np.int32)
    want = cu.composite(flag, x, ids, 3)
    trk.debug_set_composite(4)
    try:
        for chunk_steps in (1, 7, 0):
            _same(trk.composite(flag, x, ids, 3, chunk_steps=chunk_steps), want, chunk_steps)
            assert trk.debug_composite_launch() == (4, 1)
    finally:
        trk.debug_set_composite(-1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_accumulate_over_two_calls(trk, dtype):
    T, ny, nx = 61, 5, 13
    flag, x = cu.wide_case(dtype)
    ids = ((np.arange(T) + 5) // 6 % 3).astype(np.int32)
    want = cu.composite(flag, x, ids, 3)
    cells = 3 * ny * nx
    sdev, ndev = trk.malloc(cells * 8), trk.malloc(cells * 4)
    try:
        with OnDevice(trk, flag, x) as d:
            for h in (30, 32):                                     # inside a run of equal ids / at its end
                trk.memset(sdev, 0xff, cells * 8)                  # overwritten by accumulate=0
                trk.memset(ndev, 0xff, cells * 4)
                d.run(ids[:h], 3, T=h, sum_dev=sdev, n_dev=ndev, accumulate=False)
                d.run(ids[h:], 3, T=T - h, t0=h, sum_dev=sdev, n_dev=ndev, accumulate=True)
                s, n = np.empty((3, ny, nx), np.float64), np.empty((3, ny, nx), np.uint32)
                trk.d2h(s, sdev)
                trk.d2h(n, ndev)
                _same((s, n), want, ("halves", h))
            _same(d.run(ids, 3), want, "one call")
    finally:
        trk.free(sdev)
        trk.free(ndev)


# ---- above ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(5, 13), (4, 16)])
def test_above(trk, plane):
    flag, x = _case(np.float32, 21, *plane, seed=6)                 # ids 0 .. 3
    top = int(flag.max())
    for above in (-1, 0, 1, top - 1, top):
        want = _run(trk, flag, x, above=above, tag=(plane, above))
        assert np.array_equal(want[1][0], (flag > above).sum(axis=0))
        if above == -1:
            assert (want[1] == 21).all()
        if above == top:                                           # a flag equal to `above` is not selected: nothing is
            assert not want[1].any() and not want[0].any()


# ---- values -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("plane", [(5, 13), (4, 16)])
def test_nan_inf_zero_and_denormals(trk, plane, dtype):
    T = 23
    ny, nx = plane
    rng = np.random.default_rng(8)
    flag, x = _case(dtype, T, ny, nx, seed=8, frac=0.5)
    x = (x / np.abs(x).max()).astype(dtype)                        # magnitudes below 1: an inf is one we put there
    sel = flag > 0
    # NaN at selected and at unselected steps
    nan = rng.random(x.shape) < 0.1
    xn = np.where(nan, np.nan, x).astype(dtype)
    assert (nan & sel).any() and (nan & ~sel).any()
    ids = (np.arange(T) % 3).astype(np.int32)
    for skipna in (False, True):
        for g, G in ((None, 1), (ids, 3)):
            want = _run(trk, flag, xn, g, G, skipna=skipna, tag=(plane, "nan", skipna))
            assert np.isnan(want[0]).any() != skipna
    # +inf and -inf: alone they stay, together they make NaN; an unselected one does not show
    xi = x.copy()
    flag_i = flag.copy()
    flag_i[0:3, 0, 0], xi[0:3, 0, 0] = 1, [np.inf, 1.0, -np.inf]
    flag_i[0:3, 0, 1], xi[0:3, 0, 1] = [1, 0, 1], [np.inf, -np.inf, np.inf]
    flag_i[0:3, 0, 2], xi[0:3, 0, 2] = [0, 2, 0], [np.nan, -np.inf, np.inf]
    flag_i[3:, 0, 0:3] = 0
    want = _run(trk, flag_i, xi, tag=(plane, "inf"))
    assert np.isnan(want[0][0, 0, 0]) and want[0][0, 0, 1] == np.inf and want[0][0, 0, 2] == -np.inf
    # -0.0 only: the sum stays +0.0
    want = _run(trk, flag, np.full(x.shape, -0.0, dtype), tag=(plane, "-0"))
    assert not want[0].any() and not np.signbit(want[0]).any() and want[1].any()
    # denormals are kept by the conversion to float64 (float32), and added exactly
    tiny = np.finfo(dtype).smallest_subnormal
    xd = (rng.integers(-1000, 1000, x.shape) * tiny).astype(dtype)
    want = _run(trk, flag, xd, tag=(plane, "denormal"))
    if dtype == np.float32:
        assert np.array_equal(want[0][0], np.where(sel, xd.astype(np.float64), 0.0).sum(axis=0)) and want[0].any()


# ---- the resident anomaly slab ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_anomaly_as_the_field(trk, dtype):
    T, ny, nx = 61, 5, 13
    flag, raw = cu.wide_case(dtype, seed=12)
    raw = (raw / np.abs(raw).max() * 50).astype(dtype)
    gid = (np.arange(T) % 5).astype(np.int32)
    anom, _ = trk.anomalies(raw, gid, 5, keep_resident=True)
    assert trk.resident_anom() == (T, ny, nx, dtype == np.float64)
    ids = ((np.arange(T) + 5) // 6 % 3).astype(np.int32)
    want = cu.composite(flag, anom, ids, 3)
    for chunk_steps in (0, 7):
        _same(trk.composite(flag, None, ids, 3, chunk_steps=chunk_steps, resident_f64=dtype == np.float64), want, ("resident", chunk_steps))
    _same(trk.composite(flag, anom, ids, 3), want, "downloaded")
    calls = []

    def fread(t0, nt, out):
        calls.append((t0, nt))
        out[...] = flag[t0:t0 + nt]
    _same(trk.composite_cb(fread, None, flag.shape, dtype, ids, 3, chunk_steps=20), want, "resident cb")
    assert calls == [(0, 20), (20, 20), (40, 20), (60, 1)]
    base = trk.malloc(flag.nbytes)
    try:
        trk.h2d(base, flag)
        _same(trk.composite_dev(base, None, T, ny, nx, group=ids, ngroups=3, f64=dtype == np.float64), want, "resident dev")
    finally:
        trk.free(base)
    # another shape or type is not the resident slab
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.composite(flag[:-1], None, ids[:-1], 3, resident_f64=dtype == np.float64)
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.composite(flag, None, ids, 3, resident_f64=dtype != np.float64)


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(trk):
    flag, x = _case(np.float32, 9, 5, 13, seed=1)
    want = cu.composite(flag, x, None, 1)
    bad = np.zeros(9, np.int32)
    for ids, G in ((np.full(9, 3, np.int32), 3), (np.full(9, -1, np.int32), 3), (bad, 0), (None, 2)):
        with pytest.raises(_native.ContrackHipError):
            trk.composite(flag, x, ids, G)
        with pytest.raises(ValueError):                             # ... which `except ValueError` catches too, as for the frequency
            trk.composite_cb(lambda t0, nt, out: None, lambda t0, nt, out: None, flag.shape, np.float32, ids, G)
    with pytest.raises(_native.ContrackHipError):
        trk.composite(flag, x, chunk_steps=-1)
    with OnDevice(trk, flag, x) as d:
        for shape in ((0, 5, 13), (9, 0, 13), (9, 5, 0), (1 << 32, 1, 1)):
            with pytest.raises(_native.ContrackHipError):
                trk.composite_dev(d.fp, d.xp, *shape)
        with pytest.raises(_native.ContrackHipError):
            trk.composite_dev(None, d.xp, 9, 5, 13)
        _same(d.run(), want, "after the errors")
    with pytest.raises(ValueError):
        trk.composite(flag, x[:-1])
    with pytest.raises(ValueError):
        trk.composite(flag.astype(np.int64), x)

    def broken(t0, nt, out):
        raise KeyError("reader")
    with pytest.raises(KeyError):
        trk.composite_cb(broken, lambda t0, nt, out: None, flag.shape, np.float32)
    _same(trk.composite(flag, x), want, "after a failing reader")
