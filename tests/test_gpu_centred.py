"""The block-centred composite on the device (ctk_centred_*, k_centred): the float64 sums bit for bit and the counts exactly against
the numpy statement (tests/centred_util.py), through the device, host-array and reader entries, in both kernel forms (plain and fed), with the
rule's batch of stamps and workgroup width and with forced ones.  The cases are the smallest at which the kernel can still go wrong; the wide-magnitude input
is the one tests/test_centred_host.py shows to discriminate a reversed order, a float32 accumulator and a split of a bin's stamps."""
import ctypes as C

import numpy as np
import pytest

import centred_util as cu
from contrack_amd import _native

pytestmark = pytest.mark.gpu
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.debug_set_centred(-1, -1, -1)
    t.close()


class OnDevice:
    """x in a fresh device buffer"""
    def __init__(self, trk, x):
        self.trk, self.x = trk, np.ascontiguousarray(x)
        self.xp = trk.malloc(max(self.x.nbytes, 8))
        trk.h2d(self.xp, self.x)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.trk.free(self.xp)

    def run(self, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, **kw):
        T, ny, nx = self.x.shape
        return self.trk.centred_dev(self.xp, T, ny, nx, t, row, col, bin, nbins, hy, hx, wrap=wrap, skipna=skipna, f64=self.x.dtype == np.float64, **kw)


def _same(got, want, tag):
    (gs, gn), (ws, wn) = got, want
    assert gs.dtype == np.float64 and gn.dtype == np.uint32 and gs.shape == ws.shape and gn.shape == wn.shape, tag
    assert np.array_equal(gn, wn), tag
    assert cu.same_bits(gs, ws), (tag, cu.differing(gs, ws))
    assert not np.signbit(gs[gn == 0]).any() and (gs[gn == 0] == 0.0).all(), tag          # an unreached cell is +0.0


BOTH = ((-1, -1, -1), (0, -1, -1), (1, -1, -1))                                # the rule's form, the plain form, the fed form


def _run(trk, x, t, row, col, bin, nbins, hy, hx, wrap=True, skipna=False, forms=(), tag=None):
    """the device entry against the statement: under the rule, in both forms, and under every listed (form, batch, cells per
    workgroup) (-1: the rule's); returns the statement's (sum, n)"""
    want = cu.centred(x, t, row, col, bin, nbins, hy, hx, wrap=wrap, skipna=skipna)
    kept = np.asarray(bin)[np.asarray(bin) >= 0] if len(bin) else np.zeros(0, np.int32)
    longest = int(np.bincount(kept).max()) if len(kept) else 0
    with OnDevice(trk, x) as d:
        for form in BOTH + tuple(forms):
            trk.debug_set_centred(*form)
            try:
                got = d.run(t, row, col, bin, nbins, hy, hx, wrap, skipna)
            finally:
                trk.debug_set_centred(-1, -1, -1)
            if longest:
                plan = _native.centred_plan(x.dtype.itemsize, nbins, hy, hx, longest, len(kept), *form)
                assert trk.debug_centred_launch() == (plan["form"], plan["unroll"], plan["threads"], plan["grid"]), (tag, form)
                if form[0] >= 0:
                    assert plan["form"] == form[0]
                if plan["form"] == 0:
                    rule = _native.centred_plan(x.dtype.itemsize, nbins, hy, hx, longest, len(kept), 0)
                    assert plan["unroll"] == (rule["unroll"] if form[1] < 0 else form[1]) and plan["threads"] == (rule["threads"] if form[2] < 0 else form[2])
            _same(got, want, (tag, form))
    return want


def _stamps(rng, R, T, ny, nx, nbins, lowest=-1):
    return (np.sort(rng.integers(0, T, R)).astype(np.int64), rng.integers(0, ny, R).astype(np.int32), rng.integers(0, nx, R).astype(np.int32),
            rng.integers(lowest, nbins, R).astype(np.int32))


# ---- the discriminating input -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_case(trk, dtype):
    x, t, row, col, bin = cu.wide_case(dtype)
    want = _run(trk, x, t, row, col, bin, 3, 2, 3, forms=((0, 4, 64), (0, 1, 256)), tag="wide")
    assert cu.differing(want[0], cu.centred(x, t, row, col, bin, 3, 2, 3, order="falling")[0]) > 0
    _run(trk, x, t, row, col, bin, 3, 2, 3, wrap=False, forms=((0, 8, 128),), tag="no wrap")
    xn = x.copy()
    xn[np.random.default_rng(5).random(x.shape) < 0.1] = np.nan
    plain = _run(trk, xn, t, row, col, bin, 3, 2, 3, tag="nan")
    skipped = _run(trk, xn, t, row, col, bin, 3, 2, 3, skipna=True, forms=((0, 2, 64),), tag="skipna")
    assert np.isnan(plain[0]).any() and not np.isnan(skipped[0]).any() and (skipped[1] < plain[1]).any()
    _run(trk, xn, t, row, col, bin, 3, 2, 3, wrap=False, skipna=True, tag="skipna, no wrap")


# ---- longitude seam and pole clip -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_seam_and_poles(trk, dtype):
    ny, nx = 7, 12
    x = cu.wide_case(dtype, seed=3)[0]
    # centres on both sides of the seam and at both poles, every combination; hx = 3: the window is split by the seam in both directions
    row = np.array([0, 0, ny - 1, ny - 1, 3, 3, 0, ny - 1], dtype=np.int32)
    col = np.array([0, nx - 1, 0, nx - 1, 0, nx - 1, 5, 6], dtype=np.int32)
    t = np.arange(8, dtype=np.int64) * 2
    for wrap in (True, False):
        for b in range(8):                                                     # one stamp per bin: every cell is one value of x
            bin = np.full(8, -1, np.int32)
            bin[b] = 0
            s, n = _run(trk, x, t, row, col, bin, 1, 2, 3, wrap=wrap, tag=("one stamp", wrap, b))
            for j in range(-2, 3):
                for i in range(-3, 4):
                    y, c = row[b] + j, col[b] + i
                    inside = 0 <= y < ny and (wrap or 0 <= c < nx)
                    assert n[0, j + 2, i + 3] == int(inside)
                    assert s[0, j + 2, i + 3] == (np.float64(x[t[b], y, c % nx]) if inside else 0.0)
        s, n = _run(trk, x, t, row, col, np.arange(8, dtype=np.int32) % 2, 2, 2, 3, wrap=wrap, tag=("seam", wrap))
        assert (n[:, 2, 3] == 4).all() and n.min() < 4                        # clipped cells were met by fewer stamps
    # rows 0 and ny - 1 with hy = ny: only |j| < ny can be inside, and of the rows 2 ny + 1 at most ny
    s, n = _run(trk, x, t[:2], np.array([0, ny - 1], np.int32), np.array([2, 9], np.int32), np.zeros(2, np.int32), 1, ny, 1, tag="hy = ny")
    assert (n[0, 0] == 0).all() and (n[0, -1] == 0).all() and n[0, ny].tolist() == [2, 2, 2]
    # the widest window: 2 hx + 1 == nx on an odd grid, nx - 1 on an even one (a window has an odd number of columns); one more raises
    for nx_, hx in ((12, 5), (13, 6)):
        xw = cu.wide_case(dtype, nx=nx_, seed=4)[0]
        tt, rr, cc, bb = _stamps(np.random.default_rng(nx_), 9, 23, ny, nx_, 2)
        s, n = _run(trk, xw, tt, rr, cc, bb, 2, 1, hx, tag=("widest", nx_))
        with pytest.raises(ValueError, match="twice"):
            trk.centred(xw, tt, rr, cc, bb, 2, 1, hx + 1)
        _run(trk, xw, tt, rr, cc, bb, 2, 1, hx + 1, wrap=False, tag=("wider, not periodic", nx_))
        _run(trk, xw, tt, rr, cc, bb, 2, 1, 2 * nx_, wrap=False, tag=("far wider, not periodic", nx_))
    # hy = hx = 0: the value at the centre
    tt, rr, cc, bb = _stamps(np.random.default_rng(8), 30, 23, ny, nx, 4)
    s, n = _run(trk, x, tt, rr, cc, bb, 4, 0, 0, tag="point")
    assert s.shape == (4, 1, 1) and n[:, 0, 0].tolist() == np.bincount(bb[bb >= 0], minlength=4).tolist()


# ---- the stamp list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stamp_list_edges(trk, dtype):
    x = cu.wide_case(dtype, seed=6)[0]
    T, ny, nx = x.shape
    # several stamps at one time step, two identical ones, an empty bin (1)
    t = np.array([2, 2, 2, 2, 9, 9, 22], dtype=np.int64)
    row = np.array([1, 5, 1, 3, 3, 3, 6], dtype=np.int32)
    col = np.array([0, 7, 0, 11, 4, 4, 2], dtype=np.int32)
    bin = np.array([0, 2, 0, 2, 3, 3, 0], dtype=np.int32)
    s, n = _run(trk, x, t, row, col, bin, 4, 1, 2, tag="ties")
    assert (n[1] == 0).all() and n[3, 1, 2] == 2 and s[3, 1, 2] == 2 * np.float64(x[9, 3, 4])
    # all bins negative, no stamps at all, one bin
    s, n = _run(trk, x, t, row, col, np.full(7, -1, np.int32), 4, 1, 2, tag="all dropped")
    assert not n.any() and not s.any()
    e64, e32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    s, n = _run(trk, x, e64, e32, e32, e32, 2, 1, 2, tag="R = 0")
    assert s.shape == (2, 3, 5) and not n.any()
    _run(trk, x, t, row, col, np.zeros(7, np.int32), 1, 1, 2, tag="one bin")
    with OnDevice(trk, x) as d:
        got = d.run(t, row, col, None, 1, 1, 2)                                # bin None: one bin
    _same(got, cu.centred(x, t, row, col, np.zeros(7, np.int32), 1, 1, 2), "bin None")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("U", [1, 2, 4, 8, 16, 32])
def test_stamps_per_bin_at_the_batch_edges(trk, dtype, U):
    """bins of U - 1, U and U + 1 stamps under a forced batch of U, and of 2 U - 1 and 2 U + 1 (two batches, or one and every shorter one)"""
    x = cu.wide_case(dtype, seed=7)[0]
    T, ny, nx = x.shape
    rng = np.random.default_rng(U)
    counts = [U - 1, U, U + 1, 2 * U - 1, 2 * U + 1]
    bin = rng.permutation(np.repeat(np.arange(5), counts)).astype(np.int32)
    t, row, col, _ = _stamps(rng, len(bin), T, ny, nx, 1)
    want = _run(trk, x, t, row, col, bin, 5, 1, 1, forms=((0, U, -1),), tag=("batch", U))
    assert want[1][:, 1, 1].tolist() == counts
    assert _native.centred_plan(x.dtype.itemsize, 5, 1, 1)["unroll"] == (32 if dtype == np.float32 else 16)      # (the rule's own batch is among them)


@pytest.mark.parametrize("dtype", DTYPES)
def test_stamps_per_bin_at_the_fed_rounds(trk, dtype):
    """the fed form takes K = 15 feeders x 8 (float64: 4) stamps per round: bins of K - 1, K, K + 1, 2 K - 1 and 2 K + 1 stamps, of 1
    (one feeder, one slot) and of U + 1 (a second feeder's first slot); and one bin of 300 stamps, which the rule itself gives to the fed
    form, and of 127, which it does not"""
    x = cu.wide_case(dtype, seed=16)[0]
    T, ny, nx = x.shape
    K = 15 * (8 if dtype == np.float32 else 4)
    rng = np.random.default_rng(K)
    counts = [K - 1, K, K + 1, 2 * K - 1, 2 * K + 1, 1, K // 15 + 1]
    bin = rng.permutation(np.repeat(np.arange(7), counts)).astype(np.int32)
    t, row, col, _ = _stamps(rng, len(bin), T, ny, nx, 1)
    want = _run(trk, x, t, row, col, bin, 7, 2, 3, tag="fed rounds")
    assert want[1][:, 2, 3].tolist() == counts
    assert cu.differing(want[0], cu.centred(x, t, row, col, bin, 7, 2, 3, slice=K)[0]) > 0    # a round summed on its own would show
    xn = x.copy()
    xn[rng.random(x.shape) < 0.1] = np.nan
    _run(trk, xn, t, row, col, bin, 7, 2, 3, skipna=True, tag="fed rounds, skipna")
    _run(trk, xn, t, row, col, bin, 7, 2, 3, wrap=False, tag="fed rounds, no wrap")
    # the rule: one bin of 300 stamps goes to the fed form by itself, 127 do not
    t, row, col, _ = _stamps(rng, 300, T, ny, nx, 1)
    one = np.zeros(300, np.int32)
    with OnDevice(trk, x) as d:
        _same(d.run(t, row, col, one, 1, 2, 3), cu.centred(x, t, row, col, one, 1, 2, 3), "rule: fed")
        assert trk.debug_centred_launch()[0] == 1
        _same(d.run(t[:127], row[:127], col[:127], one[:127], 1, 2, 3), cu.centred(x, t[:127], row[:127], col[:127], one[:127], 1, 2, 3), "rule: plain")
        assert trk.debug_centred_launch()[0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cell_counts_at_the_workgroup_edges(trk, dtype):
    x = cu.wide_case(dtype, seed=9)[0]
    T, ny, nx = x.shape
    rng = np.random.default_rng(10)
    # 255 / 256 / 257 cells as bins of one cell each
    for nbins in (255, 256, 257):
        t, row, col, bin = _stamps(rng, 600, T, ny, nx, nbins, lowest=0)
        _run(trk, x, t, row, col, bin, nbins, 0, 0, tag=("bins", nbins))
    # one below and one above a workgroup's share of a bin (a window has an odd number of cells, so never exactly the share): 63 / 65
    # cells for 64, 119 / 135 for 128, 255 / 273 for 256; not periodic, as the windows are wider than the grid
    t, row, col, bin = _stamps(rng, 50, T, ny, nx, 2)
    for threads, windows in ((64, ((3, 4), (2, 6))), (128, ((3, 8), (4, 7))), (256, ((7, 8), (6, 10)))):
        for hy, hx in windows:
            cells = (2 * hy + 1) * (2 * hx + 1)
            assert abs(cells - threads) <= 17 and _native.centred_plan(4, 2, hy, hx, form=0, threads=threads)["parts"] == (1 if cells < threads else 2)
            _run(trk, x, t, row, col, bin, 2, hy, hx, wrap=False, forms=((0, -1, threads),), tag=("cells", threads, cells))


# ---- chunks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_give_the_same_bits(trk, dtype):
    x, t, row, col, bin = cu.wide_case(dtype, seed=11)
    T, ny, nx = x.shape
    # stamps on the last step of a chunk of 5 and the first of the next, and none at all in steps 10 .. 14
    t = np.sort(np.concatenate([t[(t < 10) | (t > 14)], [4, 4, 5, 5, 9, 15, 19, 19]])).astype(np.int64)
    R = len(t)
    rng = np.random.default_rng(12)
    row, col, bin = rng.integers(0, ny, R).astype(np.int32), rng.integers(0, nx, R).astype(np.int32), rng.integers(-1, 3, R).astype(np.int32)
    bin[t == 19] = -1                                                          # chunk 19 of chunk_steps = 1 holds dropped stamps only
    want = cu.centred(x, t, row, col, bin, 3, 2, 3)
    with OnDevice(trk, x) as d:
        _same(d.run(t, row, col, bin, 3, 2, 3), want, "dev")
    for chunk_steps in (0, 1, 5, 23, 100):
        _same(trk.centred(x, t, row, col, bin, 3, 2, 3, chunk_steps=chunk_steps), want, ("host array", chunk_steps))
        calls = []

        def reader(t0, nt, out):
            calls.append((t0, nt))
            out[...] = x[t0:t0 + nt]
        _same(trk.centred_cb(reader, x.shape, dtype, t, row, col, bin, 3, 2, 3, chunk_steps=chunk_steps), want, ("reader", chunk_steps))
        step = chunk_steps if 0 < chunk_steps < T else T
        carrying = sorted({int(v) // step for v in t[bin >= 0]})
        assert calls == [(k * step, min(step, T - k * step)) for k in carrying], chunk_steps
        if chunk_steps == 5:
            assert (10, 5) not in calls and (5, 5) in calls                  # the chunk without stamps is never read
        if chunk_steps == 1:
            assert (19, 1) not in calls and (10, 1) not in calls
    trk.debug_set_centred(1, -1, -1)                                            # the chunks in the fed form
    try:
        _same(trk.centred(x, t, row, col, bin, 3, 2, 3, chunk_steps=5), want, "host array, fed")
        assert trk.debug_centred_launch()[0] == 1
    finally:
        trk.debug_set_centred(-1, -1, -1)
    # a narrow band of latitude rows: only rows 2 .. 4 of 7 travel (hy = 1 around row 3), and rows 0 .. 1 of the chunk at the pole
    row2 = np.where(t < 12, 3, 0).astype(np.int32)
    want = cu.centred(x, t, row2, col, bin, 3, 1, 3)
    for chunk_steps in (0, 5, 12):
        _same(trk.centred(x, t, row2, col, bin, 3, 1, 3, chunk_steps=chunk_steps), want, ("band", chunk_steps))
        _same(trk.centred_cb(lambda t0, nt, out: out.__setitem__(Ellipsis, x[t0:t0 + nt]), x.shape, dtype, t, row2, col, bin, 3, 1, 3,
                             chunk_steps=chunk_steps), want, ("band, reader", chunk_steps))
    # a reader that fails
    def broken(t0, nt, out):
        raise OSError("no such chunk")
    with pytest.raises(OSError, match="no such chunk"):
        trk.centred_cb(broken, x.shape, dtype, t, row, col, bin, 3, 2, 3, chunk_steps=5)
    _same(trk.centred(x, t, row, col, bin, 3, 2, 3), cu.centred(x, t, row, col, bin, 3, 2, 3), "after the failed reader")


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_with_accumulate_equal_one(trk, dtype):
    x, t, row, col, bin = cu.wide_case(dtype, seed=13)
    want = cu.centred(x, t, row, col, bin, 3, 2, 3)
    assert cu.differing(want[0], cu.centred(x, t, row, col, bin, 3, 2, 3, slice=20)[0]) > 0
    cells = want[0].size
    ds, dn = trk.malloc(cells * 8), trk.malloc(cells * 4)
    try:
        with OnDevice(trk, x) as d:
            trk.memset(ds, 0xff, cells * 8)                                    # accumulate = 0 starts from zero whatever is there
            trk.memset(dn, 0xff, cells * 4)
            assert d.run(t[:20], row[:20], col[:20], bin[:20], 3, 2, 3, sum_dev=ds, n_dev=dn, accumulate=False) is None
            assert d.run(t[20:], row[20:], col[20:], bin[20:], 3, 2, 3, sum_dev=ds, n_dev=dn, accumulate=True) is None
            gs, gn = np.empty_like(want[0]), np.empty_like(want[1])
            trk.d2h(gs, ds)
            trk.d2h(gn, dn)
            _same((gs, gn), want, "two pieces")
            d.run(t[:0], row[:0], col[:0], bin[:0], 3, 2, 3, sum_dev=ds, n_dev=dn, accumulate=True)      # nothing more: nothing changes
            trk.d2h(gs, ds)
            _same((gs, gn), want, "an empty piece")
    finally:
        trk.free(ds)
        trk.free(dn)


# ---- the resident anomaly slab ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_resident_anomaly_as_the_field(trk, dtype):
    raw, t, row, col, bin = cu.wide_case(dtype, seed=14)
    T, ny, nx = raw.shape
    raw = (raw / np.abs(raw).max() * 50).astype(dtype)
    f64 = dtype == np.float64
    fresh = _native.Tracker(0)
    try:                                                                        # a handle that holds no slab
        with pytest.raises(_native.ContrackHipError, match="resident"):
            fresh.centred(None, t, row, col, bin, 3, 2, 3, resident_f64=f64)
        with pytest.raises(_native.ContrackHipError, match="resident"):
            fresh.centred_dev(None, T, ny, nx, t, row, col, bin, 3, 2, 3, f64=f64)
    finally:
        fresh.close()
    anom, _ = trk.anomalies(raw, (np.arange(T) % 5).astype(np.int32), 5, keep_resident=True)
    assert trk.resident_anom() == (T, ny, nx, f64)
    want = cu.centred(anom, t, row, col, bin, 3, 2, 3)
    _same(trk.centred(None, t, row, col, bin, 3, 2, 3, resident_f64=f64), want, "resident")
    _same(trk.centred(None, t, row, col, bin, 3, 2, 3, resident_f64=f64, shape=(T, ny, nx), chunk_steps=5), want, "resident, shape given")
    _same(trk.centred(anom, t, row, col, bin, 3, 2, 3), want, "downloaded")
    _same(trk.centred_cb(None, (T, ny, nx), dtype, t, row, col, bin, 3, 2, 3), want, "resident cb")
    _same(trk.centred_dev(None, T, ny, nx, t, row, col, bin, 3, 2, 3, f64=f64), want, "resident dev")
    # another shape or type is not the resident slab
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.centred(None, t, row, col, bin, 3, 2, 3, resident_f64=not f64)
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.centred(None, t, row, col, bin, 3, 2, 3, resident_f64=f64, shape=(T + 1, ny, nx))
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.centred_dev(None, T, nx, ny, t, row, col, bin, 3, 2, 3, f64=f64)
    with pytest.raises(_native.ContrackHipError, match="resident"):
        trk.centred_cb(None, (T, ny, nx), np.float32 if f64 else np.float64, t, row, col, bin, 3, 2, 3)


# ---- errors -----------------------------------------------------------------------------------------------------------------------
def test_argument_rules(trk):
    x, t, row, col, bin = cu.wide_case(np.float32, seed=15)
    T, ny, nx = x.shape
    want = cu.centred(x, t, row, col, bin, 3, 2, 3)

    def changed(a, k, v):
        a = a.copy()
        a[k] = v
        return a
    bad = [
        dict(t=t[::-1].copy()),                                                # t must be non-decreasing
        dict(t=changed(t, -1, T)), dict(t=changed(t, 0, -1)),
        dict(row=changed(row, 3, ny)), dict(row=changed(row, 3, -1)),
        dict(col=changed(col, 5, nx)), dict(col=changed(col, 5, -1)),
        dict(bin=changed(bin, 7, 3)),                                          # bin < nbins
        dict(nbins=0), dict(nbins=-2),
        dict(hy=-1), dict(hx=-1),
        dict(hx=6),                                                            # 2 hx + 1 = 13 > nx = 12 on a periodic grid
        dict(nbins=3, hy=16383, hx=32767, wrap=False),                         # 3 * 32767 * 65535 cells >= 2^31
    ]
    base = dict(t=t, row=row, col=col, bin=bin, nbins=3, hy=2, hx=3, wrap=True)
    with OnDevice(trk, x) as d:
        for change in bad:
            a = dict(base, **change)
            for call in (lambda: trk.centred(x, **a), lambda: d.run(**a),
                         lambda: trk.centred_cb(lambda t0, nt, out: None, x.shape, np.float32, a["t"], a["row"], a["col"], a["bin"], a["nbins"], a["hy"], a["hx"], a["wrap"])):
                with pytest.raises(ValueError):
                    call()
            with pytest.raises(_native.ContrackHipError):                      # the composite entries' error, which is both
                trk.centred(x, **a)
        for shape in ((0, ny, nx), (T, 0, nx), (T, ny, 0)):
            with pytest.raises(ValueError):
                trk.centred_dev(d.xp, *shape, t, row, col, bin, 3, 2, 3)
        with pytest.raises(ValueError):
            trk.centred(x, t, row, col, bin, 3, 2, 3, chunk_steps=-1)
        with pytest.raises(ValueError):
            trk.centred(x, t, row[:-1], col, bin, 3, 2, 3)
        with pytest.raises(ValueError):
            trk.centred(x, t.astype(np.float64), row, col, bin, 3, 2, 3)
        with pytest.raises(ValueError):
            d.run(t, row, col, bin, 3, 2, 3, sum_dev=C.c_void_p(8))
        _same(d.run(**base), want, "after the errors")
    _same(trk.centred(x, **base), want, "after the errors, host array")
