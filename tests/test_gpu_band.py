"""The reductions over space per time step on the device (ctk_band_*, k_band, k_band_sect) against the numpy statement of
tests/band_util.py: every table bit for bit (float64 compared as uint64, NaNs too), whatever the kernel form, the rows in flight, the
pointer alignment, the chunking or the source."""
import ctypes as C
import importlib

import numpy as np
import pytest

import band_util as bu
import golden_util
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (5, 9, 65), (57, 1, 130), (57, 33, 1), (3, 17, 64), (7, 20, 36), (2, 130, 8)]


@pytest.fixture(scope="module")
def trk():
    if _native.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests must run on the GPU box")
    t = _native.Tracker(0)
    yield t
    t.debug_set_band()
    t.close()


def _on_device(trk, arr, offset=0):
    """arr copied into a fresh device buffer, `offset` bytes past a 16-byte boundary; returns (allocation, pointer to the copy)"""
    arr = np.ascontiguousarray(arr)
    base = trk.malloc(arr.nbytes + offset + 32)
    ptr = C.c_void_p((base.value + 15) // 16 * 16 + offset)
    trk.h2d(ptr, arr)
    return base, ptr


def bands(ny):
    """one row (first, last), rows [3, 12), the whole plane, and the row counts that bracket the batches of 8 and 16 and a block of 64"""
    out = [(0, 1), (ny - 1, ny), (0, ny), (3, 12)] + [(1, 1 + n) for n in (7, 8, 9, 63, 64, 65, 129)]
    return sorted({b for b in out if b[1] <= ny})


def sectors_of(nx):
    """the full circle, a wrapping sector, a single column, two that overlap"""
    out = [(0, nx), (nx - 1, min(nx, 3)), (nx // 2, 1), (0, (nx + 1) // 2), (nx // 4, (nx + 1) // 2)]
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_form_alignment_and_band(trk, shape):
    T, ny, nx = shape
    flag = bu.flags(shape, 0.3, seed=T + nx)
    flag.flat[0] = 7                                                       # (the one pixel of the smallest shape is flagged)
    w = bu.order_weights(ny)
    sects = sectors_of(nx)
    want = {b: bu.band(flag, b[0], b[1], w, sects=sects) for b in bands(ny)}
    assert any((v["cnt"] > 0).any() for v in want.values())
    seen = set()
    try:
        for off in (0, 4, 8):
            base, ptr = _on_device(trk, flag, off)
            try:
                for form in (-1, 0, 1):
                    for rows in (-1, 1, 4, 16):
                        trk.debug_set_band(form, rows)
                        for b in bands(ny):
                            got = trk.band_dev(ptr, None, T, ny, nx, b, w, sects)
                            bu.same(got, want[b], (shape, off, form, rows, b))
                        got_form, got_rows, grid = trk.debug_band_launch()
                        vec_ok = nx % 4 == 0 and off == 0
                        assert got_form == (0 if vec_ok and form != 1 else 1) and grid == (T * ((nx + 3) // 4) + 255) // 256
                        assert got_rows == (8 if rows < 0 else rows)
                        seen.add(got_form)
            finally:
                trk.free(base)
    finally:
        trk.debug_set_band()
    assert seen == ({0, 1} if nx % 4 == 0 else {1})


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(5, 9, 65), (3, 17, 64), (2, 130, 8)], ids=lambda s: "x".join(map(str, s)))
def test_every_form_with_a_field(trk, shape, dtype):
    T, ny, nx = shape
    flag = bu.flags(shape, 0.3, seed=7)
    x = bu.field(shape, dtype, seed=ny)
    x[flag <= 0] = np.nan                                                  # never read
    sects = sectors_of(nx)
    try:
        for w in (bu.order_weights(ny), bu.cos_weights(ny)):
            want = {b: bu.band(flag, b[0], b[1], w, x=x, sects=sects) for b in bands(ny)}
            assert all(np.isfinite(v["wx"]).all() and np.isfinite(v["sec_wx"]).all() for v in want.values())
            for off in (0, 8):
                fbase, fptr = _on_device(trk, flag, off)
                xbase, xptr = _on_device(trk, x, off)
                try:
                    for form in (0, 1):
                        for rows in (-1, 1, 16):
                            trk.debug_set_band(form, rows)
                            for b in bands(ny):
                                got = trk.band_dev(fptr, xptr, T, ny, nx, b, w, sects, f64=dtype == np.float64)
                                bu.same(got, want[b], (shape, off, form, rows, b))
                finally:
                    trk.free(fbase)
                    trk.free(xbase)
    finally:
        trk.debug_set_band()


@pytest.mark.parametrize("density", [0.0, 0.05, 0.3, 1.0])
def test_flag_content_thresholds_and_weights(trk, density):
    shape = (5, 9, 65)
    flag = bu.flags(shape, density, seed=5)
    x = bu.field(shape, np.float32, seed=1)
    sects = sectors_of(65)
    for w in (bu.order_weights(9), bu.cos_weights(9)):
        for above in (-1, 0, 500, int(flag.max()) + 1):
            want = bu.band(flag, 0, 9, w, above=above, x=x, sects=sects)
            bu.same(trk.band(flag, (0, 9), w, x, sects, above=above), want, (density, above))
            if above == -1:
                assert (want["cnt"] == 9).all() and np.array_equal(want["sec_area"][0].view(np.uint64), bu.band_total(w, 0, 9, sects, 65).view(np.uint64))
            if above == int(flag.max()) + 1:
                assert not want["cnt"].any() and not want["area"].any() and not np.signbit(want["wx"]).any()


def test_a_reordered_sum_would_show(trk):
    """the order-sensitive weights: rows 1..4 of a fully flagged column add up to 1.0 in rising order and to 0.0 in falling order"""
    flag = np.ones((2, 6, 4), np.int32)
    w = bu.order_weights(6)
    got = trk.band(flag, (0, 4), w, sectors=[(0, 4), (1, 4)])
    assert (got["area"] == 1.0).all() and (got["cnt"] == 4).all()
    cols = trk.band(flag[:, :1], (0, 1), np.ones(1), x=np.tile(w[:4], (2, 1, 1)).astype(np.float64), sectors=[(0, 4), (1, 4)])
    assert np.array_equal(cols["sec_wx"], [[1.0, 0.0]] * 2)                 # columns 0 1 2 3 against 1 2 3 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_field_values_at_unflagged_pixels_reach_nothing(trk, dtype):
    shape = (7, 20, 36)
    flag = bu.flags(shape, 0.3, seed=2)
    x = bu.field(shape, dtype, seed=2)
    clean = bu.band(flag, 3, 12, bu.cos_weights(20), x=x, sects=sectors_of(36))
    bad = x.copy()
    off = np.argwhere(flag <= 0)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        sel = off[k::3]
        bad[sel[:, 0], sel[:, 1], sel[:, 2]] = v
    assert np.isnan(bad).any() and np.isinf(bad).any()
    got = trk.band(flag, (3, 12), bu.cos_weights(20), bad, sectors_of(36))
    bu.same(got, clean)
    assert all(np.isfinite(v).all() for v in got.values())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_nan_at_a_flagged_pixel(trk, dtype):
    shape = (7, 20, 36)
    flag = bu.flags(shape, 0.3, seed=2)
    x = bu.field(shape, dtype, seed=2)
    t, y, c = (int(v) for v in np.argwhere(flag[:, 3:12] > 0)[17] + (0, 3, 0))
    x[t, y, c] = np.nan
    sects = sectors_of(36)
    w = bu.cos_weights(20)
    got = trk.band(flag, (3, 12), w, x, sects)
    bu.same(got, bu.band(flag, 3, 12, w, x=x, sects=sects))
    nan_cols = np.zeros((7, 36), bool)
    nan_cols[t, c] = True
    assert np.array_equal(np.isnan(got["wx"]), nan_cols) and np.isfinite(got["area"]).all()
    nan_sec = np.zeros((7, len(sects)), bool)
    nan_sec[t] = [(c - x0) % 36 < ln for x0, ln in sects]
    assert np.array_equal(np.isnan(got["sec_wx"]), nan_sec) and 0 < nan_sec.sum() < len(sects)
    # outside the band the NaN is not read at all
    bu.same(trk.band(flag, (y + 1, 20), w, x, sects), bu.band(flag, y + 1, 20, w, x=x, sects=sects))
    assert np.isfinite(trk.band(flag, (y + 1, 20), w, x, sects)["wx"]).all()


def test_sectors_only_columns_only_both_and_none(trk):
    shape = (5, 9, 65)
    flag = bu.flags(shape, 0.3, seed=9)
    x = bu.field(shape, np.float64, seed=9)
    w = bu.order_weights(9)
    sects = sectors_of(65) + [(64, 65), (0, 1), (0, 65)]                    # a full circle that starts at the last column; a repeated one
    both = bu.band(flag, 0, 9, w, x=x, sects=sects)
    assert sorted(both) == ["area", "cnt", "sec_area", "sec_cnt", "sec_wx", "wx"]
    for xx in (x, None):
        full = bu.band(flag, 0, 9, w, x=xx, sects=sects)
        bu.same(trk.band(flag, (0, 9), w, xx, sects), full)
        bu.same(trk.band(flag, (0, 9), w, xx, sects, columns=False), {k: v for k, v in full.items() if k.startswith("sec_")})
        for none in (None, [], np.zeros((0, 2), np.int32)):                 # nsect = 0
            bu.same(trk.band(flag, (0, 9), w, xx, none), {k: v for k, v in full.items() if not k.startswith("sec_")})
        base, ptr = _on_device(trk, flag)
        xb, xp = (None, None) if xx is None else _on_device(trk, xx)
        try:
            bu.same(trk.band_dev(ptr, xp, 5, 9, 65, (0, 9), w, sects, columns=False, f64=True), {k: v for k, v in full.items() if k.startswith("sec_")})
            bu.same(trk.band_dev(ptr, xp, 5, 9, 65, (0, 9), w, None, f64=True), {k: v for k, v in full.items() if not k.startswith("sec_")})
        finally:
            trk.free(base)
            if xb is not None:
                trk.free(xb)
    assert np.array_equal(both["sec_cnt"][:, 0], both["sec_cnt"][:, -1]) and np.array_equal(both["sec_cnt"][:, 0], both["cnt"].sum(axis=1))


@pytest.mark.parametrize("dtype", [None, np.float32, np.float64])
def test_chunking_and_sources_agree(trk, dtype):
    shape = (57, 33, 130)
    T = shape[0]
    flag = bu.flags(shape, 0.05, seed=4)
    x = None if dtype is None else bu.field(shape, dtype, seed=4)
    w = bu.cos_weights(33)
    sects = sectors_of(130)
    want = bu.band(flag, 3, 12, w, x=x, sects=sects)
    for chunk_steps in (1, 5, T, 0):
        bu.same(trk.band(flag, (3, 12), w, x, sects, chunk_steps=chunk_steps), want, ("array", chunk_steps))
        calls = []

        def fread(t0, nt, out):
            calls.append(("flag", t0, nt))
            out[...] = flag[t0:t0 + nt]

        def xread(t0, nt, out):
            calls.append(("field", t0, nt))
            out[...] = x[t0:t0 + nt]
        got = trk.band_cb(fread, None if x is None else xread, shape, dtype, (3, 12), w, sects, chunk_steps=chunk_steps)
        bu.same(got, want, ("cb", chunk_steps))
        step = chunk_steps or T
        per = ["flag"] if x is None else ["flag", "field"]                  # the flag reader first
        assert calls == [(s, t0, min(step, T - t0)) for t0 in range(0, T, step) for s in per]
    # the array-level entry: wide flags are narrowed chunk by chunk, an array field beside a flag reader
    bu.same(cm.band_numpy(flag.astype(np.int64), (3, 12), w, x, sects, chunk_steps=5), want)
    bu.same(cm.band_numpy(lambda t0, nt, out: out.__setitem__(Ellipsis, flag[t0:t0 + nt]), (3, 12), w, x, sects, chunk_steps=7, shape=shape,
                          dtype=dtype), want)
    bu.same(cm.band_numpy(flag > 0, (3, 12), w, x, sects), want)                 # narrower than int32: a mask, int16 ids
    bu.same(cm.band_numpy(flag.astype(np.int16), (3, 12), w, x, sects, above=500), bu.band(flag, 3, 12, w, above=500, x=x, sects=sects))


def test_a_failing_reader_surfaces_and_the_handle_goes_on(trk):
    shape = (57, 33, 130)
    flag = bu.flags(shape, 0.3, seed=6)
    x = bu.field(shape, np.float32, seed=6)
    w = bu.cos_weights(33)
    want = bu.band(flag, 0, 33, w, x=x, sects=[(100, 60)])

    class Boom(RuntimeError):
        pass
    for failing in ("flag", "field"):
        calls = []

        def reader(which, src):
            def rd(t0, nt, out):
                calls.append((which, t0))
                if which == failing and t0 > 0:
                    raise Boom("chunk %d" % t0)
                out[...] = src[t0:t0 + nt]
            return rd
        with pytest.raises(Boom, match="chunk 10"):
            trk.band_cb(reader("flag", flag), reader("field", x), shape, np.float32, (0, 33), w, [(100, 60)], chunk_steps=10)
        assert ("flag", 20) not in calls
        bu.same(trk.band_cb(lambda t0, nt, out: out.__setitem__(Ellipsis, flag[t0:t0 + nt]), lambda t0, nt, out: out.__setitem__(Ellipsis, x[t0:t0 + nt]),
                            shape, np.float32, (0, 33), w, [(100, 60)], chunk_steps=10), want, failing)
        bu.same(trk.band(flag, (0, 33), w, x, [(100, 60)]), want, failing)


@pytest.mark.parametrize("name", golden_util.case_names())
def test_identity_with_the_frequency_kernel(trk, name):
    flag = golden_util.load(name)["flag"]
    T, ny, nx = flag.shape
    for above in (0, 1):
        got = trk.band(flag, (0, ny), np.ones(ny), sectors=[(0, nx)], above=above)
        freq = trk.frequency(flag, above=above)[0]
        assert np.array_equal(got["cnt"].sum(axis=0, dtype=np.int64), freq.sum(axis=0, dtype=np.int64))
        assert int(got["cnt"].sum(dtype=np.int64)) == int(got["sec_cnt"].sum(dtype=np.int64)) == np.count_nonzero(flag > above)
        assert np.array_equal(got["area"], got["cnt"].astype(np.float64))      # unit weights: the area is the count


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_anomaly_as_the_field(trk, dtype):
    T, ny, nx = 61, 5, 13
    rng = np.random.default_rng(12)
    raw = (rng.standard_normal((T, ny, nx)) * 50).astype(dtype)
    flag = bu.flags((T, ny, nx), 0.3, seed=12)
    gid = (np.arange(T) % 5).astype(np.int32)
    f64 = dtype == np.float64
    anom, _ = trk.anomalies(raw, gid, 5, keep_resident=True)
    assert trk.resident_anom() == (T, ny, nx, f64)
    gen = trk.resident_generation()
    w = bu.cos_weights(ny)
    sects = [(10, 6), (0, 13)]
    want = bu.band(flag, 1, 5, w, x=anom, sects=sects)
    uploaded = trk.band(flag, (1, 5), w, anom, sects)
    bu.same(uploaded, want, "uploaded")
    for chunk_steps in (0, 7):
        bu.same(trk.band(flag, (1, 5), w, None, sects, chunk_steps=chunk_steps, resident_gen=gen, resident_f64=f64), uploaded, ("resident", chunk_steps))
    calls = []

    def fread(t0, nt, out):
        calls.append((t0, nt))
        out[...] = flag[t0:t0 + nt]
    bu.same(trk.band_cb(fread, None, flag.shape, dtype, (1, 5), w, sects, chunk_steps=20, resident_gen=gen), uploaded, "resident cb")
    assert calls == [(0, 20), (20, 20), (40, 20), (60, 1)]
    base, ptr = _on_device(trk, flag)
    try:
        bu.same(trk.band_dev(ptr, None, T, ny, nx, (1, 5), w, sects, f64=f64, resident_gen=gen), uploaded, "resident dev")
        # another shape or type is not the resident slab
        with pytest.raises(_native.ContrackHipError, match="resident"):
            trk.band(flag[:-1], (1, 5), w, None, sects, resident_gen=gen, resident_f64=f64)
        with pytest.raises(_native.ContrackHipError, match="resident"):
            trk.band(flag, (1, 5), w, None, sects, resident_gen=gen, resident_f64=not f64)
        # a slab that was written since is another generation: the stale one is refused by every entry
        trk.anomalies(raw * 2, gid, 5, keep_resident=True)
        assert trk.resident_generation() != gen and trk.resident_anom() == (T, ny, nx, f64)
        with pytest.raises(_native.ContrackHipError, match="stale generation"):
            trk.band(flag, (1, 5), w, None, sects, resident_gen=gen, resident_f64=f64)
        with pytest.raises(_native.ContrackHipError, match="stale generation"):
            trk.band_cb(fread, None, flag.shape, dtype, (1, 5), w, sects, resident_gen=gen)
        with pytest.raises(_native.ContrackHipError, match="stale generation"):
            trk.band_dev(ptr, None, T, ny, nx, (1, 5), w, sects, f64=f64, resident_gen=gen)
        bu.same(trk.band(flag, (1, 5), w, None, sects, resident_gen=trk.resident_generation(), resident_f64=f64),
                bu.band(flag, 1, 5, w, x=trk.anomalies(raw * 2, gid, 5)[0], sects=sects), "the new slab")
    finally:
        trk.free(base)


def test_the_librarys_argument_errors(trk):
    L = _native.lib()
    flag = np.zeros((2, 4, 6), np.int32)
    x = np.zeros((2, 4, 6), np.float32)
    w = np.ones(4)
    sec = np.array([[0, 6], [5, 2]], np.int32)
    outs = {k: np.zeros((2, 2 if k.startswith("sec_") else 6), np.uint32 if k.endswith("cnt") else np.float64) for k in "cnt area wx sec_cnt sec_area sec_wx".split()}
    bad = [np.array(v, np.int32) for v in ([[0, 6], [6, 1]], [[0, 7], [0, 1]], [[0, 0], [0, 1]])]         # (kept alive: the specs hold their addresses)
    out = _native.BandOut(*[outs[k].ctypes.data for k in "cnt area wx sec_cnt sec_area sec_wx".split()])

    def spec(**kw):
        d = dict(y0=0, y1=4, above=0, nsect=2, w=w.ctypes.data, sectors=sec.ctypes.data, columns=1, resident=0, resident_gen=0)
        d.update(kw)
        return _native.BandSpec(*[d[k] for k, _ in _native.BandSpec._fields_])

    def call(sp, T=2, ny=4, nx=6, chunk=0, o=out, fl=flag):
        return L.ctk_band_f32(trk._h, fl.ctypes.data if fl is not None else None, x.ctypes.data, T, ny, nx, C.byref(sp), C.byref(o) if o is not None else None, chunk)
    cases = [
        (lambda: call(spec(), T=0), -1, "bad shape"), (lambda: call(spec(), nx=0), -1, "bad shape"),
        (lambda: call(spec(y1=5)), -1, "the band [0, 5)"), (lambda: call(spec(y0=4)), -1, "the band [4, 4)"), (lambda: call(spec(y0=-1)), -1, "the band"),
        (lambda: call(spec(w=None)), -1, "null weights"),
        (lambda: call(spec(nsect=-1)), -1, "nsect=-1"), (lambda: call(spec(sectors=None)), -1, "sectors is NULL"),
        (lambda: call(spec(sectors=bad[0].ctypes.data)), -1, "sector 1 = (x0=6, len=1)"),
        (lambda: call(spec(sectors=bad[1].ctypes.data)), -1, "sector 0 = (x0=0, len=7)"),
        (lambda: call(spec(sectors=bad[2].ctypes.data)), -1, "sector 0 = (x0=0, len=0)"),
        (lambda: call(spec(columns=0, nsect=0)), -1, "neither"),
        (lambda: call(spec(), chunk=-1), -1, "chunk_steps=-1"),
        (lambda: call(spec(), o=None), -1, "null output"), (lambda: call(spec(), o=_native.BandOut()), -1, "null buffer (column tables)"),
        (lambda: call(spec(columns=0), o=_native.BandOut()), -1, "null buffer (sector tables)"),
        (lambda: call(spec(), fl=None), -1, "null buffer"),
        (lambda: call(spec(), ny=70000, nx=70000), -4, "uint32 counts"),
        (lambda: L.ctk_band_cb(trk._h, 3, 2, 4, 6, C.cast(C.c_void_p(1), _native.READ_CHUNK_FN), None, C.cast(C.c_void_p(1), _native.READ_CHUNK_FN), None,
                               C.byref(spec()), C.byref(out), 0), -1, "elem_bytes must be 4"),
        (lambda: L.ctk_band_cb(trk._h, 4, 2, 4, 6, C.cast(None, _native.READ_CHUNK_FN), None, C.cast(None, _native.READ_CHUNK_FN), None,
                               C.byref(spec()), C.byref(out), 0), -1, "null flag reader"),
        (lambda: L.ctk_band_dev(trk._h, C.c_void_p(16), C.c_void_p(16), 2, 2, 4, 6, C.byref(spec()), C.byref(out)), -1, "elem_bytes must be 4"),
        (lambda: L.ctk_band_f32(trk._h, flag.ctypes.data, x.ctypes.data, 2, 4, 6, C.byref(spec(resident=1)), C.byref(out), 0), -1, "as well"),
        (lambda: L.ctk_debug_set_band(trk._h, 2, -1), -1, "ctk_debug_set_band"), (lambda: L.ctk_debug_set_band(trk._h, 0, 0), -1, "ctk_debug_set_band"),
    ]
    for fn, rc, text in cases:
        assert fn() == rc, text
        assert text in L.ctk_last_error().decode(), (text, L.ctk_last_error())
    wbad = np.array([1.0, np.inf, 1.0, 1.0])
    assert call(spec(w=wbad.ctypes.data)) == -1 and "w[1] is not finite" in L.ctk_last_error().decode()
    assert call(spec()) == 0                                               # ... and the handle works afterwards
    bu.same({k: outs[k] for k in outs}, bu.band(flag, 0, 4, w, x=x, sects=sec))
