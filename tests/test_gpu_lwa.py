"""The local wave activity on the GPU (ctk_lwa_*) against its numpy statement tests/lwa_util.py, by bit pattern (level_util.same_bits:
equal dtype and shape, NaN at the same places, equal integer views everywhere else), the output and the contours `ref` alike.  Every
comparison on an ordinary fixture first asserts that at least half of the statement's active pixels are finite and not 0: an
all-zero output cannot pass.  tests/test_lwa_host.py checks the statement itself and that these conditions hold on it."""
import ctypes as C

import numpy as np
import pytest

import lwa_util as lu
from contrack_amd import _native
from contrack_amd.contrack import lwa_numpy, row_weights, track_numpy

pytestmark = pytest.mark.gpu

VECTOR, SCALAR = 1, 0              # Tracker.debug_lwa_form
STEP = {25: 7.5, 37: 5.0, 73: 2.5, 721: 0.25}
SHAPES = ((25, 1), (25, 3), (37, 8), (37, 65), (73, 24), (721, 4))


@pytest.fixture(scope="module")
def trk():
    t = _native.Tracker(0)
    yield t
    t.close()


def fixture(ny, nx, steps=3, seed=None, dtype=np.float32):
    """(lat, z): one column has no waves, so its weather is as large as the difference of neighbouring rows"""
    lat = lu.grid(STEP[ny])
    return lat, lu.field(lat, nx, steps=steps, seed=ny + nx if seed is None else seed, dtype=dtype, noise=400.0 if nx == 1 else 30.0)


TWO_ROWS = np.array([20.0, 40.0])


def two_rows_field(nx):
    return lu.field(TWO_ROWS, nx, steps=8, seed=nx, noise=2000.0)                # (weather alone: two rows have no neighbours to displace)


def busy(want, tab):
    return lu.nonzero_share(want, tab) >= 0.5


def longest(tab):
    return int(np.diff(tab["dom_off"]).max())


def on_device(trk, z, tab, part=0, off=0):
    """the _dev entry on a copy of z that starts `off` bytes past a 16-byte boundary (the output too): (out, ref)"""
    d_x, d_o = trk.malloc(z.nbytes + 16), trk.malloc(z.nbytes + 16)
    try:
        px, po = C.c_void_p(d_x.value + off), C.c_void_p(d_o.value + off)
        trk.h2d(px, z)
        ref = trk.lwa_dev(px, z.shape[0], z.shape[1], z.shape[2], tab, po, part=part, f64=z.dtype == np.float64, want_ref=True)
        got = np.empty_like(z)
        trk.d2h(got, po)
        return got, ref
    finally:
        trk.free(d_x)
        trk.free(d_o)


def both_same(got, want):
    return lu.same_bits(got[0], want[0]) and lu.same_bits(got[1], want[1])


# ---- forms ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_forms(trk, dtype):
    seen = set()
    for ny, nx in SHAPES:
        lat, z = fixture(ny, nx, dtype=dtype)
        tab = lu.rows(lat)
        want = lu.from_table(z, tab, return_ref=True)
        assert busy(want[0], tab), (ny, nx)
        got = trk.lwa(z, tab, want_ref=True)
        form = trk.debug_lwa_form()
        assert form == lu.plan(z.itemsize, longest(tab), nx, 2, 3)["vec"] == int(nx % 4 == 0), (ny, nx, form)
        seen.add(form)
        assert both_same(got, want), (ny, nx)
        assert both_same(lwa_numpy(z, lat, return_reference=True), want), (ny, nx)
    assert seen == {VECTOR, SCALAR}
    assert lu.plan(4, 361, 4)["strip"] == 4 and lu.plan(8, 361, 4, aligned=False)["strip"] == 4 and longest(lu.rows(lu.grid(0.25))) == 361


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_dev_entry_and_offset_pointers(trk, dtype):
    """x_dev and out_dev each one element past a 16-byte boundary: the scalar form, the same bits"""
    for ny, nx in ((37, 8), (721, 4)):
        lat, z = fixture(ny, nx, dtype=dtype)
        tab = lu.rows(lat)
        for part in (0, 1):
            want = lu.from_table(z, tab, part, return_ref=True)
            assert busy(want[0], tab) or part
            for off, form in ((0, VECTOR), (z.itemsize, SCALAR)):
                got = on_device(trk, z, tab, part, off=off)
                assert trk.debug_lwa_form() == form
                assert both_same(got, want), (ny, part, off)


def test_stride_loop_strips_and_workgroup_to_xcd_mappings(trk):
    """fewer workgroups than (step, domain, strip) triples, every XCD mapping, and rows of more than one strip -- whole strips and a
    narrower last one, in both forms"""
    cases = []
    for (ny, nx), steps in (((37, 65), 6), ((73, 24), 5), ((73, 120), 3), ((73, 59), 3)):
        lat, z = fixture(ny, nx, steps=steps)
        cases.append((z, lu.rows(lat)))
    wants = [lu.from_table(z, tab, return_ref=True) for z, tab in cases]
    assert all(busy(w[0], tab) for w, (_, tab) in zip(wants, cases))
    plans = [_native.lwa_plan(4, 19, 65, 2, 6), _native.lwa_plan(4, 37, 24, 2, 5), _native.lwa_plan(4, 37, 120, 2, 3), _native.lwa_plan(4, 37, 59, 2, 3)]
    assert [(p["vec"], p["strip"], p["nstrips"], p["blocks"]) for p in plans] == [(0, 65, 1, 12), (1, 24, 1, 10), (1, 52, 3, 18), (0, 55, 2, 12)]
    try:
        for mode in (-1, 0, 1, 2):
            for cap in (0, 1, 5, 1000):
                trk.debug_set_lwa(mode, cap)
                for (z, tab), want, p in zip(cases, wants, plans):
                    assert both_same(trk.lwa(z, tab, want_ref=True), want), (mode, cap, z.shape)
                    assert trk.debug_lwa_launch() == (p["vec"], min(cap or p["blocks"], p["blocks"]))
    finally:
        trk.debug_set_lwa()


# ---- rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hemisphere", ["both", "north", "south"])
def test_hemispheres_parts_and_latitude_axes(trk, hemisphere):
    base = lu.grid(5.0)
    for lat in (base, base[::-1].copy(), lu.shuffled(base, 3), lu.gaussian(), lu.shuffled(lu.gaussian(), 5)):
        z = lu.field(lat, 8, steps=3, seed=len(lat))
        tab = lu.rows(lat, hemisphere=hemisphere)
        act = np.flatnonzero(tab["active"])
        assert len(act) == {37: 10, 48: 12}[len(lat)] * (2 if hemisphere == "both" else 1)
        for part in lu.PARTS:
            want = lu.from_table(z, tab, part, return_ref=True)
            assert busy(want[0], tab) or part != "total"
            assert np.count_nonzero(want[0]) and not np.count_nonzero(np.delete(want[0], act, axis=1))
            assert both_same(trk.lwa(z, tab, part=part, want_ref=True), want), (part, lat[:3])
            assert both_same(lwa_numpy(z, lat, hemisphere=hemisphere, part=part, return_reference=True), want), (part, lat[:3])


def test_two_row_domain_pole_row_and_shared_equator_row(trk):
    two = TWO_ROWS                                                               # one domain of two rows, one of them active
    tab = lu.rows(two, hemisphere="north")
    assert tab["dom_rows"].tolist() == [0, 1] and tab["active"].tolist() == [0, 1]
    for nx in (3, 8):
        z = two_rows_field(nx)
        want = lu.from_table(z, tab, return_ref=True)
        assert busy(want[0], tab)
        assert both_same(trk.lwa(z, tab, want_ref=True), want) and both_same(on_device(trk, z, tab), want)
    lat = lu.grid(7.5)                                                           # 90N and 90S: W = 0, the last row of each domain; the equator row in both
    tab = lu.rows(lat, lat_bounds=(7.5, 82.5))
    north, south = lu.domains(tab)
    assert north[-1] == 0 and south[-1] == 24 and tab["W"][0] == 0 and tab["W"][24] == 0 and north[0] == south[0] == 12 and not tab["active"][12]
    z = lu.field(lat, 8, steps=3, seed=11)
    z[:, 0, :], z[:, 24, :] = np.float32(9e9), np.float32(-9e9)                  # pole rows weigh nothing in the contours but are integrated over (q = 0 there only if cos is 0)
    want = lu.from_table(z, tab, return_ref=True)
    assert busy(want[0], tab) and np.all(np.abs(want[1]) < 1e5)
    assert both_same(trk.lwa(z, tab, want_ref=True), want)
    eq = z.copy()
    eq[:, 12, :] = np.float32(5800.0) + np.arange(8, dtype=np.float32)           # the shared row matters to both hemispheres
    want2 = lu.from_table(eq, tab, return_ref=True)
    assert lu.differing(want2[0][:, :12], want[0][:, :12]) and lu.differing(want2[0][:, 13:], want[0][:, 13:])
    assert both_same(trk.lwa(eq, tab, want_ref=True), want2)


# ---- values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_all_equal_plane(trk, dtype):
    lat = lu.grid(5.0)
    tab = lu.rows(lat)
    z = lu.all_equal(lat, 8, value=5500.0, dtype=dtype)
    for got in (trk.lwa(z, tab, want_ref=True), on_device(trk, z, tab), on_device(trk, z, tab, off=z.itemsize)):
        assert not got[0].any() and not np.signbit(got[0]).any()
        assert np.all(got[1][:, tab["active"] != 0] == 5500.0) and not got[1][:, tab["active"] == 0].any()
    assert both_same(trk.lwa(z, tab, want_ref=True), lu.from_table(z, tab, return_ref=True))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_ties_signed_zeros_nan_and_inf(trk, dtype):
    lat = lu.grid(5.0)
    tab, low = lu.rows(lat), lu.rows(lat, lat_bounds=(5, 75))
    z = lu.field(lat, 65, steps=3, seed=1, dtype=dtype)
    planes = {}
    planes["ties"] = (lu.quantised(z), tab)
    assert lu.tie_rows(planes["ties"][0], tab) >= 3
    zero = (z - dtype(5400.0)).astype(dtype)                                     # contours near 0: +0.0 and -0.0 are different keys
    planes["zeros"] = (lu.sprinkle(zero, tab, [0.0, -0.0], share=0.3, seed=2), tab)
    planes["nan"] = (lu.sprinkle(z, low, [np.nan], share=0.15, seed=5, steps=[0]), low)
    planes["inf"] = (lu.sprinkle(z, tab, [np.inf, -np.inf], share=0.03, seed=6), tab)
    planes["mixed"] = (lu.sprinkle(lu.quantised(z), low, [np.nan, np.inf, -np.inf, 0.0, -0.0], share=0.1, seed=7), low)
    for name, (zz, t) in planes.items():
        for part in (0, 1, 2):
            want = lu.from_table(zz, t, part, return_ref=True)
            if name == "nan":
                bad, good = lu.nan_rows(want[1], t)
                assert bad[0] >= 1 and good[0] >= 1 and np.isnan(want[0][0]).any() and np.isfinite(want[0][0][t["active"] != 0]).any()
            if name == "zeros":
                assert np.count_nonzero(want[1] == 0) > np.count_nonzero(t["active"] == 0) * 3          # some contours ARE a zero
            if name == "inf" and part == 0:
                assert np.isinf(want[0]).any()
            assert both_same(trk.lwa(zz, t, part=part, want_ref=True), want), (name, part)
        assert both_same(on_device(trk, zz, t, off=zz.itemsize), lu.from_table(zz, t, return_ref=True)), name


# ---- copies -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hemisphere", ["both", "north"])
def test_chunks_row_ranges_reader_and_writer(trk, hemisphere):
    lat = lu.grid(5.0)
    steps = 5
    z = lu.field(lat, 8, steps=steps, seed=12)
    tab = lu.rows(lat, hemisphere=hemisphere)
    if hemisphere == "north":
        z[:, 19:] = np.float32(7e30)                                             # rows of no domain: never uploaded, never read
    want = lu.from_table(z, tab, return_ref=True)
    assert busy(want[0], tab)
    dev = on_device(trk, z, tab)
    assert both_same(dev, want)
    args, keep = _native._lwa_rows(tab, 37)
    for cs in (1, 2, steps, 0):
        assert both_same(trk.lwa(z, tab, chunk_steps=cs, want_ref=True), want), cs
        out, ref = np.full_like(z, 3e33), np.full((steps, 37), 3e33, dtype=np.float32)          # what the call does not download it zeroes
        _native.check(_native.lib().ctk_lwa_f32(trk.handle, z.ctypes.data, steps, 37, 8, *args, 0, out.ctypes.data, ref.ctypes.data, cs, 0))
        assert both_same((out, ref), want), cs
        asked, chunks = [], []

        def reader(t0, nt, view):
            asked.append((t0, nt, view.shape))
            view[...] = z[t0:t0 + nt]

        def writer(t0, nt, values):
            chunks.append((t0, values.copy()))
        none, ref = trk.lwa_cb(reader, z.shape, z.dtype, tab, sink=writer, chunk_steps=cs, want_ref=True)
        n = cs or steps
        assert none is None and asked == [(t0, min(n, steps - t0), (min(n, steps - t0), 37, 8)) for t0 in range(0, steps, n)], cs
        assert [t0 for t0, _ in chunks] == [a[0] for a in asked] and both_same((np.concatenate([v for _, v in chunks]), ref), want), cs
        assert both_same(lwa_numpy(reader, lat, hemisphere=hemisphere, chunk_steps=cs, shape=z.shape, dtype=z.dtype, return_reference=True), want), cs


def test_reader_or_writer_that_gives_up(trk):
    lat = lu.grid(5.0)
    z = lu.field(lat, 8, steps=5, seed=12)
    tab = lu.rows(lat)
    want = lu.from_table(z, tab)
    L, h = _native.lib(), trk.handle
    args, _keep = _native._lwa_rows(tab, 37)
    tr = _native._Trampolines()
    fill = tr.reader(lambda t0, nt, view: view.__setitem__(Ellipsis, z[t0:t0 + nt]), C.c_float, (37, 8))
    give_up_r = _native.READ_CHUNK_FN(lambda user, t0, nt, dst: 1 if t0 else 0)
    give_up_w = _native.WRITE_CHUNK_FN(lambda user, t0, nt, src: 1 if t0 else 0)
    no_writer = C.cast(None, _native.WRITE_CHUNK_FN)
    for keep in (0, 1):
        assert L.ctk_lwa_stream_cb(h, 4, 5, 37, 8, give_up_r, None, *args, 0, no_writer if keep else give_up_w, None, None, 2, keep) == -1       # CTK_E_INVALID
        assert b"ctk_lwa_stream_cb" in L.ctk_last_error() and b"reader returned 1" in L.ctk_last_error()
        assert L.ctk_lwa_stream_cb(h, 4, 5, 37, 8, fill, None, *args, 0, give_up_w, None, None, 2, keep) == -1
        assert b"writer returned 1" in L.ctk_last_error()
        if keep:
            assert trk.resident_anom() is None
        assert lu.same_bits(trk.lwa(z, tab), want)                               # the next call on the handle works
    assert not tr.errors


# ---- the resident slot ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_resident_slot(trk, dtype):
    import reversal_util as ru
    lat = lu.grid(5.0)
    z = lu.field(lat, 65, steps=6, seed=21, dtype=dtype)
    tab = lu.rows(lat)
    want = lu.from_table(z, tab, part=1)
    wrow = row_weights(lat.astype(np.float32), np.float32(5.0), np.float32(5.0))
    level = float(np.percentile(want[:, tab["active"] != 0], 80))
    ids, n_ids = track_numpy(want, wrow, level, ">", 0.0, 1)
    assert n_ids > 5
    thr = np.full(6, level)
    shape = (6, 37, 65, dtype == np.float64)

    def tracked():
        flag, n = trk.track_resident(thr, _native.CMP_OPS[">"], wrow, 0.0, 1)
        return np.array(flag), n
    g0 = trk.resident_generation()
    assert trk.lwa(z, tab, part=1, keep_resident=True, want_out=False, chunk_steps=4) is None          # out = NULL
    g1 = trk.resident_generation()
    assert g1 != g0 and trk.resident_anom() == shape
    flag, n = tracked()
    assert n == n_ids and np.array_equal(flag, ids)
    assert trk.resident_generation() == g1
    bad = dict(tab)                                                              # a failing call: the slab stays what it was, or is dropped
    bad["dom_rows"] = tab["dom_rows"].copy()
    bad["dom_rows"][3] = 37
    with pytest.raises(ValueError, match="outside"):
        trk.lwa(z, bad, keep_resident=True)
    assert trk.resident_anom() == shape and trk.resident_generation() == g1
    host = trk.lwa(z, tab, part=1, keep_resident=True)                           # with the host copy too; another generation
    g2 = trk.resident_generation()
    assert lu.same_bits(host, want) and g2 != g1
    assert lu.same_bits(trk.lwa(z, tab, part=1), want) and trk.resident_generation() == g2       # a call that keeps nothing leaves the slot alone
    group = (np.arange(6) % 2).astype(np.int32)
    anom, _ = trk.anomalies(z, group, 2, keep_resident=True)                     # a later anomaly call replaces the slot ...
    g3 = trk.resident_generation()
    assert g3 != g2 and trk.percentile(None, 3, 12, 0.9) == trk.percentile(anom, 3, 12, 0.9)
    assert trk.lwa(z, tab, part=1, keep_resident=True, want_out=False) is None    # ... and the reverse
    g4 = trk.resident_generation()
    flag, n = tracked()
    assert g4 != g3 and n == n_ids and np.array_equal(flag, ids)
    rtab = ru.table(lat)
    rev = trk.reversal(z, rtab, keep_resident=True)                              # a later reversal call replaces it ...
    g5 = trk.resident_generation()
    assert g5 != g4 and ru.same_bits(rev, ru.from_table(z, rtab)) and trk.percentile(None, 3, 12, 0.9) == trk.percentile(rev, 3, 12, 0.9)
    assert lu.same_bits(trk.lwa(z, tab, part=1, keep_resident=True), want)        # ... and the reverse
    flag, n = tracked()
    assert trk.resident_generation() != g5 and n == n_ids and np.array_equal(flag, ids)
    trk.release_io()
    assert trk.resident_anom() is None


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_handle_usable(trk):
    lat = lu.grid(7.5)
    z = lu.field(lat, 8, steps=3)
    tab = lu.rows(lat)
    want = lu.from_table(z, tab)
    L, h, out = _native.lib(), trk.handle, np.empty_like(z)
    act = int(np.flatnonzero(tab["active"])[0])

    def call(steps=3, ny=25, nx=8, chunk_steps=0, out_ptr=out.ctypes.data, keep=0, part=0, null=None, ndom=None, x_ptr=z.ctypes.data, handle=h, **changed):
        t = dict(tab)
        for key, (j, v) in changed.items():
            t[key] = t[key].copy()
            t[key][j] = v
        args, _keep = _native._lwa_rows(t, 25)
        if ndom is not None:
            args[0] = ndom
        if null is not None:
            args[null] = None
        return L.ctk_lwa_f32(handle, x_ptr, steps, ny, nx, *args, part, out_ptr, None, chunk_steps, keep)
    assert call() == 0 and lu.same_bits(out, want)
    # every case with a word that only its own check says: one guard cannot stand in for another
    bads = [(dict(null=i), b"null pointer") for i in range(1, 7)] + [
        (dict(handle=None), b"null pointer"), (dict(ny=0), b"size below 1"), (dict(nx=0), b"size below 1"), (dict(x_ptr=None), b"null input"),
        (dict(steps=0), b"steps = 0"), (dict(ndom=0), b"ndom = 0"), (dict(ndom=3), b"ndom = 3"),
        (dict(dom_rows=(2, 25)), b"row 25 outside"), (dict(dom_rows=(2, -1)), b"row -1 outside"),
        (dict(dom_rows=(2, int(tab["dom_rows"][3]))), b"twice"),                                       # a row twice in one domain
        (dict(dom_off=(0, 1)), b"dom_off[0] = 1"), (dict(dom_off=(1, 0)), b"domain 0 has 0 rows"),    # not from 0, an empty domain,
        (dict(dom_off=(2, 9)), b"domain 1 has -4 rows"), (dict(dom_off=(1, 26)), b"domain 0 has 26 rows"),   # offsets that fall, a domain longer than ny
        (dict(active=(12, 1), S=(12, 1.0)), b"row 12 lies in two domains"),                            # the equator row, active: it is in both
        (dict(active=(12, 1)), b"S[12]"),                                                               # ... and without an S
        (dict(q=(act, np.nan)), b"q[%d] = nan" % act), (dict(q=(act, np.inf)), b"q[%d] = inf" % act), (dict(q=(0, -1e-9)), b"q[0] = -1e-09"),
        (dict(S=(act, 0.0)), b"S[%d] = 0" % act), (dict(S=(act, np.inf)), b"S[%d] = inf" % act), (dict(S=(act, np.nan)), b"S[%d] = nan" % act),
        (dict(S=(act, -1.0)), b"S[%d] = -1" % act),
        (dict(part=3), b"part = 3"), (dict(part=-1), b"part = -1"), (dict(chunk_steps=-1), b"chunk_steps = -1"), (dict(out_ptr=None), b"nothing to produce")]
    for bad, word in bads:
        assert call(**bad) == -1 and word in L.ctk_last_error(), (bad, L.ctk_last_error())
    # an active row in no domain; cap = 0 on an active row (the pole row, W = 0, the last of its domain); nx * the weights at 2^63
    north = lu.rows(lat, hemisphere="north")
    for key, j, v, text in (("active", 20, 1, b"no domain"), ("active", 0, 1, b"cap = 0")):
        t = dict(north)
        t[key] = north[key].copy()
        t[key][j] = v
        t["S"] = north["S"].copy()
        t["S"][j] = 1.0
        args, _keep = _native._lwa_rows(t, 25)
        assert L.ctk_lwa_f32(h, z.ctypes.data, 3, 25, 8, *args, 0, out.ctypes.data, None, 0, 0) == -1 and text in L.ctk_last_error(), key
    # nx * the weights of a domain at 2^63: the library guards it, but uint32 weights cannot get there -- the largest weights on the
    # largest plane stay below it, and one pixel more is refused as a plane of 2^31 pixels (checked before x is read)
    t = dict(ndom=1, dom_off=[0, 4], dom_rows=[0, 1, 2, 3], active=[0, 1, 0, 0], W=[2 ** 32 - 1] * 4, q=[0.1] * 4, S=[0, 1.0, 0, 0])
    args, _keep = _native._lwa_rows(t, 4)
    assert (2 ** 32 - 1) * (2 ** 31 - 1) < 2 ** 63
    assert L.ctk_lwa_f32(h, z.ctypes.data, 1, 4, 2 ** 29, *args, 0, out.ctypes.data, None, 0, 0) == -1 and b"pixels" in L.ctk_last_error()
    long_ = dict(ndom=1, dom_off=[0, 2044], dom_rows=np.arange(2044), active=np.ones(2044), W=np.ones(2044), q=np.ones(2044), S=np.ones(2044))
    args, _keep = _native._lwa_rows(long_, 2044)
    assert L.ctk_lwa_f32(h, z.ctypes.data, 1, 2044, 1, *args, 0, out.ctypes.data, None, 0, 0) == -1 and b"LDS" in L.ctk_last_error()           # the capacity edge: no other form
    assert call(S=(12, np.nan)) == 0 and lu.same_bits(out, want)                 # what an inactive row carries in S is not looked at
    with pytest.raises(ValueError, match="dom_rows"):                            # offsets beyond the table: refused before the library reads it
        _native._lwa_rows(dict(tab, dom_off=[0, 13, 40]), 25)
    assert call() == 0 and lu.same_bits(out, want)                               # the handle works
    with pytest.raises(ValueError, match="part"):
        trk.lwa(z, tab, part="both")
