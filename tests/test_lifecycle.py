"""run_lifecycle (next row N1): oracle port and host finishing step against the reference's own frames
(tests/golden/life), then the HIP reductions (ctk_lifecycle_*) against both."""
import numpy as np
import pytest

import life_util
import minixr
from contrack_amd.contrack import contrack, lifecycle_frame, row_weights
from oracle import lifecycle_port

minixr.install_as_xarray()
CASES = life_util.case_names()


def test_fixtures_present():
    assert {"refslab", "smooth0", "smooth1", "smooth2", "ring", "float64", "othervar", "big"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_oracle_port_matches_reference(name):
    g = life_util.load(name)
    got = lifecycle_port.run_lifecycle(g["flag"], g["variable"], g["lat"], g["lon"], g["wrow"], life_util.dates_of(g["time"]))
    assert got == g["frame"]                       # same call sequence as the reference: identical, digit for digit


@pytest.mark.parametrize("name", CASES)
def test_host_finish_matches_reference(name):
    """lifecycle_frame (divisions, int(), coordinate look-ups, rounding) on numpy-built rows"""
    g = life_util.load(name)
    rows = life_util.numpy_rows(g["flag"], g["variable"], g["wrow"])
    got = lifecycle_frame(rows, g["lat"], g["lon"], life_util.dates_of(g["time"]))
    _compare(got, g["frame"])


def test_fixtures_cover_the_seam_roll():
    rolled = 0
    for name in CASES:
        g = life_util.load(name)
        rows = life_util.numpy_rows(g["flag"], g["variable"], g["wrow"])
        rolled += int((rows["shift"] > 0).sum())
    assert rolled >= 20
    ring = life_util.numpy_rows(life_util.load("ring")["flag"], life_util.load("ring")["variable"], life_util.load("ring")["wrow"])
    assert (ring["shift"] == 1).any()              # every column occupied: np.argmax of equal gaps -> roll by cols[1]


def test_finish_errors():
    from contrack_amd._native import LIFE_ROW
    lat, lon = np.linspace(90, -90, 5), np.arange(4.0)
    r = np.zeros(1, dtype=LIFE_ROW)
    r["label"], r["shift"], r["area"], r["swv"] = 3, -1, 2.0, 0.0
    with pytest.raises(ValueError, match="NaN"):
        lifecycle_frame(r, lat, lon, ["d0"])       # int(nan) in the reference
    r["shift"] = -2
    with pytest.raises(ValueError, match="argmax"):
        lifecycle_frame(r, lat, lon, ["d0"])
    r["shift"], r["swv"], r["swvy"], r["swvx"] = -1, 1.0, -0.5, -1.5     # negative centre: int() truncates, Python index wraps
    out = lifecycle_frame(r, lat, lon, ["d0"])
    assert out[0][2] == int(lon[-1]) and out[0][3] == int(lat[0])
    r["swvx"] = 99.0
    with pytest.raises(IndexError):
        lifecycle_frame(r, lat, lon, ["d0"])


def _compare(got, want, tol=0.0101):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[:4] == b[:4], (a, b)
        assert abs(a[4] - b[4]) <= tol and abs(a[5] - b[5]) <= tol * max(1.0, abs(b[5]) * 1e-9), (a, b)


# ---------------------------------------------------------------------------------------------------------------
# HIP
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tracker():
    from contrack_amd import _native
    with _native.Tracker(0) as t:
        yield t


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_rows_and_frame_match_reference(tracker, name):
    g = life_util.load(name)
    rows = tracker.lifecycle(g["flag"], g["variable"], g["wrow"])
    want = life_util.numpy_rows(g["flag"], g["variable"], g["wrow"])
    assert np.array_equal(rows["t"], want["t"]) and np.array_equal(rows["label"], want["label"])
    assert np.array_equal(rows["shift"], want["shift"])
    assert np.array_equal(rows["area"], want["area"])                 # exact: integer limbs, rounded once
    for k in ("swv", "swvy", "swvx"):
        assert np.allclose(rows[k], want[k], rtol=1e-12, atol=1e-9), k
    _compare(lifecycle_frame(rows, g["lat"], g["lon"], life_util.dates_of(g["time"])), g["frame"])


@pytest.mark.gpu
def test_class_run_lifecycle_known_answer():
    """tests/test_contrack.py:93-103 through the drop-in class: 3 flags, 28 rows, and the reference's values"""
    g = life_util.load("refslab")
    ds = minixr.make_dataset(g["field"], g["lat"], g["lon"], time=g["time"])
    ds["time"].attrs = {}
    ds["flag"] = minixr.DataArray(g["flag"].astype(np.int64), ("time", "latitude", "longitude"))
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    df = c.run_lifecycle(flag="flag", variable="anom")
    assert list(df.columns) == ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']
    assert len(df.Flag.unique()) == 3 and len(df) == 28
    _compare([tuple(r) for r in df.itertuples(index=False)], g["frame"])


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True])
def test_hip_lifecycle_on_tracked_slab(tracker, f64):
    """track a synthetic slab on the GPU, then life cycle of its flags against the scipy port"""
    from contrack_amd import synth
    T, ny, nx = 40, 91, 180
    anom = synth.smooth_field(T, ny, nx, seed=5)
    if f64:
        anom = anom.astype(np.float64) + 1e-7
    lat, lon = synth.grid(ny, nx)
    wrow = row_weights(lat, 2.0, 2.0)
    flag, n = tracker.track(anom, np.full(T, 100.0), 0, wrow, 0.4, 3, True, f64=f64)
    assert n > 3
    rows = tracker.lifecycle(flag, anom, wrow)
    dates = ["%03d" % t for t in range(T)]
    got = lifecycle_frame(rows, lat, lon, dates)
    want = lifecycle_port.run_lifecycle(flag, anom, lat, lon, wrow, dates)
    assert (rows["shift"] > 0).any()
    _compare(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,thr,pers", [((6, 721, 1440), 160.0, 2), ((24, 181, 360), 160.0, 3), ((8, 192, 288), 150.0, 2)])
def test_hip_lifecycle_on_baseline_grids(tracker, shape, thr, pers):
    """the grids of BASELINE.json (0.25 deg: six 256-column strips x 23 bands of 4 x 8 rows per plane -- few time steps keep the rows
    per wave at 8; the production forms, 37 and 46 rows per wave, are in tests/test_gpu_lifecycle_forms.py; 1 deg; CESM): frame
    identical to the scipy port's in every column, with the rows on rounding boundaries re-evaluated on the device"""
    from contrack_amd import synth
    T, ny, nx = shape
    anom = synth.smooth_field(T, ny, nx, seed=9)
    lat, lon = synth.grid(ny, nx)
    wrow = row_weights(lat, 180.0 / (ny - 1), 360.0 / nx)
    flag, n = tracker.track(anom, np.full(T, thr), 0, wrow, 0.5, pers, True)
    assert n > 2
    rows = tracker.lifecycle(flag, anom, wrow)
    dates = ["%03d" % t for t in range(T)]
    got = lifecycle_frame(rows, lat, lon, dates, tracker)
    assert (rows["shift"] > 0).any()                                   # contours across the seam
    assert got == lifecycle_port.run_lifecycle(flag, anom, lat, lon, wrow, dates)


@pytest.mark.gpu
def test_hip_lifecycle_device_resident_and_empty(tracker):
    from contrack_amd import synth
    T, ny, nx = 6, 46, 72
    rng = np.random.default_rng(0)
    flag = np.zeros((T, ny, nx), dtype=np.int32)
    field = rng.random((T, ny, nx), dtype=np.float32) + 1
    wrow = row_weights(synth.grid(ny, nx)[0], 4.0, 5.0)
    assert len(tracker.lifecycle(flag, field, wrow)) == 0
    assert len(tracker.lifecycle(flag[:0], field[:0], wrow)) == 0
    flag[2, 10:14, 70:] = 7
    flag[2, 10:12, :3] = 7
    flag[3, 5, 5] = -4                                            # any non-zero id counts (labels != 0, contrack.py:866)
    fd, vd = tracker.malloc(flag.nbytes), tracker.malloc(field.nbytes)
    try:
        tracker.h2d(fd, flag)
        tracker.h2d(vd, field)
        rows = tracker.lifecycle_dev(fd, vd, T, ny, nx, wrow)
    finally:
        tracker.free(fd)
        tracker.free(vd)
    want = life_util.numpy_rows(flag, field, wrow)
    assert [tuple(r)[:3] for r in rows] == [tuple(r)[:3] for r in want] == [(3, -4, -1), (2, 7, 70)]
    assert np.array_equal(rows["area"], want["area"]) and np.allclose(rows["swvx"], want["swvx"], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(40))
def test_hip_lifecycle_random_frames(tracker, i):
    """random label planes (thin contours whose centre of mass is an integer up to rounding included): the frame equals
    the scipy port's in every column, digit for digit"""
    flag, field, lat, lon, wrow, dates = life_util.random_life_case(i)
    rows = tracker.lifecycle(flag, field, wrow)
    got = lifecycle_frame(rows, lat, lon, dates, tracker)
    assert got == lifecycle_port.run_lifecycle(flag, field, lat, lon, wrow, dates)
    # ... and with EVERY row re-evaluated in the reference's summation orders on the device: the sums themselves are the
    # reference's, bit for bit (np.sum pairwise for area / intensity, np.bincount sequential for the centre of mass)
    ex = tracker.lifecycle_exact(np.arange(len(rows)))
    want = life_util.numpy_exact_rows(flag, field, wrow, rows)
    for k in ("area", "swv", "s", "sy", "sx"):
        assert np.array_equal(ex[k], want[k]), k


@pytest.mark.gpu
def test_hip_lifecycle_limits(tracker):
    ny, nx = 40, 64
    wrow = row_weights(np.linspace(60, 21, ny, dtype=np.float32), 1.0, 1.0)
    flag = np.zeros((1, ny, nx), dtype=np.int32)
    flag[0, ::2, ::2] = np.arange(1, 20 * 32 + 1).reshape(20, 32)          # 640 ids in one time step: more than the LDS tables hold,
    rows = tracker.lifecycle(flag, np.ones(flag.shape, np.float32), wrow)   # processed in passes over residue classes of the ids
    want = life_util.numpy_rows(flag, np.ones(flag.shape, np.float32), wrow)
    assert len(rows) == 640 and np.array_equal(rows["label"], want["label"]) and np.array_equal(rows["area"], want["area"])
    big = np.zeros((2, ny, nx), dtype=np.int32)
    big[1] = np.arange(1, ny * nx + 1).reshape(ny, nx)                      # 2560 ids, every one its own pixel; 40 of them touch both seam columns? no: one column each
    big[1, :, -1] = big[1, :, 0]                                            # ... now 40 ids cross the seam (more than the 32 column bit sets)
    rows = tracker.lifecycle(big, np.ones(big.shape, np.float32), wrow)
    want = life_util.numpy_rows(big, np.ones(big.shape, np.float32), wrow)
    assert len(rows) == len(want) and np.array_equal(rows["label"], want["label"]) and np.array_equal(rows["shift"], want["shift"])
    assert np.array_equal(rows["area"], want["area"]) and np.allclose(rows["swvx"], want["swvx"], rtol=1e-12)
    flag[0, ::2, ::2] = np.arange(1, 20 * 32 + 1).reshape(20, 32) % 500 + 1 # 500 ids: fits in one pass
    rows = tracker.lifecycle(flag, np.ones(flag.shape, np.float32), wrow)
    assert len(rows) == 500
    want = life_util.numpy_rows(flag, np.ones(flag.shape, np.float32), wrow)
    assert np.array_equal(rows["area"], want["area"]) and np.allclose(rows["swvy"], want["swvy"], rtol=1e-12)
    with pytest.raises(ValueError):
        tracker.lifecycle(flag, np.ones((1, ny, nx + 1), np.float32), wrow)


# ---------------------------------------------------------------------------------------------------------------
# large contours: numpy's np.sum tree (blocks of 8192, leaves of <= 128) and the exact path on contours that reach its hard cases
# ---------------------------------------------------------------------------------------------------------------
def _values(rng, n):
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)


def test_np_tree_sum_is_numpy_sum():
    rng = np.random.default_rng(11)
    for n in life_util.sweep_lengths() + life_util.edge_lengths() + life_util.round_lengths() + [105000, 721 * 1440]:
        a = _values(rng, n)
        assert life_util.np_tree_sum(a) == np.sum(a), n
        lv = life_util.np_leaves(n)
        assert lv[0][0] == 0 and all(o + m == o2 for (o, m), (o2, _) in zip(lv, lv[1:])) and sum(m for _, m in lv) == n


def test_np_leaves_at_most_65_per_block():
    """the bound wg_np_sum2 relies on: 441 block lengths (7689..8191) have 65 leaves, none has more, 8192 has 64"""
    counts = np.array([len(life_util.np_leaves(n)) for n in range(1, 8193)])
    assert counts.max() == 65 and (counts == 65).sum() == 441
    l65 = life_util.leaf_lengths(65)
    assert len(l65) == 441 and l65[0] == 7689 and l65[-1] == 8191
    assert counts[8191] == 64 and len(life_util.np_leaves(8192 * 3 + 8191)) == 3 * 64 + 65


@pytest.mark.parametrize("grid,kind", [("1deg", "raster"), ("1deg", "band"), ("1deg", "full"), ("0.25deg", "raster")])
def test_large_cases_have_the_prescribed_shapes(grid, kind):
    lengths = ([7689, 8191, 8192, 16383] if grid == "1deg" else life_util.round_lengths()[-4:] + [721 * 1440]) + life_util.edge_lengths()
    c = life_util.large_life_case(lengths, grid, kind, seed=3)
    flag, (ny, nx) = c["flag"], c["flag"].shape[1:]
    for ident, L in zip(c["ids"], c["lengths"]):
        assert (flag == ident).sum() == L
    rows = life_util.numpy_rows(flag, c["field"], c["wrow"])
    big = rows[np.isin(rows["label"], c["ids"][c["lengths"] >= 2 * nx])]
    assert len(big) >= 4
    if kind == "raster":
        assert (big["shift"] == 1).all()                                   # both seam columns, every column occupied
    elif kind == "band":
        assert (big["shift"] > 1).all()                                    # across the seam, rolled order != raster order
    else:
        for r in big:
            assert (flag[r["t"]] == r["label"]).any(axis=1).all()          # every row, the pole rows included
        assert (big["shift"] > 1).sum() >= 1
    assert (c["field"] < 0).any() and np.ptp(np.log10(np.abs(c["field"][flag != 0]))) > 10


@pytest.mark.parametrize("grid,kind,dtype", [("1deg", "raster", np.float32), ("1deg", "band", np.float64), ("0.25deg", "band", np.float32)])
def test_large_cases_tell_summation_orders_apart(grid, kind, dtype):
    """a kernel that summed in another order than numpy's would fail on these values: np.sum differs from the sequential sum, above
    8192 from the unblocked pairwise sum, and np.bincount's sequential sums over the rolled list from np.sum of that list"""
    lengths = life_util.sweep_lengths()[::8] + life_util.edge_lengths() if grid == "1deg" else \
        life_util.round_lengths() + [105000] + [8192 * k + r for k in (1, 2, 5) for r in (100, 3000, 5000)]
    c = life_util.large_life_case(lengths, grid, kind, dtype=dtype, seed=4)
    flag, field = c["flag"], c["field"]
    rows = life_util.numpy_rows(flag, field, c["wrow"])
    ex = life_util.numpy_exact_rows(flag, field, c["wrow"], rows, extent=True)
    wgrid = np.ones(flag.shape[1:]) * c["wrow"].astype(np.float64)[:, None]
    seq, unblocked, rolled = [], [], []
    for r, e in zip(rows, ex):
        m = flag[r["t"]] == r["label"]
        p = wgrid[m] * field[r["t"]][m]
        assert e["swv"] == np.sum(p)
        if len(p) >= 129:
            seq.append(np.sum(p) != life_util.seq_sum(p))
        if len(p) > 8192 and not 16384 <= len(p) < 16400:                  # (there the unblocked tree's first split is at 8192: the same tree)
            unblocked.append(np.sum(p) != life_util.np_tree_sum(p, block=None))
        sh = int(r["shift"]) if r["shift"] > 0 else 0
        pr = np.roll(np.where(m, field[r["t"]].astype(np.float64), 0.0) * wgrid, -sh, axis=1)[np.roll(m, -sh, axis=1)]
        assert e["s"] == life_util.seq_sum(pr)
        rolled.append(e["s"] != np.sum(pr))
    assert len(seq) >= 10 and np.mean(seq) >= 2 / 3
    assert np.mean(rolled) >= 2 / 3
    if grid != "1deg":
        assert len(unblocked) >= 10 and np.mean(unblocked) >= 2 / 3


def _check_exact(tracker, c, idx=None):
    """lifecycle_exact on rows idx (default: all) of the last lifecycle call equals numpy's own calls bit for bit"""
    rows = life_util.numpy_rows(c["flag"], c["field"], c["wrow"])
    idx = np.arange(len(rows)) if idx is None else np.asarray(idx)
    ex = tracker.lifecycle_exact(idx)
    want = life_util.numpy_exact_rows(c["flag"], c["field"], c["wrow"], rows[idx], extent=True)
    for k in ("area", "swv", "s", "sy", "sx"):
        bad = np.nonzero(ex[k] != want[k])[0]
        assert len(bad) == 0, (k, len(bad), "pixel counts", [int((c["flag"][rows[idx[i]]["t"]] == rows[idx[i]]["label"]).sum()) for i in bad[:8]])


def _large_rows(tracker, c):
    """tracker.lifecycle on a large case: t / label / shift as numpy_rows, the area as math.fsum of the weights (exact: integer
    limbs, rounded once)"""
    import math
    rows = tracker.lifecycle(c["flag"], c["field"], c["wrow"])
    want = life_util.numpy_rows(c["flag"], c["field"], c["wrow"])
    for k in ("t", "label", "shift"):
        assert np.array_equal(rows[k], want[k]), k
    w64 = c["wrow"].astype(np.float64)
    fs = [math.fsum(np.repeat(w64, (c["flag"][r["t"]] == r["label"]).sum(axis=1))) for r in rows]
    assert np.array_equal(rows["area"], np.array(fs))
    return rows, want


LARGE = [("1deg", kind, dt, False) for kind in ("raster", "band", "full") for dt in (np.float32, np.float64)] + \
        [("0.25deg", kind, dt, False) for kind in ("raster", "band", "full") for dt in (np.float32, np.float64)] + \
        [("1deg", "band", np.float64, True), ("0.25deg", "raster", np.float32, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("grid,kind,dtype,positive", LARGE)
def test_hip_lifecycle_exact_large_contours(tracker, grid, kind, dtype, positive):
    """1 deg: every length 7600..8192 (the 441 block lengths with 65 leaves among them) and the block edges of the sequential sums,
    256-thread launch; 0.25 deg: 8192 k + r (k = 1, 2, 3, 4, 12; r = 0, 1, 7689, 8191), the 105 000 pixels of DESIGN 9 and (raster)
    the whole plane, 1024-thread launch"""
    if grid == "1deg":
        lengths = life_util.sweep_lengths() + life_util.edge_lengths()
    else:
        lengths = life_util.round_lengths() + [105000] + ([721 * 1440] if kind == "raster" else [])
    c = life_util.large_life_case(lengths, grid, kind, dtype=dtype, positive=positive, seed=len(lengths) + 7 * positive)
    rows, want = _large_rows(tracker, c)
    if positive:
        for k in ("swv", "swvy", "swvx"):
            assert np.allclose(rows[k], want[k], rtol=1e-12, atol=0), k
    _check_exact(tracker, c)


@pytest.mark.gpu
def test_hip_lifecycle_exact_launch_shapes(tracker):
    """the same rows under the 256-thread launch (no listed row above 8192 pixels) and the 1024-thread one (a row of 8192 + 8191
    listed with them), in order, permuted and with duplicates"""
    small = life_util.edge_lengths() + [7600, 7688, 7689, 7690, 7900, 8190, 8191, 8192]
    c = life_util.large_life_case(small + [8192 + 8191], "1deg", "band", dtype=np.float64, seed=21)
    rows, _ = _large_rows(tracker, c)
    counts = np.array([(c["flag"][r["t"]] == r["label"]).sum() for r in rows])
    i_small, i_big = np.nonzero(counts <= 8192)[0], np.nonzero(counts > 8192)[0]
    assert len(i_big) == 1 and len(i_small) == len(small)
    _check_exact(tracker, c, i_small)                                       # 256 threads
    _check_exact(tracker, c)                                                # 1024 threads, every row
    rng = np.random.default_rng(5)
    _check_exact(tracker, c, rng.permutation(len(rows)))
    _check_exact(tracker, c, np.concatenate([i_big, i_small[::-1], i_small[-3:], i_big]))


@pytest.mark.gpu
@pytest.mark.parametrize("nx", [767, 768, 769, 1537])
def test_hip_lifecycle_exact_row_widths(tracker, nx):
    """rows of one batch of k_life_rows / k_life_lists (768 = LR_U x 64 columns), one column past it, and three batches"""
    for kind, dtype in (("raster", np.float32), ("band", np.float64)):
        c = life_util.large_life_case([129, 513, nx, 7689, 8191, 8192, 16383, 2 * nx + 1], (41, nx), kind, dtype=dtype, seed=nx)
        rows, _ = _large_rows(tracker, c)
        assert (rows["shift"] > 0).sum() >= 4
        _check_exact(tracker, c)


@pytest.mark.gpu
def test_hip_big_golden_rows_take_the_exact_path(tracker):
    """the 'big' golden: contours of 7689, 8191 and 8192 + 8191 pixels whose intensity sits on a half cent go through
    lifecycle_exact, and the frame is the reference's"""
    from contrack_amd.contrack import lifecycle_columns
    g = life_util.load("big")
    rows = tracker.lifecycle(g["flag"], g["variable"], g["wrow"])
    seen = []

    class Recorder:
        def lifecycle_exact(self, idx):
            seen.extend(int(i) for i in idx)
            return tracker.lifecycle_exact(idx)
    cols = lifecycle_columns(rows, g["lat"], g["lon"], life_util.dates_of(g["time"]), Recorder())
    counts = sorted({int((g["flag"][r["t"]] == r["label"]).sum()) for r in rows[seen]})
    assert sorted(set(seen)) == list(range(len(rows))) and counts == [7689, 8191, 16383]
    got = [(int(f), d, int(lo), int(la), float(it), float(sz)) for f, d, lo, la, it, sz in
           zip(cols["Flag"], cols["Date"], cols["Longitude"], cols["Latitude"], cols["Intensity"], cols["Size"])]
    assert got == g["frame"]
