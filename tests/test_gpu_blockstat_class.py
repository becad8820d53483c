"""contrack.calc_block_stats on the xarray stand-in (tests/minixr.py): run_contrack on a small synthetic slab, the life-cycle frame with
its index columns, then the peak and extent of every row of it against the statement of tests/blockstat_util.py fed with a table
built here from the frame's own Flag / Step columns -- equal everywhere, the two floats bit for bit."""
import functools

import numpy as np
import pytest

import blockstat_util as bu
import minixr
import subset_util as su
from contrack_amd import contrack as cm
from contrack_amd import synth

minixr.install_as_xarray()
pytestmark = pytest.mark.gpu
TLL = ("time", "latitude", "longitude")
T, NY, NX = 24, 45, 90                                                          # a 4-degree grid, 88 N .. 88 S (the other class tests' slab)
LAT, LON = 88.0 - 4.0 * np.arange(NY), 4.0 * np.arange(NX)
SINGLE = 7777                                                                   # an id put on ONE grid row by hand


def _time(n=T):
    return (np.datetime64("2001-01-01") + np.arange(n)).astype("datetime64[D]").astype("datetime64[ns]")


def _data(a):
    return np.asarray(a.data)


def _instance(anom, flag, dims=TLL):
    ds = minixr.make_dataset(anom, LAT, LON, time=_time())
    ds["time"].attrs = {}
    ds["flag"] = minixr.DataArray(flag.transpose([TLL.index(d) for d in dims]), dims, attrs={"units": "1"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c


@functools.lru_cache(maxsize=None)
def tracked(seed=5):
    """(anom, flag, the frame with index columns) of one tracked synthetic slab; the flag also holds SINGLE on seven pixels of one row,
    over the date line, where nothing was tracked"""
    anom = synth.smooth_field(T, NY, NX, seed=seed)
    ds = minixr.make_dataset(anom, LAT, LON, time=_time())
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    c.run_contrack(variable='anom', threshold=100.0, gorl='>=', overlap=0.4, persistence=3)
    flag = _data(c.ds["flag"]).astype(np.int32)
    cols = [NX - 3, NX - 2, NX - 1, 0, 1, 2, 3]
    free = [(t, r) for t in range(T) for r in range(5, NY - 5) if not flag[t, r, cols].any() and (anom[t, r, cols] > 1).all()]
    assert free, "a free stretch of positive values over the date line"
    t, r = free[0]
    flag[t, r, cols] = SINGLE
    df = _instance(anom, flag).run_lifecycle("flag", "anom", indices=True)
    assert len(df) >= 12 and len(df.Flag.unique()) >= 3, "the synthetic slab must give a few blocks of a few steps"
    return anom, flag, df


def expected(flag, x, ids, steps, want=bu.SHAPE | bu.PEAKS):
    """the statement's row of every (id, flat step) pair, in the pairs' order"""
    slices = [sorted(set(int(i) for i, s in zip(ids, steps) if s == t)) for t in range(flag.shape[0])]
    off, tab = su.table_by_row(slices)
    rows = bu.blockstat(flag, x, off, tab, want=want)
    return rows[[int(off[s]) + slices[s].index(int(i)) for i, s in zip(ids, steps)]]


def check_frame(df, rows, frame, variable=True):
    """every column of calc_block_stats(indices=True) from the statement's rows"""
    assert len(df) == len(rows) == len(frame) and (rows["n"] > 0).all()
    for k in ("Flag", "Date", "Step"):
        assert np.array_equal(df[k].to_numpy(), frame[k].to_numpy()), k
    r0, r1, west, width = (rows[k].astype(np.int64) for k in ("r0", "r1", "west", "width"))
    want = {"N": rows["n"], "Row0": r0, "Row1": r1, "ColWest": west, "Width": width, "South": LAT[r0], "North": LAT[r1], "LatExtent": (r1 - r0 + 1) * 4.0,
            "West": LON[west], "East": LON[(west + width - 1) % NX], "LonExtent": width * 4.0}
    if variable:
        assert (rows["nv"] > 0).all()
        want.update({"NValid": rows["nv"]})
        for name in ("max", "min"):
            p, cap = rows[name + "_p"], name.capitalize()
            want.update({cap: rows[name], cap + "Row": p // NX, cap + "Col": p % NX, cap + "Latitude": LAT[p // NX], cap + "Longitude": LON[p % NX]})
    for k, v in want.items():
        got = df[k].to_numpy()
        if got.dtype == np.float64:
            assert np.array_equal(got.view(np.uint64), np.asarray(v, dtype=np.float64).view(np.uint64)), k
        else:
            assert got.dtype.kind == "i" and np.array_equal(got, v), k
    assert set(want) <= set(df.columns)


def test_every_row_of_the_life_cycle_frame():
    anom, flag, df = tracked()
    c = _instance(anom, flag)
    rows = expected(flag, anom, df["Flag"], df["Step"])
    got = c.calc_block_stats("flag", "anom", frame=df, indices=True)
    check_frame(got, rows, df)
    assert list(got.columns)[:4] == ["Flag", "Date", "Step", "N"] and "Row" not in got.columns
    assert (rows["width"] < NX).any() and (rows["r1"] > rows["r0"]).any()
    # the peak brackets the area mean: the weights are positive.  Intensity is rounded to two decimals (the reference's frame), and
    # rounding is monotonic, so it lies between the equally rounded extremes -- exactly, for every row
    it = df["Intensity"].to_numpy()
    assert (np.round(got["Min"].to_numpy(), 2) <= it).all() and (it <= np.round(got["Max"].to_numpy(), 2)).all()
    assert (got["Max"].to_numpy() > got["Min"].to_numpy()).any()
    # a block on a single grid row: its area is its pixel count times that row's weight, to the frame's rounding of Size
    one = got[got["Flag"] == SINGLE]
    assert len(one) == 1 and int(one["Row0"].iloc[0]) == int(one["Row1"].iloc[0]) and int(one["N"].iloc[0]) == 7
    w = float(cm.row_weights(LAT, c._dlat, c._dlon)[int(one["Row0"].iloc[0])])
    size = float(df[df["Flag"] == SINGLE]["Size"].iloc[0])
    assert abs(size - 7 * w) <= 0.005 + 1e-6 * 7 * w, (size, 7 * w)              # (round(, 2), and float32 weights summed in float64)
    # ... and it lies over the date line: seven columns wide, not NX
    assert (int(one["ColWest"].iloc[0]), int(one["Width"].iloc[0]), float(one["West"].iloc[0]), float(one["East"].iloc[0]), float(one["LonExtent"].iloc[0])) == \
        (NX - 3, 7, LON[NX - 3], LON[3], 28.0)
    # without indices, without a variable, a selection in another order
    plain = c.calc_block_stats("flag", "anom", frame=df)
    assert list(plain.columns) == ["Flag", "Date", "Step", "N", "South", "North", "LatExtent", "West", "East", "LonExtent", "Max", "MaxLatitude", "MaxLongitude",
                                   "Min", "MinLatitude", "MinLongitude"] and plain.equals(got[list(plain.columns)])
    some = df.iloc[::-2]
    shape = c.calc_block_stats("flag", frame=some, indices=True)
    check_frame(shape, expected(flag, None, some["Flag"], some["Step"], bu.SHAPE), some, variable=False)
    assert "Max" not in shape.columns


def test_frame_none_chunk_steps_and_permuted_dims():
    anom, flag, df = tracked()
    rows = expected(flag, anom, df["Flag"], df["Step"])
    c = _instance(anom, flag)
    check_frame(c.calc_block_stats("flag", "anom", indices=True), rows, df)         # frame=None: run_lifecycle is called first
    for chunk in (5, 0, T + 3):
        check_frame(c.calc_block_stats("flag", "anom", frame=df, chunk_steps=chunk, indices=True), rows, df)
    dims = ("latitude", "time", "longitude")
    c = _instance(anom, flag, dims)
    for chunk in (None, 7):
        check_frame(c.calc_block_stats("flag", "anom", frame=df, chunk_steps=chunk, indices=True), rows, df)
    assert tuple(c.ds["flag"].dims) == dims and set(c.variables) >= {"flag", "anom"}


@pytest.mark.parametrize("dims", [("member", "time", "latitude", "longitude"), ("time", "latitude", "member", "longitude")])
def test_member_dimension(dims):
    canon = ("member", "time", "latitude", "longitude")
    (a0, f0, _), (a1, f1, _) = tracked(5), tracked(7)
    flag4 = np.stack([f0, np.where(f1 > 0, f1 + 10000, 0)]).astype(np.int32)
    order = [canon.index(d) for d in dims]
    ds = minixr.make_dataset(a0, LAT, LON, time=_time())
    ds["time"].attrs = {}
    ds["member"] = minixr.DataArray(np.array([20, 10]), ("member",), attrs={})       # (not sorted: the values are looked up)
    ds["flag"] = minixr.DataArray(flag4.transpose(order), dims)
    ds["z"] = minixr.DataArray(np.stack([a0, a1]).transpose(order), dims, attrs={"units": "m"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    df = c.run_lifecycle("flag", "z", indices=True)
    assert set(df["member"]) == {10, 20}
    m = np.where(df["member"].to_numpy() == 20, 0, 1)
    flat, zflat = flag4.reshape(2 * T, NY, NX), np.stack([a0, a1]).reshape(2 * T, NY, NX)
    rows = expected(flat, zflat, df["Flag"], m * T + df["Step"].to_numpy())
    for chunk in (None, 5):                                                       # (a chunk of 5 flat steps spans the member break at 24)
        got = c.calc_block_stats("flag", "z", frame=df, chunk_steps=chunk, indices=True)
        assert list(got.columns)[:5] == ["Flag", "Date", "member", "Step", "N"] and np.array_equal(got["member"].to_numpy(), df["member"].to_numpy())
        check_frame(got.drop(columns=["member"]), rows, df)
    with pytest.raises(ValueError):
        c.calc_block_stats("flag", "z", frame=df.drop(columns=["member"]))
    with pytest.raises(ValueError):
        c.calc_block_stats("flag", "z", frame=df.assign(member=30))


def test_check_raises_on_a_foreign_row():
    anom, flag, df = tracked()
    c = _instance(anom, flag)
    free = int(flag.max()) + 5
    foreign = df.copy()
    foreign.iloc[0, foreign.columns.get_loc("Flag")] = free
    with pytest.raises(ValueError, match="id {}".format(free)):
        c.calc_block_stats("flag", "anom", frame=foreign)
    moved = df.copy()
    moved["Step"] = (moved["Step"] + 11) % T                                      # right ids, wrong days
    with pytest.raises(ValueError, match="another run"):
        c.calc_block_stats("flag", "anom", frame=moved)
    got = c.calc_block_stats("flag", "anom", frame=foreign, check=False, indices=True)
    assert got["N"].iloc[0] == 0 and np.isnan(got["Max"].iloc[0]) and np.isnan(got["West"].iloc[0]) and got["Width"].iloc[0] == 0
    check_frame(got.iloc[1:].reset_index(drop=True), expected(flag, anom, df["Flag"][1:], df["Step"][1:]), df.iloc[1:].reset_index(drop=True))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_anomaly_after_calc_anom(monkeypatch, dtype):
    """the anomaly calc_anom left in HBM is the field: blockstat_numpy gets x = None, only the flags are uploaded -- the same rows as
    the call with the host array"""
    raw, flag, df = tracked()
    ds = minixr.make_dataset(raw.astype(dtype), LAT, LON, time=_time(), var="z", time_units="days since 2001-01-01")
    ds["flag"] = minixr.DataArray(flag, TLL, attrs={"units": "1"})
    c = cm.contrack(ds=ds)
    c.calc_anom("z", window=1, smooth=1, groupby="month")
    anom = _data(c.ds["anom"])
    assert anom.dtype == dtype
    rows = expected(flag, anom, df["Flag"], df["Step"])
    seen = []
    inner = cm.blockstat_numpy

    def spy(flag, table, x=None, **kw):
        seen.append(x is None)
        return inner(flag, table, x, **kw)
    monkeypatch.setattr(cm, "blockstat_numpy", spy)
    check_frame(c.calc_block_stats("flag", "anom", frame=df, indices=True), rows, df)
    keep, c._anom_resident = c._anom_resident, None                                # the host-array path
    check_frame(c.calc_block_stats("flag", "anom", frame=df, indices=True), rows, df)
    c._anom_resident = keep
    check_frame(c.calc_block_stats("flag", "z", frame=df, indices=True), expected(flag, raw.astype(dtype), df["Flag"], df["Step"]), df)
    assert seen == [True, False, False]
