"""contrack.select_blocks on the xarray stand-in (tests/minixr.py): run_contrack on a small synthetic slab, the life-cycle frame with
its index columns, then the flag restricted to chosen tracks or to rows of the frame against the statement of tests/subset_util.py fed
with a table built here from the frame's own Flag / Step columns -- equal everywhere, all integers."""
import functools

import numpy as np
import pytest

import minixr
import subset_util as su
from contrack_amd import contrack as cm
from contrack_amd import synth

minixr.install_as_xarray()
pytestmark = pytest.mark.gpu
TLL = ("time", "latitude", "longitude")
T, NY, NX = 24, 45, 90                                                          # a 4-degree grid, 88 N .. 88 S
LAT, LON = 88.0 - 4.0 * np.arange(NY), 4.0 * np.arange(NX)


def _time(n=T):
    return (np.datetime64("2001-01-01") + np.arange(n)).astype("datetime64[D]").astype("datetime64[ns]")


def _data(a):
    return np.asarray(a.data)


@functools.lru_cache(maxsize=None)
def tracked(seed=5):
    """(anom, flag, the frame with index columns) of one tracked synthetic slab"""
    anom = synth.smooth_field(T, NY, NX, seed=seed)
    ds = minixr.make_dataset(anom, LAT, LON, time=_time())
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    c.run_contrack(variable='anom', threshold=100.0, gorl='>=', overlap=0.4, persistence=3)
    df = c.run_lifecycle("flag", "anom", indices=True)
    assert len(df) >= 12 and len(df.Flag.unique()) >= 2, "the synthetic slab must give a few blocks of a few steps"
    return anom, _data(c.ds["flag"]).astype(np.int32), df


def instance(dims=TLL):
    anom, flag, df = tracked()
    ds = minixr.make_dataset(anom, LAT, LON, time=_time())
    ds["time"].attrs = {}
    ds["flag"] = minixr.DataArray(flag.transpose([TLL.index(d) for d in dims]), dims, attrs={"units": "1"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c, flag, df


def row_table(flags, steps, nsteps):
    return su.table_by_row([sorted(set(int(f) for f, s in zip(flags, steps) if s == t)) for t in range(nsteps)])


def sector(df):
    """the rows whose centre lies in 0 .. 180 E"""
    rows = df[(df["Longitude"] >= 0) & (df["Longitude"] < 180)]
    assert 0 < len(rows) < len(df)
    return rows


def test_chosen_tracks():
    c, flag, df = instance()
    ids = sorted(df.Flag.unique())[::2]
    want = su.subset_fast(flag, *su.table_by_id(ids))
    assert 0 < want[2] < np.count_nonzero(flag > 0)
    n = c.select_blocks(ids=ids[::-1] + ids[:1])                                  # (any order, duplicates)
    got = c.ds["flag_sel"]
    assert n == want[2] and tuple(got.dims) == TLL and _data(got).dtype == np.int32 and np.array_equal(_data(got), want[0])
    assert got.attrs["history"] == "Selected from flag with input attributes: {} ids, invert = False, out = id.".format(len(ids))
    assert np.array_equal(_data(c.ds["flag"]), flag)                              # the flag variable itself is left alone
    inv = su.subset_fast(flag, *su.table_by_id(ids), invert=True)
    assert c.select_blocks(ids=ids, invert=True, name="rest") == inv[2] == np.count_nonzero(flag > 0) - want[2]
    assert np.array_equal(_data(c.ds["rest"]), inv[0]) and np.array_equal(_data(c.ds["rest"]) + _data(got), np.where(flag > 0, flag, 0))
    assert c.select_blocks(ids=ids, out='mask', name="m") == want[2]
    assert np.array_equal(_data(c.ds["m"]), (want[0] > 0).astype(np.int32)) and "out = mask" in c.ds["m"].attrs["history"]


@pytest.mark.parametrize("invert", [False, True])
def test_rows_of_one_sector(invert):
    c, flag, df = instance()
    rows = sector(df)
    want = su.subset_fast(flag, *row_table(rows["Flag"], rows["Step"], T), invert=invert)
    by_id = su.subset_fast(flag, *su.table_by_id(sorted(rows.Flag.unique())), invert=invert)
    assert 0 < want[2] < np.count_nonzero(flag > 0) and not np.array_equal(want[0], by_id[0]), "some track leaves the sector: rows are not tracks"
    assert c.select_blocks(frame=rows, invert=invert) == want[2]
    assert np.array_equal(_data(c.ds["flag_sel"]), want[0])
    assert "{} rows".format(len(rows)) in c.ds["flag_sel"].attrs["history"]


def test_chunk_steps_gives_the_same_variable():
    c, flag, df = instance()
    rows = sector(df)
    n = c.select_blocks(frame=rows, name="a")
    for chunk in (5, 0, T + 3):
        assert c.select_blocks(frame=rows, name="b", chunk_steps=chunk) == n
        assert np.array_equal(_data(c.ds["a"]), _data(c.ds["b"])) and tuple(c.ds["b"].dims) == TLL


def test_permuted_dims_are_kept():
    dims = ("latitude", "time", "longitude")
    c, flag, df = instance(dims)
    rows = sector(df)
    want = su.subset_fast(flag, *row_table(rows["Flag"], rows["Step"], T))
    for chunk in (None, 7):
        assert c.select_blocks(frame=rows, chunk_steps=chunk) == want[2]
        got = c.ds["flag_sel"]
        assert tuple(got.dims) == dims and np.array_equal(_data(got), want[0].transpose(1, 0, 2))
        assert set(got.attrs) == {"units", "long_name", "history"}


@pytest.mark.parametrize("dims", [("member", "time", "latitude", "longitude"), ("time", "latitude", "member", "longitude")])
def test_member_dimension(dims):
    canon = ("member", "time", "latitude", "longitude")
    (a0, f0, _), (a1, f1, _) = tracked(5), tracked(7)
    flag4 = np.stack([f0, np.where(f1 > 0, f1 + 1000, 0)]).astype(np.int32)
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
    rows = sector(df)
    m = np.where(rows["member"].to_numpy() == 20, 0, 1)
    flat = flag4.reshape(2 * T, NY, NX)
    want = su.subset_fast(flat, *row_table(rows["Flag"], m * T + rows["Step"].to_numpy(), 2 * T))
    assert want[0][:T].any() and want[0][T:].any()
    for chunk in (None, 5):                                                       # (a chunk of 5 flat steps spans the member break at 24)
        assert c.select_blocks(frame=rows, chunk_steps=chunk) == want[2]
        got = c.ds["flag_sel"]
        assert tuple(got.dims) == dims and np.array_equal(_data(got), want[0].reshape(flag4.shape).transpose(order))
    ids = sorted(df.Flag.unique())[::2]
    assert c.select_blocks(ids=ids, name="t") == su.subset_fast(flat, *su.table_by_id(ids))[2]
    with pytest.raises(ValueError):
        c.select_blocks(frame=rows.drop(columns=["member"]))
    with pytest.raises(ValueError):
        c.select_blocks(frame=rows.assign(member=30))


def test_check_raises_on_a_foreign_row():
    c, flag, df = instance()
    rows = sector(df)
    free = int(flag.max()) + 5
    foreign = rows.copy()
    foreign.iloc[0, foreign.columns.get_loc("Flag")] = free
    with pytest.raises(ValueError, match="id {}".format(free)):
        c.select_blocks(frame=foreign)
    assert "flag_sel" not in c.variables
    moved = rows.copy()
    moved["Step"] = (moved["Step"] + 11) % T                                      # right ids, wrong days
    with pytest.raises(ValueError, match="another run"):
        c.select_blocks(frame=moved)
    with pytest.raises(ValueError, match=str(free)):
        c.select_blocks(ids=[free, int(df.Flag.iloc[0])])
    n = c.select_blocks(frame=foreign, check=False)
    want = su.subset_fast(flag, *row_table(foreign["Flag"], foreign["Step"], T))
    assert n == want[2] and np.array_equal(_data(c.ds["flag_sel"]), want[0])
    for kw in (dict(), dict(ids=[1], frame=rows), dict(ids=[1], out='both'), dict(ids=[0]), dict(frame=rows[["Flag"]])):
        with pytest.raises(ValueError):
            c.select_blocks(**kw)


def test_calc_frequency_of_the_selection():
    c, flag, df = instance()
    rows = sector(df)
    want = su.subset_fast(flag, *row_table(rows["Flag"], rows["Step"], T))[0]
    c.select_blocks(frame=rows, name="atlantic")
    freq = c.calc_frequency("atlantic")
    assert np.array_equal(_data(freq), cm.frequency_percent((want > 0).sum(axis=0)[None], [T])[0]) and _data(freq).any()
    assert np.array_equal(_data(freq), cm.frequency_numpy(want))
