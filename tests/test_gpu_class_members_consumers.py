"""The two consumers of 'flag' on what run_contrack(segments=<dim>, chunk_steps=...) writes: run_lifecycle and calc_frequency of
the class over a member dimension (both dim orders) and with the variables read slice by slice, through the duck-typed dataset of
tests/minixr.py.  Members: the golden slabs smooth0 / smooth1 / smooth2 with their own variables, ids offset by 1000 per member."""
import functools

import numpy as np
import pytest

import freq_util
import life_util
import minixr
from contrack_amd import contrack as cm
from oracle import lifecycle_port

minixr.install_as_xarray()
pytestmark = pytest.mark.gpu
MEMBERS = ("smooth0", "smooth1", "smooth2")
CANON = ("member", "time", "latitude", "longitude")
ORDERS = [CANON, ("time", "member", "latitude", "longitude")]
COLUMNS = ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']


@functools.lru_cache(maxsize=None)
def members():
    gs = [life_util.load(n) for n in MEMBERS]
    for g in gs:
        assert g["flag"].shape == (16, 46, 72)
        assert np.array_equal(g["lat"], gs[0]["lat"]) and np.array_equal(g["lon"], gs[0]["lon"]) and np.array_equal(g["time"], gs[0]["time"])
        assert 0 <= g["flag"].min() and g["flag"].max() < 1000
    flag = np.stack([np.where(g["flag"] != 0, g["flag"] + 1000 * m, 0) for m, g in enumerate(gs)]).astype(np.int32)
    var = np.stack([g["variable"] for g in gs])
    return gs, flag, var


def dataset(dims, flag_dtype=np.int32, coordinate=True, flag=None):
    gs, flag4, var = members()
    flag4 = flag4 if flag is None else flag
    g = gs[0]
    ds = minixr.make_dataset(g["field"], g["lat"], g["lon"], time=g["time"])
    ds["time"].attrs = {}
    if coordinate:
        ds["member"] = minixr.DataArray(np.array([10, 20, 30]), ("member",), attrs={})
    order = [CANON.index(d) for d in dims]
    ds["flag"] = minixr.DataArray(flag4.astype(flag_dtype).transpose(order), dims)
    ds["z"] = minixr.DataArray(var.transpose(order), dims, attrs={"units": "m", "long_name": "z"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c


def single(m, flag_dtype=np.int32):
    gs, flag4, var = members()
    g = gs[m]
    ds = minixr.make_dataset(g["field"], g["lat"], g["lon"], time=g["time"])
    ds["time"].attrs = {}
    ds["flag"] = minixr.DataArray(flag4[m].astype(flag_dtype), ("time", "latitude", "longitude"))
    ds["z"] = minixr.DataArray(var[m], ("time", "latitude", "longitude"), attrs={"units": "m", "long_name": "z"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c


def _compare(got, want, tol=0.0101):                   # the standard of tests/test_lifecycle.py for stored frames
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a[:4] == b[:4], (a, b)
        assert abs(a[4] - b[4]) <= tol and abs(a[5] - b[5]) <= tol * max(1.0, abs(b[5]) * 1e-9), (a, b)


@functools.lru_cache(maxsize=None)
def wanted(values):
    """(the stored reference frames with the id offsets applied, concatenated; the port's frames, run per member; member column)"""
    gs, flag4, var = members()
    c = dataset(CANON)
    wrow = cm.row_weights(gs[0]["lat"], c._dlat, c._dlon)
    dates = life_util.dates_of(gs[0]["time"])
    stored, port, col = [], [], []
    for m, g in enumerate(gs):
        stored += [(r[0] + 1000 * m,) + tuple(r[1:]) for r in g["frame"]]
        port += lifecycle_port.run_lifecycle(flag4[m], var[m], g["lat"], g["lon"], wrow, dates)
        col += [values[m]] * len(g["frame"])
    assert [r[0] for r in stored] == sorted(r[0] for r in stored)          # unique ids: (Flag, member, Date) is the reference's (Flag, Date)
    assert len(port) == len(stored)
    return stored, port, col


@pytest.mark.parametrize("chunk_steps", [None, 5])
@pytest.mark.parametrize("dims", ORDERS)
def test_run_lifecycle_over_members(dims, chunk_steps):
    """chunk_steps = 5: the chunk of flat steps 15..19 spans the member break at 16"""
    coordinate = dims == CANON
    c = dataset(dims, coordinate=coordinate)
    df = c.run_lifecycle("flag", "z", chunk_steps=chunk_steps)
    assert list(df.columns) == COLUMNS + ["member"]
    stored, port, col = wanted((10, 20, 30) if coordinate else (0, 1, 2))
    got = [tuple(r)[:6] for r in df.itertuples(index=False)]
    _compare(got, stored)
    assert got == port                                                     # digit for digit
    assert df["member"].tolist() == col


@pytest.mark.parametrize("chunk_steps", [None, 5])
def test_three_dims_still_give_six_columns(chunk_steps):
    gs, flag4, var = members()
    c = single(1)
    df = c.run_lifecycle("flag", "z", chunk_steps=chunk_steps)
    assert list(df.columns) == COLUMNS
    _compare([tuple(r) for r in df.itertuples(index=False)], [(r[0] + 1000,) + tuple(r[1:]) for r in gs[1]["frame"]])


@pytest.mark.parametrize("groupby", [None, "month"])
@pytest.mark.parametrize("dims", ORDERS)
def test_frequency_per_member(dims, groupby):
    c = dataset(dims)
    ref = c.calc_frequency("flag", groupby=groupby, above=0)
    want_dims = tuple(groupby if d == "time" else d for d in dims if d != "time" or groupby is not None)
    assert tuple(ref.dims) == want_dims
    assert np.array_equal(np.asarray(ref.coords["member"]), [10, 20, 30])
    data = np.asarray(ref.data)
    for m in range(3):
        one = single(m).calc_frequency("flag", groupby=groupby, above=0)
        part = np.take(data, m, axis=want_dims.index("member"))
        assert freq_util.same_bits(part, np.asarray(one.data))
        assert tuple(one.dims) == tuple(d for d in want_dims if d != "member")
    assert (data > 0).any()
    for steps in (1, 5, 100):
        assert freq_util.same_bits(np.asarray(c.calc_frequency("flag", groupby=groupby, chunk_steps=steps).data), data)


@pytest.mark.parametrize("groupby", [None, "month"])
@pytest.mark.parametrize("dims", ORDERS)
def test_frequency_pooled(dims, groupby):
    gs, flag4, var = members()
    c = dataset(dims)
    pooled = c.calc_frequency("flag", groupby=groupby, pool=True)
    assert "member" not in pooled.dims
    flat = flag4.reshape((-1,) + flag4.shape[2:])
    ids = None if groupby is None else np.tile(c._group_ids(groupby)[0], 3)
    want = cm.frequency_numpy(flat, ids)
    sort = [(((groupby,) if groupby else ()) + ("latitude", "longitude")).index(d) for d in pooled.dims]
    assert freq_util.same_bits(np.asarray(pooled.data), want.transpose(sort))
    if groupby is not None:                                                 # a group's size: its size x members
        n = np.bincount(ids)
        assert freq_util.same_bits(want, freq_util.percent(flat, ids, len(n)))
    for steps in (1, 5, 100):
        assert freq_util.same_bits(np.asarray(c.calc_frequency("flag", groupby=groupby, pool=True, chunk_steps=steps).data), np.asarray(pooled.data))


def test_frequency_three_dims_chunked_and_pool_ignored():
    c = single(2)
    ref = np.asarray(c.calc_frequency("flag", groupby="month").data)
    assert freq_util.same_bits(np.asarray(c.calc_frequency("flag", groupby="month", pool=True).data), ref)
    for steps in (1, 5, 100):
        assert freq_util.same_bits(np.asarray(c.calc_frequency("flag", groupby="month", chunk_steps=steps).data), ref)


def test_int64_flags_are_narrowed_chunk_by_chunk():
    gs, flag4, var = members()
    c = dataset(CANON, flag_dtype=np.int64)
    df = c.run_lifecycle("flag", "z", chunk_steps=5)
    stored, port, col = wanted((10, 20, 30))
    assert [tuple(r)[:6] for r in df.itertuples(index=False)] == port
    ref = np.asarray(dataset(CANON).calc_frequency("flag").data)
    assert freq_util.same_bits(np.asarray(c.calc_frequency("flag", chunk_steps=5).data), ref)
    big = flag4.astype(np.int64)
    big[2, 15, 3, 4] = 2 ** 31                                             # flat step 47: the last chunk
    c = dataset(CANON, flag_dtype=np.int64, flag=big)
    seen = []
    inner = c._steps

    def spying(da, step_dims, level=None):                                 # every reader the class builds, through its view
        view = inner(da, step_dims, level)
        build = view.reader

        def reader(integer=False, **kwargs):
            read = build(integer=integer, **kwargs)

            def spy(t0, nt, out):
                seen.append((integer, t0))
                read(t0, nt, out)
            return spy
        view.reader = reader
        return view
    c._steps = spying
    with pytest.raises(ValueError, match="flag ids beyond int32"):
        c.run_lifecycle("flag", "z", chunk_steps=5)
    assert max(t0 for integer, t0 in seen if integer) == 45                  # raised from the chunk that holds it
    with pytest.raises(ValueError, match="flag ids beyond int32"):
        c.calc_frequency("flag", chunk_steps=5)
    with pytest.raises(ValueError, match="flag ids beyond int32"):
        c.run_lifecycle("flag", "z")
