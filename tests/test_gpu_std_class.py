"""contrack.std_field / contrack.std_threshold of the class on the GPU, on tests/minixr.py: labels, attrs, the band, k, the groupings,
pooled members, the resident anomaly slab, and the chain into run_contrack.  Expected values: tests/std_util.want_std, bit for bit."""
import numpy as np
import pytest

import minixr
import std_util
from contrack_amd import synth
from contrack_amd.contrack import contrack, row_weights, track_numpy

pytestmark = pytest.mark.gpu
minixr.install_as_xarray()

T, NY, NX = 48, 19, 24


def _same(got, ref, case):
    assert got.shape == ref.shape, (case, got.shape, ref.shape)
    assert np.array_equal(got, ref, equal_nan=True), (case, int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum()))


@pytest.fixture(scope="module")
def block():
    """(class instance on a synth slab of 48 daily steps over a new year, the slab, lat, lon, stamps): dayofyear 339 .. 365 and 1 .. 21"""
    lat, lon = synth.grid(NY, NX)
    a = synth.smooth_field(T, NY, NX, seed=9)
    a = (a - a.mean(axis=0)).astype(np.float32)
    a[5, 3, 7] = np.nan
    stamps = (np.datetime64("2001-12-05") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(a, lat, lon, time=stamps)
    ds["time"].attrs = {}
    ds["anom"].attrs.update({"units": "m"})
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c, a, lat, lon, stamps


def _ids(stamps, what):
    import pandas as pd
    return np.unique(np.asarray(getattr(pd.DatetimeIndex(stamps), what)), return_inverse=True)


def test_field_labels_attrs_band_and_k(block):
    c, a, lat, lon, stamps = block
    days, ids = _ids(stamps, "dayofyear")
    rows = np.nonzero((lat >= 30) & (lat <= 90))[0]
    y0, y1 = int(rows[0]), int(rows[-1]) + 1
    want = std_util.want_std(a, (y0, y1), ids, len(days), 5, 1, True)[0]
    f = c.std_field(variable="anom", k=1.5, groupby="dayofyear", window=5, lat_bounds=(30, 90), ddof=1)
    assert tuple(f.dims) == ("dayofyear", "latitude", "longitude") and f.name == "anom_std_field"
    assert np.array_equal(np.asarray(f["dayofyear"].data), days) and np.array_equal(np.asarray(f["latitude"].data), lat)
    assert np.array_equal(np.asarray(f["longitude"].data), lon)
    assert f.attrs["k"] == 1.5 and f.attrs["ddof"] == 1 and f.attrs["window"] == 5 and f.attrs["lat_bounds"] == (30.0, 90.0) and f.attrs["units"] == "m"
    assert "k = 1.5" in f.attrs["history"] and "window = 5 groups" in f.attrs["history"]
    v = np.asarray(f.data)
    assert v.shape == (len(days), NY, NX) and np.isnan(v[:, y1:]).all() and y0 == 0
    _same(v[:, y0:y1], 1.5 * want, "k = 1.5")
    neg = np.asarray(c.std_field(variable="anom", k=-2.0, groupby="dayofyear", window=5, lat_bounds=(30, 90), ddof=1).data)
    _same(neg[:, y0:y1], -2.0 * want, "k = -2")
    assert (neg[:, y0:y1][~np.isnan(want)] <= 0).all()
    plain = np.asarray(c.std_field(variable="anom", groupby="dayofyear", window=5, lat_bounds=(30, 90), skipna=False).data)
    _same(plain[:, y0:y1], std_util.want_std(a, (y0, y1), ids, len(days), 5, 0, False)[0], "skipna False")
    assert np.isnan(plain[:, 3, 7]).any() and not np.isnan(v[:, 3, 7]).all()


def test_groupings(block):
    c, a, lat, lon, stamps = block
    one = c.std_field(variable="anom", k=2.0, groupby=None)
    assert tuple(one.dims) == ("latitude", "longitude")
    _same(np.asarray(one.data), 2.0 * std_util.want_std(a, (0, NY), np.zeros(T, int), 1, 1, 0, True)[0][0], "groupby None")
    months, ids = _ids(stamps, "month")
    m = c.std_field(variable="anom", groupby="month", window=2, ddof=1)
    assert tuple(m.dims) == ("month", "latitude", "longitude") and np.array_equal(np.asarray(m["month"].data), months) and len(months) == 2
    _same(np.asarray(m.data), std_util.want_std(a, (0, NY), ids, 2, 2, 1, True)[0], "month")
    days, ids = _ids(stamps, "dayofyear")
    d = c.std_field(variable="anom", groupby="dayofyear", window=31)
    _same(np.asarray(d.data), std_util.want_std(a, (0, NY), ids, len(days), 31, 0, True)[0], "dayofyear")


def test_threshold_is_the_band_mean(block):
    c, a, lat, lon, stamps = block
    rows = np.nonzero((lat >= 50) & (lat <= 80))[0]
    band = (int(rows[0]), int(rows[-1]) + 1)
    thr = c.std_threshold(variable="anom", k=1.5)
    assert isinstance(thr, float) and thr == 1.5 * np.mean(std_util.want_std(a, band, np.zeros(T, int), 1, 1, 0, True)[0][0])
    days, ids = _ids(stamps, "dayofyear")
    per = c.std_threshold(variable="anom", k=-1.0, groupby="dayofyear", window=9, ddof=1, lat_bounds=(50, 80))
    want = std_util.want_std(a, band, ids, len(days), 9, 1, True)[0]
    assert tuple(per.dims) == ("dayofyear",) and np.array_equal(np.asarray(per["dayofyear"].data), days) and per.attrs["k"] == -1.0
    _same(np.asarray(per.data), np.array([-1.0 * np.mean(p) for p in want]), "per day")
    c.run_contrack(variable="anom", threshold=per, gorl="<=", overlap=0.5, persistence=2)          # a 1-D dayofyear threshold as it is
    wrow = row_weights(lat, c._dlat, c._dlon)
    flag, _ = track_numpy(a, wrow, np.asarray(per.data)[ids], "<=", 0.5, 2)
    assert np.array_equal(np.asarray(c.flag), flag)


def test_chain_into_run_contrack(block):
    c, a, lat, lon, stamps = block
    days, ids = _ids(stamps, "dayofyear")
    rows = np.nonzero((lat >= 20) & (lat <= 80))[0]
    y0, y1 = int(rows[0]), int(rows[-1]) + 1
    field = c.std_field(variable="anom", k=1.0, groupby="dayofyear", window=15, lat_bounds=(20, 80))
    c.run_contrack(variable="anom", threshold=field, gorl=">=", overlap=0.3, persistence=2)
    got = np.array(c.flag)
    whole = np.full((len(days), NY, NX), np.nan)
    whole[:, y0:y1] = std_util.want_std(a, (y0, y1), ids, len(days), 15, 0, True)[0]
    flag, n = track_numpy(a, row_weights(lat, c._dlat, c._dlon), whole[ids], ">=", 0.3, 2)
    assert np.array_equal(got, flag) and flag.max() > 0 and n > 0, ("flag", n)
    assert not got[:, :y0].any() and not got[:, y1:].any(), "rows outside the band are never flagged"


def test_members_are_pooled_in_the_order_of_the_flattened_slab():
    M = 3
    lat, lon = synth.grid(9, 16)
    stamps = (np.datetime64("2000-12-20") + np.arange(40)).astype("datetime64[ns]")
    rng = np.random.default_rng(2)
    x = (30.0 * rng.standard_normal((M, 40, 9, 16))).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    dims = ("time", "member", "latitude", "longitude")
    ds = minixr.make_dataset(np.zeros((40, 9, 16), dtype=np.float32), lat, lon, time=stamps, var="base")
    ds["time"].attrs = {}
    ds["member"] = minixr.DataArray(np.arange(M), ("member",), attrs={})
    ds["pv"] = minixr.DataArray(x.transpose(1, 0, 2, 3), dims, attrs={"units": "pvu"})
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    days, ids = _ids(stamps, "dayofyear")
    flat, tiled = x.reshape((M * 40, 9, 16)), np.tile(ids, M)
    f = c.std_field(variable="pv", k=1.0, window=5, ddof=1, segments="member")
    _same(np.asarray(f.data), std_util.want_std(flat, (0, 9), tiled, len(days), 5, 1, True)[0], "members pooled")
    assert f.attrs["units"] == "pvu" and f.name == "pv_std_field"
    from contrack_amd.contrack import std_field_numpy
    _same(np.asarray(f.data), std_field_numpy(flat, (0, 9), tiled, window=5, ddof=1), "the call on the flattened slab")
    thr = c.std_threshold(variable="pv", k=2.0, lat_bounds=(-40, 40), segments="member")
    rows = np.nonzero((lat >= -40) & (lat <= 40))[0]
    assert thr == 2.0 * np.mean(std_util.want_std(flat, (int(rows[0]), int(rows[-1]) + 1), np.zeros(M * 40, int), 1, 1, 0, True)[0][0])
    with pytest.raises(ValueError):
        c.std_field(variable="pv", segments="gaps")


def test_resident_anomaly_slab_is_used():
    from contrack_amd.contrack import _tracker
    lat, lon = synth.grid(NY, NX)
    rng = np.random.default_rng(8)
    stamps = (np.datetime64("2002-01-10") + np.arange(60)).astype("datetime64[ns]")
    z = (5500.0 + 50.0 * rng.standard_normal((60, NY, NX))).astype(np.float32)
    ds = minixr.make_dataset(z, lat, lon, time=stamps, var="z")
    ds["time"].attrs = {}
    ds["z"].attrs.update({"units": "m", "long_name": "Z500"})
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    c.calc_anom("z", window=5, smooth=2)
    anom = np.asarray(c.ds["anom"].data)
    assert _tracker().resident_anom() == anom.shape + (False,)
    seen = []
    real = _tracker().std_field
    months, ids = _ids(stamps, "month")
    try:
        _tracker().std_field = lambda x, *a, **k: (seen.append(x is None), real(x, *a, **k))[1]
        f = c.std_field(variable="anom", groupby="month", ddof=1)
    finally:
        del _tracker().std_field
    assert seen == [True], "the slab calc_anom left in HBM is read, not uploaded again"
    _same(np.asarray(f.data), std_util.want_std(anom, (0, NY), ids, len(months), 1, 1, True)[0], "resident")
