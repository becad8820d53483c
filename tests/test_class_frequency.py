"""contrack.calc_frequency on the xarray stand-in: the README's blocking frequency (README.rst:159-160 of the reference) and its
groupby('time.<x>') versions, as labelled arrays over the flag variable's own dims."""
import numpy as np
import pytest

import freq_util
import golden_util
import minixr
from contrack_amd.contrack import contrack, season_of_month

pytestmark = pytest.mark.gpu

minixr.install_as_xarray()          # only when the real package is absent


def _time(T, step_days=40, start="2000-10-20"):
    return (np.datetime64(start) + np.arange(T) * step_days).astype("datetime64[D]").astype("datetime64[ns]")


def _months_years(time):
    m = time.astype("datetime64[M]").astype(np.int64)
    return m % 12 + 1, m // 12 + 1970


def _tracked(name="refslab_fwd"):
    g = golden_util.load(name)
    T = g["anom"].shape[0]
    ds = minixr.make_dataset(g["anom"], g["lat"], g["lon"], time=_time(T), time_units="days since 2000-10-20")
    c = contrack(ds=ds)
    c.run_contrack(variable='anom', threshold=g["thr"], gorl=g["gorl"], overlap=g["overlap"], persistence=g["persistence"],
                   twosided=g["twosided"])
    assert np.array_equal(np.asarray(c['flag'].data), g["flag"])
    return c, g


@pytest.mark.parametrize("groupby", [None, 'month', 'season', 'year'])
def test_after_run_contrack(groupby):
    c, g = _tracked()
    flag = g["flag"]
    time = np.asarray(c.ds['time'].data)
    month, year = _months_years(time)
    f = c.calc_frequency(groupby=groupby)
    assert 'frequency' not in c.variables and c.variables == ['anom', 'flag']
    assert f.attrs['units'] == '%' and 'Calculated from flag' in f.attrs['history']
    assert np.asarray(f.data).dtype == np.float64
    if groupby is None:
        assert tuple(f.dims) == ('latitude', 'longitude')
        assert freq_util.same_bits(f.data, freq_util.percent(flag))
    else:
        vals = {'month': month, 'year': year, 'season': season_of_month(month)}[groupby]
        uniq, ids = np.unique(vals, return_inverse=True)
        assert tuple(f.dims) == (groupby, 'latitude', 'longitude')
        assert list(np.asarray(f.coords[groupby])) == list(uniq)
        assert freq_util.same_bits(f.data, freq_util.percent(flag, ids, len(uniq)))
        if groupby == 'season':
            assert list(uniq) == sorted(set(uniq)) and set(uniq) <= {'DJF', 'JJA', 'MAM', 'SON'}
    assert np.array_equal(np.asarray(f.coords['latitude']), g["lat"]) and np.array_equal(np.asarray(f.coords['longitude']), g["lon"])


def test_readme_expression_above_1():
    """xr.where(block['flag'] > 1, 1, 0).sum(dim='time') / block.ntime * 100"""
    c, g = _tracked("refslab_two")
    f = c.calc_frequency(flag='flag', above=1)
    want = minixr.where(c.ds['flag'] > 1, 1, 0).data.sum(axis=0) / c.ntime * 100
    assert freq_util.same_bits(f.data, want)


def _dataset_with_flag(flag, lat, lon, dims, dtype=np.int32):
    T = flag.shape[0]
    ds = minixr.make_dataset(np.zeros(flag.shape, np.float32), lat, lon, time=_time(T, 17), time_units="days since 2000-10-20")
    order = [("time", "latitude", "longitude").index(d) for d in dims]
    ds["blocks"] = minixr.DataArray(flag.astype(dtype).transpose(order), dims, attrs={"units": "flag"})
    return ds


@pytest.mark.parametrize("dims", [("latitude", "time", "longitude"), ("longitude", "latitude", "time")])
def test_dim_order_and_coords(dims):
    g = golden_util.load("odd_65x130")
    flag = g["flag"]
    c = contrack(ds=_dataset_with_flag(flag, g["lat"], g["lon"], dims))
    f = c.calc_frequency(flag="blocks")
    sp = tuple(d for d in dims if d != "time")
    assert tuple(f.dims) == sp
    ref = freq_util.percent(flag)
    assert freq_util.same_bits(f.data, ref.transpose([("latitude", "longitude").index(d) for d in sp]))
    fm = c.calc_frequency(flag="blocks", groupby='month')
    gd = tuple('month' if d == 'time' else d for d in dims)
    assert tuple(fm.dims) == gd
    month, _ = _months_years(np.asarray(c.ds['time'].data))
    uniq, ids = np.unique(month, return_inverse=True)
    ref = freq_util.percent(flag, ids, len(uniq))
    assert freq_util.same_bits(fm.data, ref.transpose([("month", "latitude", "longitude").index(d) for d in gd]))
    for d, v in (("latitude", g["lat"]), ("longitude", g["lon"]), ("month", uniq)):
        assert np.array_equal(np.asarray(fm.coords[d]), v)


def test_int64_flag():
    g = golden_util.load("syn2deg_s1")
    flag = g["flag"]
    c = contrack(ds=_dataset_with_flag(flag, g["lat"], g["lon"], ("time", "latitude", "longitude"), np.int64))
    for groupby in (None, 'season'):
        f = c.calc_frequency(flag="blocks", groupby=groupby, above=2)
        if groupby is None:
            assert freq_util.same_bits(f.data, freq_util.percent(flag, above=2))
        else:
            month, _ = _months_years(np.asarray(c.ds['time'].data))
            uniq, ids = np.unique(season_of_month(month), return_inverse=True)
            assert freq_util.same_bits(f.data, freq_util.percent(flag, ids, len(uniq), above=2))
    c.ds["blocks"].data[3, 4, 5] = 2 ** 40
    with pytest.raises(ValueError, match="int32"):
        c.calc_frequency(flag="blocks")
