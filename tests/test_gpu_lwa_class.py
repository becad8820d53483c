"""calc_lwa of the class on tests/minixr.py -- the local wave activity as a third producer of the field run_contrack tracks -- against
the numpy statement tests/lwa_util.py (bit patterns), then percentile_threshold and run_contrack from the resident slot against the
same calls on the host array, and calc_frequency on the tracked flag."""
import numpy as np
import pytest

import lwa_util as lu
import minixr
from contrack_amd.contrack import _tracker, contrack, frequency_percent, lwa_numpy

pytestmark = pytest.mark.gpu
minixr.install_as_xarray()

TLL = ("time", "latitude", "longitude")
T, NX = 12, 24
LAT = lu.grid(5.0)
NY = len(LAT)


def weather(steps, seed=0, dtype=np.float32):
    """the falling profile with noise that is smooth in time and longitude: ridges that overlap from step to step"""
    rng = np.random.default_rng(seed)
    n = rng.normal(0.0, 1.0, (steps + 2, NY, NX))
    n = sum(np.roll(n, k, axis=2) for k in range(-2, 3))
    n = n[:-2] + n[1:-1] + n[2:]
    prof = 5700.0 - 800.0 * np.sin(np.deg2rad(LAT)) ** 2
    return (prof[None, :, None] + 150.0 * n / n.std()).astype(dtype)


def dataset(z, dims=TLL, canon=TLL, extra=None):
    """z in the order `canon`; the variable 'z' is stored with dims `dims`"""
    days = (np.datetime64("2000-12-20") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(np.zeros((T, NY, NX), dtype=np.float32), LAT.astype(np.float32), (np.arange(NX) * (360.0 / NX)).astype(np.float32), time=days, var="base")
    if extra:
        ds[extra] = minixr.DataArray(np.arange(z.shape[canon.index(extra)]), (extra,), attrs={})
    ds['z'] = minixr.DataArray(z.transpose([canon.index(d) for d in dims]), dims, attrs={"units": "m", "long_name": "geopotential height"})
    c = contrack(ds=ds)
    c.set_up()
    return c


def to(da, order=TLL):
    return np.asarray(da.data).transpose([tuple(da.dims).index(d) for d in order])


def test_weather_has_wave_activity():
    tab = lu.rows(LAT)
    for part in (0, 1):
        assert lu.nonzero_share(lu.from_table(weather(T, 1), tab, part), tab) >= (0.5, 0.3)[part]


@pytest.mark.parametrize("dims", [TLL, ("longitude", "time", "latitude")])
def test_calc_lwa_dims_attrs_values_reference(dims):
    z = weather(T, 1)
    c = dataset(z, dims)
    c.calc_lwa('z', reference='zref')
    v, r = c.ds['lwa'], c.ds['zref']
    assert tuple(v.dims) == dims and v.data.dtype == np.float32
    assert v.attrs['units'] == 'm m' and 'geopotential height' in v.attrs['long_name'] and 'local wave activity' in v.attrs['long_name']
    for part in ('Calculated from z', 'lat_bounds = (30, 75)', 'hemisphere = both', 'part = total', 'radius = 6371000.0'):
        assert part in v.attrs['history'], part
    want, ref = lu.lwa(z, LAT, return_ref=True)
    assert lu.same_bits(to(v), want) and lu.same_bits(lwa_numpy(z, LAT), want)
    assert tuple(r.dims) == tuple(d for d in dims if d != "longitude") and r.attrs['units'] == 'm'
    assert lu.same_bits(np.asarray(r.data).transpose([tuple(r.dims).index(d) for d in ("time", "latitude")]), ref)
    assert _tracker().resident_anom() == (T, NY, NX, False) and not np.asarray(v.data).flags.writeable
    c.calc_lwa('z', lat_bounds=(35, 70), hemisphere='north', part='anticyclonic', name='awa', radius=1.0)
    m = c.ds['awa']
    want = lu.lwa(z, LAT, lat_bounds=(35, 70), hemisphere='north', part=1, radius=1.0)
    assert np.count_nonzero(want) and not want[:, LAT < 35].any() and lu.same_bits(to(m), want)
    assert 'anticyclonic' in m.attrs['long_name'] and 'hemisphere = north' in m.attrs['history'] and 'part = anticyclonic' in m.attrs['history']
    with pytest.raises(ValueError, match="part="):
        c.calc_lwa('z', part='sum')
    with pytest.raises(ValueError, match="hemisphere="):
        c.calc_lwa('z', hemisphere='east')
    with pytest.raises(ValueError, match="lat_bounds"):
        c.calc_lwa('z', lat_bounds=(0, 75))


@pytest.mark.parametrize("dims", [("member",) + TLL, ("latitude", "time", "member", "longitude")])
def test_member_dimension_and_chunks(dims):
    canon = ("member",) + TLL
    z4 = np.stack([weather(T, s, np.float64) for s in (2, 3, 4)])
    both = [lu.lwa(z, LAT, part=2, return_ref=True) for z in z4]
    want, ref = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    assert np.count_nonzero(want) > want.size // 10
    c = dataset(z4, dims, canon, extra="member")
    c.calc_lwa('z', part='cyclonic', reference='zr')                             # the whole variable at once: every (member, time) pair is a step
    assert tuple(c.ds['lwa'].dims) == dims and c.ds['lwa'].data.dtype == np.float64 and lu.same_bits(to(c.ds['lwa'], canon), want)
    assert lu.same_bits(to(c.ds['zr'], ("member", "time", "latitude")), ref)
    g = _tracker().resident_generation()
    for cs in (5, 0):                                                            # streamed against the call on the whole slab
        c.calc_lwa('z', part='cyclonic', chunk_steps=cs, name='lwa_cs', reference='zr_cs')
        assert tuple(c.ds['lwa_cs'].dims) == dims and lu.same_bits(to(c.ds['lwa_cs'], canon), want), cs
        assert lu.same_bits(to(c.ds['zr_cs'], ("member", "time", "latitude")), ref), cs
    assert _tracker().resident_generation() == g                                 # streamed calls keep nothing on the device


def test_chunks_against_the_resident_path():
    z = weather(T, 3)
    c = dataset(z)
    c.calc_lwa('z', part='anticyclonic')
    assert _tracker().resident_anom() == (T, NY, NX, False)
    g = _tracker().resident_generation()
    c.calc_lwa('z', part='anticyclonic', chunk_steps=5, name='cs')
    assert _tracker().resident_generation() == g and np.asarray(c.ds['cs'].data).flags.writeable
    assert lu.same_bits(np.asarray(c.ds['cs'].data), np.asarray(c.ds['lwa'].data)) and np.count_nonzero(c.ds['cs'].data)


def test_percentile_threshold_run_contrack_and_frequency(monkeypatch):
    seen = dict(resident=0, host=0)
    trk = _tracker()
    real_r, real_h = trk.track_resident, trk.track
    monkeypatch.setattr(trk, "track_resident", lambda *a, **k: (seen.__setitem__("resident", seen["resident"] + 1), real_r(*a, **k))[1])
    monkeypatch.setattr(trk, "track", lambda *a, **k: (seen.__setitem__("host", seen["host"] + 1), real_h(*a, **k))[1])
    z = weather(T, 5)
    c = dataset(z)
    c.calc_lwa('z', part='anticyclonic')
    want = lu.lwa(z, LAT, part=1)
    g = trk.resident_generation()
    thr = c.percentile_threshold(variable='lwa', q=0.8, lat_bounds=(40, 70))      # from HBM
    keep = c._anom_resident
    c._anom_resident = None
    assert c.percentile_threshold(variable='lwa', q=0.8, lat_bounds=(40, 70)) == thr          # from the host array
    c._anom_resident = keep
    band = want[:, (LAT >= 40) & (LAT <= 70)].astype(np.float64)
    assert thr == pytest.approx(np.quantile(band, 0.8, axis=0).mean(), rel=1e-12) and thr > 0
    c.run_contrack('lwa', threshold=thr, gorl='>', overlap=0.0, persistence=1)
    assert seen == dict(resident=1, host=0) and trk.resident_generation() == g
    from_hbm = np.asarray(c['flag'].data).copy()
    assert from_hbm.max() > 3 and np.array_equal(from_hbm > 0, want > thr)
    c._anom_resident = None                                                       # force the host-array path: identical ids
    c.run_contrack('lwa', threshold=thr, gorl='>', overlap=0.0, persistence=1)
    assert seen == dict(resident=1, host=1) and np.array_equal(np.asarray(c['flag'].data), from_hbm)
    freq = c.calc_frequency()
    assert tuple(freq.dims) == ("latitude", "longitude")
    expect = frequency_percent(np.count_nonzero(from_hbm > 0, axis=0)[None], np.array([T]))
    assert np.array_equal(np.asarray(freq.data), expect.reshape(NY, NX)) and np.asarray(freq.data).max() > 0
