"""calc_reversal of the class on tests/minixr.py -- the gradient-reversal blocking index as a second producer of the field
run_contrack tracks -- against the numpy statement tests/reversal_util.py (bit patterns), then run_contrack from the resident slot
against the same call on the host array, and calc_frequency / calc_hovmoller on the tracked mask against their numpy utilities."""
import numpy as np
import pytest

import band_util as bu
import minixr
import reversal_util as ru
from contrack_amd.contrack import _tracker, contrack, frequency_percent, reversal_numpy, row_weights

pytestmark = pytest.mark.gpu
minixr.install_as_xarray()

TLL = ("time", "latitude", "longitude")
T, NX = 12, 24
LAT = ru.grid(5.0)
NY = len(LAT)
TRACK = dict(threshold=0, gorl='>', overlap=0.0, persistence=1)


def weather(steps, seed=0, dtype=np.float32):
    """the fixture profile with noise that is smooth in time and longitude (contours that overlap from step to step), N(0, 150) again"""
    rng = np.random.default_rng(seed)
    n = rng.normal(0.0, 1.0, (steps + 2, NY, NX))
    n = sum(np.roll(n, k, axis=2) for k in range(-2, 3))
    n = n[:-2] + n[1:-1] + n[2:]
    prof = 5600.0 - 900.0 * np.sin(np.deg2rad(LAT)) ** 2
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


def test_weather_has_blocks():
    for ghgs2 in (None, -5.0):
        tab = ru.table(LAT, ghgs2=ghgs2)
        assert 0.05 <= ru.blocked_share(ru.from_table(weather(T, 1), tab), tab["eq"]) <= 0.5


@pytest.mark.parametrize("dims", [TLL, ("longitude", "time", "latitude")])
def test_calc_reversal_dims_attrs_values(dims):
    z = weather(T, 1)
    c = dataset(z, dims)
    c.calc_reversal('z')
    v = c.ds['reversal']
    assert tuple(v.dims) == dims and v.data.dtype == np.float32
    assert v.attrs['units'] == 'm / degree' and 'geopotential height' in v.attrs['long_name']
    for part in ('Calculated from z', 'delta = 15.0', 'ghgs = 0.0', 'ghgn = -10.0', 'ghgs2 = None', 'lat_bounds = (30, 75)', 'hemisphere = both', 'stat = gradient'):
        assert part in v.attrs['history'], part
    want = ru.reversal(z, LAT)
    assert ru.same_bits(to(v), want) and ru.same_bits(reversal_numpy(z, LAT), want)
    assert _tracker().resident_anom() == (T, NY, NX, False) and not np.asarray(v.data).flags.writeable
    c.calc_reversal('z', delta=10., ghgs=-1., ghgn=-5., ghgs2=-5., lat_bounds=(35, 70), hemisphere='north', stat='mask', name='tm')
    m = c.ds['tm']
    want = ru.reversal(z, LAT, delta=10., ghgs=-1., ghgn=-5., ghgs2=-5., lat_bounds=(35, 70), hemisphere='north', stat='mask')
    assert set(np.unique(want)) == {0.0, 1.0} and ru.same_bits(to(m), want) and m.attrs['units'] == '1'
    assert 'ghgs2 = -5.0' in m.attrs['history'] and 'hemisphere = north' in m.attrs['history'] and 'stat = mask' in m.attrs['history']
    with pytest.raises(ValueError, match="stat="):
        c.calc_reversal('z', stat='sum')
    with pytest.raises(ValueError, match="hemisphere="):
        c.calc_reversal('z', hemisphere='east')


class Counting:
    """wraps a DataArray: records the pieces read through isel, refuses to be read as a whole"""

    def __init__(self, da):
        self._da = da
        self.dims, self.shape, self.dtype, self.attrs = da.dims, da.data.shape, da.data.dtype, da.attrs
        self.pieces = []

    @property
    def data(self):
        raise AssertionError("the whole variable was materialised")

    def isel(self, **kw):
        part = self._da.isel(**kw)
        self.pieces.append((dict(kw), part.data.shape))
        return part


@pytest.mark.parametrize("dims", [("member",) + TLL, ("latitude", "time", "member", "longitude")])
def test_member_dimension_and_chunks(dims, monkeypatch):
    canon = ("member",) + TLL
    z4 = np.stack([weather(T, s, np.float64) for s in (2, 3, 4)])
    want = np.stack([ru.reversal(z, LAT, ghgs2=-5.) for z in z4])
    c = dataset(z4, dims, canon, extra="member")
    c.calc_reversal('z', ghgs2=-5.)                                               # the whole variable at once: every (member, time) pair is a step
    assert tuple(c.ds['reversal'].dims) == dims and ru.same_bits(to(c.ds['reversal'], canon), want)
    g = _tracker().resident_generation()
    outer, inner = [d for d in dims if d in ("member", "time")]                   # the step dims in their own order: index, slice
    for cs in (5, 0):                                                             # streamed: read slice by slice, never the 4-D array
        counting, real = Counting(c.ds['z']), type(c.ds).__getitem__
        monkeypatch.setattr(type(c.ds), "__getitem__", lambda self, key: counting if key == 'z' else real(self, key))
        c.calc_reversal('z', ghgs2=-5., chunk_steps=cs, name='rev_cs')
        monkeypatch.undo()
        assert tuple(c.ds['rev_cs'].dims) == dims and ru.same_bits(to(c.ds['rev_cs'], canon), want), cs
        assert len(counting.pieces) >= 3 and all(isinstance(kw[outer], int) and isinstance(kw[inner], slice) for kw, _ in counting.pieces)
        assert sum(int(np.prod(shape)) for _, shape in counting.pieces) == want.size
    assert _tracker().resident_generation() == g                                # streamed calls keep nothing on the device


def test_two_outer_step_dims_in_chunks():
    """(run, member, time, lat, lon) = (2, 3, 4, 5, 8): 24 steps behind two outer step dims; chunks of 5 steps cross the runs of 4"""
    lat = np.arange(30.0, 91.0, 15.0)
    rng = np.random.default_rng(7)
    z = ((5600.0 - 900.0 * np.sin(np.deg2rad(lat)) ** 2)[:, None] + 150.0 * rng.normal(0.0, 1.0, (2, 3, 4, 5, 8))).astype(np.float32)
    days = (np.datetime64("2000-12-20") + np.arange(4)).astype("datetime64[ns]")
    ds = minixr.make_dataset(np.zeros((4, 5, 8), dtype=np.float32), lat.astype(np.float32), (np.arange(8) * 45.0).astype(np.float32), time=days, var="base")
    ds['run'], ds['member'] = minixr.DataArray(np.arange(2), ("run",), attrs={}), minixr.DataArray(np.arange(3), ("member",), attrs={})
    ds['z'] = minixr.DataArray(z, ("run", "member") + TLL, attrs={"units": "m", "long_name": "geopotential height"})
    c = contrack(ds=ds)
    c.set_up()
    c.calc_reversal('z')
    c.calc_reversal('z', chunk_steps=5, name='rev_cs')
    whole = np.asarray(c.ds['reversal'].data)
    assert tuple(c.ds['rev_cs'].dims) == ("run", "member") + TLL and whole.shape == z.shape
    assert ru.same_bits(whole.reshape(24, 5, 8), ru.reversal(z.reshape(24, 5, 8), lat.astype(np.float32))) and whole.any()
    assert ru.same_bits(np.asarray(c.ds['rev_cs'].data), whole)


def spy(monkeypatch):
    """counts the tracker's calls by path"""
    seen = dict(resident=0, host=0)
    trk = _tracker()
    real_r, real_h = trk.track_resident, trk.track
    monkeypatch.setattr(trk, "track_resident", lambda *a, **k: (seen.__setitem__("resident", seen["resident"] + 1), real_r(*a, **k))[1])
    monkeypatch.setattr(trk, "track", lambda *a, **k: (seen.__setitem__("host", seen["host"] + 1), real_h(*a, **k))[1])
    return seen


def test_run_contrack_from_the_resident_slot(monkeypatch):
    seen = spy(monkeypatch)
    z = weather(T, 5)
    c = dataset(z)
    c.calc_reversal('z')
    g = _tracker().resident_generation()
    c.run_contrack('reversal', **TRACK)
    assert seen == dict(resident=1, host=0) and _tracker().resident_generation() == g
    from_hbm = np.asarray(c['flag'].data).copy()
    assert from_hbm.max() > 3 and np.array_equal(from_hbm > 0, ru.reversal(z, LAT) > 0)
    keep = c._anom_resident
    c._anom_resident = None                                                       # force the host-array path
    c.run_contrack('reversal', **TRACK)
    assert seen == dict(resident=1, host=1) and np.array_equal(np.asarray(c['flag'].data), from_hbm)
    c._anom_resident = keep
    other = dataset(weather(T, 6))                                                # another instance's calc_anom takes the slot: back to the host array, equal ids
    other.calc_anom('z', window=5)
    assert _tracker().resident_generation() != g
    c.run_contrack('reversal', **TRACK)
    assert seen == dict(resident=1, host=2) and np.array_equal(np.asarray(c['flag'].data), from_hbm)
    other.run_contrack('anom', threshold=50.0, gorl='>=', overlap=0.0, persistence=1)      # calc_anom, then run_contrack('anom'): as ever
    assert seen == dict(resident=2, host=2)
    hbm = np.asarray(other['flag'].data).copy()
    other._anom_resident = None
    other.run_contrack('anom', threshold=50.0, gorl='>=', overlap=0.0, persistence=1)
    assert seen == dict(resident=2, host=3) and hbm.max() > 0 and np.array_equal(np.asarray(other['flag'].data), hbm)
    c.calc_reversal('z')                                                          # the other consumers pass 'anom': this variable comes from the host array
    c.calc_anom('z', window=5)                                             # ... and calc_anom on the same instance takes the name back
    c.run_contrack('reversal', **TRACK)
    assert seen == dict(resident=2, host=4) and np.array_equal(np.asarray(c['flag'].data), from_hbm)
    c.run_contrack('anom', threshold=50.0, gorl='>=', overlap=0.0, persistence=1)
    assert seen == dict(resident=3, host=4)


def test_consumers_on_the_tracked_mask():
    z = weather(T, 7)
    c = dataset(z)
    c.calc_reversal('z', ghgs2=-5.)
    c.run_contrack('reversal', threshold=0, gorl='>', overlap=0.5, persistence=2)
    flag = np.asarray(c['flag'].data)
    assert flag.dtype == np.int32 and flag.max() > 0
    freq = c.calc_frequency()
    assert tuple(freq.dims) == ("latitude", "longitude")
    want = frequency_percent(np.count_nonzero(flag > 0, axis=0)[None], np.array([T]))
    assert np.array_equal(np.asarray(freq.data), want.reshape(NY, NX)) and np.asarray(freq.data).max() > 0
    w = row_weights(np.asarray(c.ds["latitude"].data), c._dlat, c._dlon).astype(np.float64)
    rows = np.nonzero((LAT >= 56) & (LAT <= 64))[0]                               # the narrow band of the one-dimensional diagram: 60N alone here
    assert rows.tolist() == [6]
    hov = c.calc_hovmoller(lat_bounds=(56, 64), stat="count")
    assert tuple(hov.dims) == ("time", "longitude")
    assert np.array_equal(np.asarray(hov.data), bu.band(flag, 6, 7, w)["cnt"]) and np.asarray(hov.data).max() > 0
    frac = c.calc_hovmoller(lat_bounds=(56, 64))
    assert np.array_equal(bu.bits(frac.data), bu.bits(bu.band(flag, 6, 7, w)["area"] / bu.band_total(w, 6, 7)))
