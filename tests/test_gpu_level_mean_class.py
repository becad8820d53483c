"""calc_vertical_mean of the class on tests/minixr.py: the first step of the third recipe of the reference's README (README.rst:235-240:
"The PV fields are vertically averaged between 500-150 hPa"), then calc_anom on the mean that stayed in HBM and run_contrack.  Expected
values: the numpy statement tests/level_util.py with contrack.level_weights, compared by bit pattern (level_util.same_bits: NaN at the same
places, equal integer views everywhere else; the sign and payload of a NaN, which differ between host and device, are not compared)."""
import numpy as np
import pytest

import level_util as lu
import minixr
from contrack_amd import _native, synth
from contrack_amd.contrack import _tracker, contrack, level_weights

pytestmark = pytest.mark.gpu
minixr.install_as_xarray()

CANON = ("time", "level", "latitude", "longitude")
T, NY, NX = 40, 9, 16
LEVELS = lu.PINNED_LEVELS


def smooth4(dtype=np.float32, seed=0):
    """(T, 15, NY, NX): a smooth field per level (contours that persist), scaled differently on every level"""
    x = np.stack([synth.smooth_field(T, NY, NX, seed=seed + l) * (1.0 + 0.05 * l) for l in range(len(LEVELS))], axis=1)
    return x.astype(dtype)


def dataset(x, dims=CANON, levels=LEVELS, lev_name="level", lev_units="hPa", extra=None):
    """x in the canonical order (extra dimension first if any); the variable 'pv' is stored with dims `dims`"""
    canon = ((extra,) if extra else ()) + tuple(lev_name if d == "level" else d for d in CANON)
    dims = tuple(lev_name if d == "level" else d for d in dims)
    lat = np.linspace(80, -80, NY).astype(np.float32)
    lon = (np.arange(NX) * (360.0 / NX)).astype(np.float32)
    days = (np.datetime64("2000-12-20") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(np.zeros((T, NY, NX), dtype=np.float32), lat, lon, time=days, var="base")
    ds[lev_name] = minixr.DataArray(np.asarray(levels, dtype=np.float64), (lev_name,), attrs={"units": lev_units})
    if extra:
        ds[extra] = minixr.DataArray(np.arange(x.shape[0]), (extra,), attrs={})
    ds['pv'] = minixr.DataArray(x.transpose([canon.index(d) for d in dims]), dims, attrs={"units": "pvu", "long_name": "potential vorticity"})
    return ds


def instance(ds):
    c = contrack(ds=ds)
    c.set_up()
    return c


def to_tll(da):
    return np.asarray(da.data).transpose([tuple(da.dims).index(d) for d in ("time", "latitude", "longitude")])


@pytest.mark.parametrize("dims", [CANON, ("longitude", "time", "latitude", "level")])
@pytest.mark.parametrize("descending", [True, False])
def test_vertical_mean_dims_attrs_values(dims, descending):
    x = smooth4()
    x[3, 5, 2, 2] = np.nan
    levels = LEVELS if descending else LEVELS[::-1]
    c = instance(dataset(x, dims, levels))
    c.calc_vertical_mean('pv', bounds=(150, 500))
    w = level_weights(levels, (150, 500))
    assert np.array_equal(w, lu.PINNED_WEIGHTS if descending else lu.PINNED_WEIGHTS[::-1])
    v = c.ds['pv_vmean']
    assert tuple(v.dims) == tuple(d for d in dims if d != "level") and v.data.dtype == np.float32
    assert v.attrs['units'] == "pvu" and v.attrs['long_name'] == "potential vorticity vertical mean"
    sel = levels[w > 0].tolist()
    assert 'bounds = (150, 500)' in v.attrs['history'] and str(sel) in v.attrs['history'] and 'weights = pressure' in v.attrs['history']
    want = lu.level_mean(x, w)
    assert np.isnan(want[3, 2, 2]) and lu.same_bits(to_tll(v), want)
    assert _tracker().resident_level_mean() == (T, NY, NX, False) and not np.asarray(v.data).flags.writeable
    c.calc_vertical_mean('pv', bounds=(500, 150), weights='equal', skipna=True, name='pv_eq')
    assert lu.same_bits(to_tll(c.ds['pv_eq']), lu.level_mean(x, (w > 0).astype(np.float64), skipna=True))
    given = np.where(w > 0, np.arange(15) + 1.0, 0.0)
    c.calc_vertical_mean('pv', weights=given, name='pv_given')
    assert lu.same_bits(to_tll(c.ds['pv_given']), lu.level_mean(x, given)) and 'weights = given' in c.ds['pv_given'].attrs['history']


def test_level_dimension_is_found_or_named():
    x = smooth4()
    c = instance(dataset(x, lev_name="height", lev_units="Pa"))         # by the units of its coordinate
    c.calc_vertical_mean('pv', bounds=(150, 500))
    assert lu.same_bits(to_tll(c.ds['pv_vmean']), lu.level_mean(x, lu.PINNED_WEIGHTS))
    c = instance(dataset(x, lev_name="height", lev_units="m"))
    with pytest.raises(ValueError, match="no level dimension found among the dims"):
        c.calc_vertical_mean('pv', bounds=(150, 500))
    c.calc_vertical_mean('pv', bounds=(150, 500), level_name="height")
    assert lu.same_bits(to_tll(c.ds['pv_vmean']), lu.level_mean(x, lu.PINNED_WEIGHTS))
    with pytest.raises(ValueError, match="select no level"):
        c.calc_vertical_mean('pv', bounds=(1, 2), level_name="height")


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


@pytest.mark.parametrize("dims", [("member",) + CANON, ("latitude", "time", "level", "member", "longitude")])
def test_member_dimension_and_chunks(dims, monkeypatch):
    M = 3
    x = np.stack([smooth4(np.float64, seed=20 * m) for m in range(M)])
    w = lu.PINNED_WEIGHTS.copy()
    w[6] = 0.0                                                            # a hole: two runs of selected levels
    want = lu.level_mean(x.reshape((M * T,) + x.shape[2:]), w).reshape((M, T, NY, NX))
    c = instance(dataset(x, dims, extra="member"))
    out_dims = tuple(d for d in dims if d != "level")

    def canon(da):
        return np.asarray(da.data).transpose([out_dims.index(d) for d in ("member", "time", "latitude", "longitude")])
    c.calc_vertical_mean('pv', weights=w)
    assert tuple(c.ds['pv_vmean'].dims) == out_dims and c.ds['pv_vmean'].data.dtype == np.float64
    assert lu.same_bits(canon(c.ds['pv_vmean']), want)
    assert c._vmean_resident is None                                      # (a member dimension: nothing is kept for calc_anom)
    # streamed: read slice by slice, the selected levels only, never the 4-D array
    counting, real = Counting(c.ds['pv']), type(c.ds).__getitem__
    monkeypatch.setattr(type(c.ds), "__getitem__", lambda self, key: counting if key == 'pv' else real(self, key))
    c.calc_vertical_mean('pv', weights=w, chunk_steps=7, name='pv_s')
    monkeypatch.undo()
    assert lu.same_bits(canon(c.ds['pv_s']), want)
    outer, inner = [d for d in dims if d in ("member", "time")]            # the step dims in their own order: index, slice
    assert counting.pieces and all(kw["level"] in (slice(3, 6), slice(7, 13)) and isinstance(kw[outer], int) and isinstance(kw[inner], slice)
                                   for kw, _ in counting.pieces)
    assert sum(int(np.prod(shape)) for _, shape in counting.pieces) == M * T * 9 * NY * NX


def test_chain_to_run_contrack_and_fallback():
    x = smooth4()
    w = lu.PINNED_WEIGHTS
    mean = lu.level_mean(x, w)
    a = instance(dataset(x))
    a.calc_vertical_mean('pv', bounds=(150, 500))
    trk = _tracker()
    gen = trk.resident_level_mean_generation()
    assert a._vmean_resident_for('pv_vmean', to_tll(a.ds['pv_vmean']))
    a.calc_anom('pv_vmean', window=3, smooth=2)                          # from the mean in HBM
    assert trk.resident_level_mean_generation() == gen
    # the same chain from a numpy-computed mean
    ds_b = dataset(x)
    ds_b['pv_vmean'] = minixr.DataArray(mean, ("time", "latitude", "longitude"), attrs={"units": "pvu", "long_name": "pv mean"})
    b = instance(ds_b)
    assert not b._vmean_resident_for('pv_vmean', mean)
    b.calc_anom('pv_vmean', window=3, smooth=2)
    anom_a, anom_b = np.asarray(a.ds['anom'].data), np.asarray(b.ds['anom'].data)
    assert lu.same_bits(anom_a, anom_b) and np.isfinite(anom_b).any()
    thr = float(np.nanquantile(anom_b, 0.85))
    # b ran last: its anomaly is the resident one, a's run_contrack goes back to its host array; both give the same flag
    for c in (a, b):
        c.run_contrack('anom', thr, '>=', 0.3, 2)
    assert np.array_equal(a.ds['flag'].data, b.ds['flag'].data) and np.asarray(b.ds['flag'].data).max() >= 1
    # another instance's calc_vertical_mean on the shared handle: the first instance's calc_anom falls back to its host array
    other = instance(dataset(smooth4(seed=99)))
    other.calc_vertical_mean('pv', bounds=(150, 500))
    assert trk.resident_level_mean_generation() != gen and not a._vmean_resident_for('pv_vmean', to_tll(a.ds['pv_vmean']))
    a.calc_anom('pv_vmean', window=3, smooth=2)
    assert lu.same_bits(np.asarray(a.ds['anom'].data), anom_b)
    # a replaced host array never counts as the resident twin
    other.ds['pv_vmean'] = (("time", "latitude", "longitude"), mean.copy(), {"units": "pvu", "long_name": "pv mean"})
    assert not other._vmean_resident_for('pv_vmean', mean)
    other.calc_anom('pv_vmean', window=3, smooth=2)
    assert lu.same_bits(np.asarray(other.ds['anom'].data), anom_b)
