"""contrack.calc_composite on the xarray stand-in (tests/minixr.py) against the numpy statement of tests/composite_util.py: the sums
bit for bit, the counts exactly, the mean as sum / n.  Flags: the golden slabs smooth0 / smooth1 / smooth2 (16 x 46 x 72, coherent
blocks); the variable spans 18 orders of magnitude, so a sum in another order or in float32 shows in the bits."""
import functools

import numpy as np
import pytest

import composite_util as cu
import life_util
import minixr
from contrack_amd import contrack as cm
from contrack_amd.contrack import season_of_month

minixr.install_as_xarray()
pytestmark = pytest.mark.gpu
MEMBERS = ("smooth0", "smooth1", "smooth2")
TLL = ("time", "latitude", "longitude")
CANON = ("member",) + TLL


def _time(T, step_days=40, start="2000-10-20"):
    return (np.datetime64(start) + np.arange(T) * step_days).astype("datetime64[D]").astype("datetime64[ns]")


@functools.lru_cache(maxsize=None)
def members(dtype=np.float32):
    gs = [life_util.load(n) for n in MEMBERS]
    flag = np.stack([g["flag"] for g in gs]).astype(np.int32)
    assert flag.shape == (3, 16, 46, 72) and (flag > 0).any()
    rng = np.random.default_rng(31)
    var = (rng.standard_normal(flag.shape) * 10.0 ** rng.uniform(-8, 10, flag.shape)).astype(dtype)
    return gs[0], flag, var


def _ids(groupby, T=16):
    if groupby is None:
        return None, None
    month = _time(T).astype("datetime64[M]").astype(np.int64) % 12 + 1
    uniq, ids = np.unique(month if groupby == "month" else season_of_month(month), return_inverse=True)
    return uniq, ids.astype(np.int32)


def single(m=0, dims=TLL, dtype=np.float32, name="t2m"):
    g, flag4, var4 = members(dtype)
    order = [TLL.index(d) for d in dims]
    ds = minixr.make_dataset(np.zeros(flag4[m].shape, np.float32), g["lat"], g["lon"], time=_time(16), time_units="days since 2000-10-20")
    ds["flag"] = minixr.DataArray(flag4[m].transpose(order), dims, attrs={"units": "flag"})
    ds[name] = minixr.DataArray(var4[m].transpose(order).copy(), dims, attrs={"units": "K", "long_name": "2 m temperature"})
    return cm.contrack(ds=ds), flag4[m], var4[m]


def dataset4(dims, dtype=np.float32):
    g, flag4, var4 = members(dtype)
    order = [CANON.index(d) for d in dims]
    ds = minixr.make_dataset(np.zeros(flag4[0].shape, np.float32), g["lat"], g["lon"], time=_time(16), time_units="days since 2000-10-20")
    ds["member"] = minixr.DataArray(np.array([10, 20, 30]), ("member",), attrs={})
    ds["flag"] = minixr.DataArray(flag4.transpose(order), dims, attrs={"units": "flag"})
    ds["t2m"] = minixr.DataArray(var4.transpose(order), dims, attrs={"units": "K", "long_name": "2 m temperature"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c, flag4, var4


def _mean(s, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n == 0, np.nan, s / n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("groupby", [None, "season", "month"])
def test_mean_sum_and_count(groupby, dtype):
    c, flag, var = single(dtype=dtype)
    uniq, ids = _ids(groupby)
    G = 1 if ids is None else len(uniq)
    s, n = cu.composite(flag, var, ids, G)
    if groupby != "month":                                                     # (a month holds two steps at most: no order to get wrong)
        assert cu.differing(s, cu.composite(flag, var, ids, G, order="falling")[0]) >= 1
    want_dims = ((groupby,) if groupby else ()) + TLL[1:]
    m, cnt = c.calc_composite("t2m", groupby=groupby, return_count=True)
    assert sorted(c.variables) == ["anom", "flag", "t2m"]                            # nothing is added to the dataset
    assert tuple(m.dims) == want_dims == tuple(cnt.dims)
    assert np.asarray(m.data).dtype == np.float64 and np.asarray(cnt.data).dtype == np.uint32
    assert m.attrs["units"] == "K" and "Calculated from t2m" in m.attrs["history"] and "flag > 0" in m.attrs["history"]
    sq = (lambda a: a[0]) if groupby is None else (lambda a: a)
    assert np.array_equal(np.asarray(cnt.data), sq(n))
    assert cu.same_bits(np.asarray(m.data), sq(_mean(s, n)))
    assert np.isnan(np.asarray(m.data)).any() and not np.isnan(np.asarray(m.data)).all()
    tot = c.calc_composite("t2m", groupby=groupby, stat="sum")
    assert cu.same_bits(np.asarray(tot.data), sq(s)) and tuple(tot.dims) == want_dims and "stat = sum" in tot.attrs["history"]
    if groupby is not None:
        assert list(np.asarray(m.coords[groupby])) == list(uniq)
    assert np.array_equal(np.asarray(m.coords["latitude"]), np.asarray(c.ds["latitude"].data))
    for steps in (1, 5, 100):
        again = c.calc_composite("t2m", groupby=groupby, stat="sum", chunk_steps=steps)
        assert cu.same_bits(np.asarray(again.data), sq(s)), steps


def test_above_and_skipna():
    c, flag, var = single()
    vn = var.copy()
    vn[::3] = np.nan
    c.ds["t2m"].data[...] = vn
    for skipna in (False, True):
        s, n = cu.composite(flag, vn, None, 1, above=1, skipna=skipna)
        m, cnt = c.calc_composite("t2m", above=1, skipna=skipna, return_count=True)
        assert np.array_equal(np.asarray(cnt.data), n[0]) and cu.same_bits(np.asarray(m.data), _mean(s, n)[0])
    assert (cu.composite(flag, vn, None, 1, above=1)[1] != n).any()


@pytest.mark.parametrize("dims", [("latitude", "time", "longitude"), ("longitude", "latitude", "time")])
def test_dims_in_another_order(dims):
    c, flag, var = single(dims=dims)
    uniq, ids = _ids("month")
    s, n = cu.composite(flag, var, ids, len(uniq))
    for chunk_steps in (None, 5):
        m = c.calc_composite("t2m", groupby="month", stat="sum", chunk_steps=chunk_steps)
        gd = tuple("month" if d == "time" else d for d in dims)
        assert tuple(m.dims) == gd
        assert cu.same_bits(np.asarray(m.data), s.transpose([(("month",) + TLL[1:]).index(d) for d in gd]))
    plain = c.calc_composite("t2m", stat="sum")
    sp = tuple(d for d in dims if d != "time")
    assert tuple(plain.dims) == sp
    assert cu.same_bits(np.asarray(plain.data), cu.composite(flag, var, None, 1)[0][0].transpose([TLL[1:].index(d) for d in sp]))


@pytest.mark.parametrize("groupby", [None, "month"])
@pytest.mark.parametrize("dims", [CANON, ("time", "latitude", "member", "longitude")])
def test_members_each_and_pooled(dims, groupby):
    """chunk_steps = 5: the chunk of flat steps 15..19 spans the member break at 16"""
    c, flag4, var4 = dataset4(dims)
    uniq, ids = _ids(groupby)
    G = 1 if ids is None else len(uniq)
    each = [cu.composite(flag4[m], var4[m], ids, G) for m in range(3)]
    s = np.stack([e[0] for e in each])                                         # (member, group, lat, lon)
    n = np.stack([e[1] for e in each])
    have = ("member", groupby, "latitude", "longitude")
    want_dims = tuple(groupby if d == "time" else d for d in dims if d != "time" or groupby is not None)
    sort = [have.index(d) for d in want_dims] if groupby else None
    for chunk_steps in (None, 5, 100):
        tot, cnt = c.calc_composite("t2m", groupby=groupby, stat="sum", return_count=True, chunk_steps=chunk_steps)
        assert tuple(tot.dims) == want_dims == tuple(cnt.dims)
        assert np.array_equal(np.asarray(tot.coords["member"]), [10, 20, 30])
        pick = (lambda a: a.transpose(sort)) if groupby else (lambda a: a[:, 0].transpose([(("member",) + TLL[1:]).index(d) for d in want_dims]))
        assert np.array_equal(np.asarray(cnt.data), pick(n)), chunk_steps
        assert cu.same_bits(np.asarray(tot.data), pick(s)), chunk_steps
    # pooled: one composite over the flattened slab, member after member
    flat_f, flat_v = flag4.reshape((-1,) + flag4.shape[2:]), var4.reshape((-1,) + var4.shape[2:])
    ps, pn = cu.composite(flat_f, flat_v, None if ids is None else np.tile(ids, 3), G)
    pdims = tuple(d for d in want_dims if d != "member")
    psort = [(((groupby,) if groupby else ()) + TLL[1:]).index(d) for d in pdims]
    for chunk_steps in (None, 5):
        m, cnt = c.calc_composite("t2m", groupby=groupby, pool=True, return_count=True, chunk_steps=chunk_steps)
        assert tuple(m.dims) == pdims and "member" not in m.coords
        sq = (lambda a: a) if groupby else (lambda a: a[0])
        assert np.array_equal(np.asarray(cnt.data), sq(pn).transpose(psort))
        assert cu.same_bits(np.asarray(m.data), sq(_mean(ps, pn)).transpose(psort))


def test_variable_with_other_dims_is_refused():
    c, flag4, var4 = dataset4(CANON)
    c.ds["t3"] = minixr.DataArray(var4[0], TLL, attrs={"units": "K"})
    with pytest.raises(ValueError, match="they must be the same"):
        c.calc_composite("t3")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_anomaly_after_calc_anom(monkeypatch, dtype):
    """the anomaly calc_anom left in HBM is the field: composite_numpy gets x = None, only the flags are uploaded -- same bits as the
    call with the host array"""
    g, flag4, var4 = members(dtype)
    raw = (var4[0] / np.abs(var4[0]).max() * 300).astype(dtype)
    ds = minixr.make_dataset(raw, g["lat"], g["lon"], time=_time(16), var="z", time_units="days since 2000-10-20")
    ds["flag"] = minixr.DataArray(flag4[0], TLL, attrs={"units": "flag"})
    c = cm.contrack(ds=ds)
    c.calc_anom("z", window=1, smooth=1, groupby="month")
    anom = np.asarray(c.ds["anom"].data)
    assert anom.dtype == dtype
    uniq, ids = _ids("season")
    s, n = cu.composite(flag4[0], anom, ids, len(uniq))
    seen = []
    inner = cm.composite_numpy

    def spy(flag, x, *a, **kw):
        seen.append(x is None)
        return inner(flag, x, *a, **kw)
    monkeypatch.setattr(cm, "composite_numpy", spy)
    got = c.calc_composite("anom", groupby="season", stat="sum")
    assert seen == [True] and cu.same_bits(np.asarray(got.data), s)
    keep, c._anom_resident = c._anom_resident, None                            # the host-array path
    again = c.calc_composite("anom", groupby="season", stat="sum")
    c._anom_resident = keep
    assert seen == [True, False] and cu.same_bits(np.asarray(again.data), s)
    got = c.calc_composite("z", groupby="season", stat="sum")                  # another variable is not the resident slab
    assert seen == [True, False, False] and cu.same_bits(np.asarray(got.data), cu.composite(flag4[0], raw, ids, len(uniq))[0])


@pytest.mark.parametrize("groupby", [None, "season"])
def test_count_is_the_frequency(groupby):
    """n x 100 / group size is calc_frequency on the same flag"""
    c, flag, var = single()
    uniq, ids = _ids(groupby)
    size = np.array([16]) if ids is None else np.bincount(ids)
    for above in (0, 1):
        _, cnt = c.calc_composite("t2m", groupby=groupby, above=above, return_count=True)
        freq = c.calc_frequency("flag", groupby=groupby, above=above)
        n = np.asarray(cnt.data).astype(np.float64)
        want = n / size[0] * 100 if ids is None else n / size[:, None, None] * 100
        assert cu.same_bits(want, np.asarray(freq.data)) and tuple(cnt.dims) == tuple(freq.dims)
