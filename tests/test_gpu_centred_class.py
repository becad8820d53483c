"""contrack.calc_centred_composite on the xarray stand-in (tests/minixr.py): run_contrack on a small synthetic slab, the life-cycle
frame with its index columns (run_lifecycle(indices=True)), then the composite in the blocks' own frame of reference against the
numpy statement of tests/centred_util.py fed from the frame's own Step / Row / Col -- the sums bit for bit, the counts exactly, the
mean as sum / n.  The composited variable spans 18 orders of magnitude, so a sum in another order or in float32 shows in the bits."""
import functools

import numpy as np
import pytest

import centred_util as cu
import minixr
from contrack_amd import contrack as cm
from contrack_amd import synth

minixr.install_as_xarray()
pytestmark = pytest.mark.gpu
TLL = ("time", "latitude", "longitude")
SIX = ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']
T, NY, NX = 24, 45, 90                                                          # a 4-degree grid, 88 N .. 88 S
LAT, LON = 88.0 - 4.0 * np.arange(NY), 4.0 * np.arange(NX)
HALF = (12.0, 20.0)                                                             # degrees: 3 x 5 grid points


def _time(n=T):
    return (np.datetime64("2001-01-01") + np.arange(n)).astype("datetime64[D]").astype("datetime64[ns]")


def _wide(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-8, 10, shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def tracked():
    """(contrack instance with 'anom', 'flag', 'wide' (float32) and 'wide64', the frame with index columns)"""
    anom = synth.smooth_field(T, NY, NX, seed=5)
    ds = minixr.make_dataset(anom, LAT, LON, time=_time())
    ds["time"].attrs = {}
    ds["wide"] = minixr.DataArray(_wide(anom.shape, np.float32, 1), TLL, attrs={"units": "K", "long_name": "2 m temperature"})
    ds["wide64"] = minixr.DataArray(_wide(anom.shape, np.float64, 2), TLL, attrs={"units": "mm"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    c.run_contrack(variable='anom', threshold=100.0, gorl='>=', overlap=0.4, persistence=3)
    df = c.run_lifecycle("flag", "anom", indices=True)
    assert len(df) >= 12 and len(df.Flag.unique()) >= 2, "the synthetic slab must give a few blocks of a few steps"
    return c, df


def _statement(var, df, by, nbins=None, max_age=None, half=(3, 5), t=None, block=None, **kw):
    step = df["Step"].to_numpy()
    t = step if t is None else t
    bins, nb = cm.lifecycle_bins(df["Flag"].to_numpy() if block is None else block, step, by, nbins=nbins, max_age=max_age)
    order = np.argsort(t, kind="stable")
    s, n = cu.centred(var, t[order], df["Row"].to_numpy()[order], df["Col"].to_numpy()[order], bins[order], nb, half[0], half[1], **kw)
    return s, n, nb


def _data(a):
    return np.asarray(a.data)


def test_run_lifecycle_index_columns():
    c, df = tracked()
    plain = c.run_lifecycle("flag", "anom")
    assert list(plain.columns) == SIX                                          # without the keyword: exactly today's columns
    assert list(df.columns) == SIX + ['Step', 'Row', 'Col']
    assert plain.equals(df[SIX])
    for k in ('Step', 'Row', 'Col'):
        assert df[k].dtype == np.int64
    labels = c._time_labels()
    assert [labels[s] for s in df["Step"]] == list(df["Date"])
    assert np.array_equal(np.trunc(LAT[df["Row"].to_numpy()]).astype(np.int64), df["Latitude"].to_numpy())
    assert np.array_equal(np.trunc(LON[df["Col"].to_numpy()]).astype(np.int64), df["Longitude"].to_numpy())
    streamed = c.run_lifecycle("flag", "anom", chunk_steps=5, indices=True)
    assert streamed.equals(df)


@pytest.mark.parametrize("variable", ["wide", "wide64"])
@pytest.mark.parametrize("by,nbins", [(None, None), ("age", None), ("to_lysis", None), ("normalized", 4)])
def test_mean_sum_count_and_labels(by, nbins, variable):
    c, df = tracked()
    var = _data(c.ds[variable])
    s, n, nb = _statement(var, df, by, nbins)
    assert n.max() >= 2 and (by is None or nb >= 3)
    if by is None:
        assert cu.differing(s, _statement(var, df, by, nbins, order="falling")[0]) > 0
    m, cnt = c.calc_centred_composite(variable, df, half_width=HALF, by=by, nbins=nbins, return_count=True)
    assert sorted(c.variables) == ["anom", "flag", "wide", "wide64"]                 # nothing is added to the dataset
    bdim = by if by is not None else "bin"
    assert tuple(m.dims) == (bdim, "rel_latitude", "rel_longitude") == tuple(cnt.dims)
    assert _data(m).dtype == np.float64 and _data(cnt).dtype == np.uint32 and _data(m).shape == (nb, 7, 11)
    assert np.array_equal(_data(cnt), n)
    assert cu.same_bits(_data(m), cu.mean(s, n))
    assert np.array_equal(np.asarray(m.coords[bdim]), np.arange(nb))
    assert np.array_equal(np.asarray(m.coords["rel_latitude"]), np.arange(-3, 4) * -4.0)      # latitude runs north to south
    assert np.array_equal(np.asarray(m.coords["rel_longitude"]), np.arange(-5, 6) * 4.0)
    assert m.attrs["units"] == c.ds[variable].attrs["units"] and "Calculated from " + variable in m.attrs["history"]
    assert "by = {}".format(by) in m.attrs["history"] and cnt.attrs["units"] == "1"
    tot = c.calc_centred_composite(variable, df, half_width=HALF, by=by, nbins=nbins, stat="sum")
    assert cu.same_bits(_data(tot), s) and "stat = sum" in tot.attrs["history"]
    for steps in (1, 5, 100):
        again = c.calc_centred_composite(variable, df, half_width=HALF, by=by, nbins=nbins, stat="sum", chunk_steps=steps)
        assert cu.same_bits(_data(again), s), steps


def test_options_selection_and_fallback(monkeypatch):
    c, df = tracked()
    var = _data(c.ds["wide"])
    # the default window: 20 x 40 degrees are 5 x 10 grid points
    s, n, nb = _statement(var, df, None, half=(5, 10))
    m = c.calc_centred_composite("wide", df)
    assert _data(m).shape == (1, 11, 21) and cu.same_bits(_data(m), cu.mean(s, n))
    # max_age cuts the axis; skipna and wrap reach the kernel
    vn = var.copy()
    vn[::3] = np.nan
    c.ds["wide"].data[...] = vn
    try:
        for kw in (dict(), dict(skipna=True), dict(wrap=False), dict(skipna=True, wrap=False)):
            s, n, nb = _statement(vn, df, "age", max_age=2, **kw)
            m, cnt = c.calc_centred_composite("wide", df, half_width=HALF, by="age", max_age=2, return_count=True, **kw)
            assert nb == 3 and np.array_equal(_data(cnt), n) and cu.same_bits(_data(m), cu.mean(s, n)), kw
    finally:
        c.ds["wide"].data[...] = var
    # a row selection of the frame: the blocks of the northern hemisphere, and the long-lived ones -- ages count among the rows given
    long_lived = df.groupby("Flag")["Step"].transform("count") >= 4
    for pick in (df[df["Latitude"] > 0], df[long_lived], df.iloc[::-1], df.iloc[:0]):
        s, n, nb = _statement(var, pick, "age", nbins=6)
        tot, cnt = c.calc_centred_composite("wide", pick, half_width=HALF, by="age", nbins=6, stat="sum", return_count=True)
        assert np.array_equal(_data(cnt), n) and cu.same_bits(_data(tot), s)
    # bins given: a column of the frame by name, or an array
    marked = df.assign(sector=(df["Col"].to_numpy() * 3 // NX).astype(np.int64))
    s, n, nb = _statement(var, marked, marked["sector"].to_numpy(), nbins=3)
    tot = c.calc_centred_composite("wide", marked, half_width=HALF, by="sector", nbins=3, stat="sum")
    assert tuple(tot.dims)[0] == "sector" and cu.same_bits(_data(tot), s)
    tot = c.calc_centred_composite("wide", df, half_width=HALF, by=marked["sector"].to_numpy() - 1, nbins=2, stat="sum")      # sector 0 is dropped
    assert tuple(tot.dims)[0] == "bin" and cu.same_bits(_data(tot), s[1:])
    # without the index columns: Date is looked up, Latitude / Longitude go to the nearest grid index
    six = df[SIX]
    near = df.assign(Row=np.abs(LAT[None, :] - six["Latitude"].to_numpy()[:, None]).argmin(axis=1),
                     Col=np.abs(LON[None, :] - six["Longitude"].to_numpy()[:, None]).argmin(axis=1))
    s, n, nb = _statement(var, near, "to_lysis")
    tot = c.calc_centred_composite("wide", six, half_width=HALF, by="to_lysis", stat="sum")
    assert cu.same_bits(_data(tot), s)
    monkeypatch.setattr(c, "_time_labels", lambda: ["same"] * T)
    with pytest.raises(ValueError, match="not unique"):
        c.calc_centred_composite("wide", six)
    c.calc_centred_composite("wide", df)                                       # (the index columns need no labels)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="stat must be"):
        c.calc_centred_composite("wide", df, stat="median")
    with pytest.raises(ValueError, match="twice"):
        c.calc_centred_composite("wide", df, half_width=(12.0, 184.0))        # 2 * 46 + 1 columns on a periodic grid of 90
    with pytest.raises(ValueError):
        c.calc_centred_composite("wide", df, by="onset")


def test_member_dimension():
    """two members tracked in one call (segments='member'); the stamps' t is m * T + Step, the flattening the other consumers use"""
    M = 2
    anom = np.stack([synth.smooth_field(T, NY, NX, seed=s) for s in (5, 6)])
    for dims in (("member",) + TLL, ("time", "latitude", "member", "longitude")):
        order = [(("member",) + TLL).index(d) for d in dims]
        ds = minixr.make_dataset(np.zeros((T, NY, NX), np.float32), LAT, LON, time=_time(), var="unused")
        ds["time"].attrs = {}
        ds["member"] = minixr.DataArray(np.array([10, 20]), ("member",), attrs={})
        ds["z"] = minixr.DataArray(anom.transpose(order), dims, attrs={"units": "m"})
        wide = _wide(anom.shape, np.float32, 3)
        ds["wide"] = minixr.DataArray(wide.transpose(order), dims, attrs={"units": "K"})
        c = cm.contrack(ds=ds)
        c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
        c.run_contrack('z', 100.0, '>=', 0.4, 3, segments='member')
        df = c.run_lifecycle("flag", "z", indices=True)
        assert list(df.columns) == SIX + ["member", 'Step', 'Row', 'Col'] and set(df["member"]) == {10, 20}
        assert df["Step"].max() < T
        m_of = (df["member"].to_numpy() // 10 - 1).astype(np.int64)
        flat = wide.reshape((M * T, NY, NX))
        for by, nbins in ((None, None), ("age", None), ("normalized", 3)):
            s, n, nb = _statement(flat, df, by, nbins, t=m_of * T + df["Step"].to_numpy(), block=list(zip(df["Flag"].tolist(), m_of.tolist())))
            for chunk_steps in (None, 5, 100):                                 # (a chunk of 5 spans the member break at 24)
                tot, cnt = c.calc_centred_composite("wide", df, half_width=HALF, by=by, nbins=nbins, stat="sum", return_count=True, chunk_steps=chunk_steps)
                assert np.array_equal(_data(cnt), n) and cu.same_bits(_data(tot), s), (dims, by, chunk_steps)
        with pytest.raises(ValueError, match="needs that column"):
            c.calc_centred_composite("wide", df[SIX + ['Step', 'Row', 'Col']])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_resident_anomaly_after_calc_anom(monkeypatch, dtype):
    """the anomaly calc_anom left in HBM is the field: centred_numpy gets x = None and no field bytes are uploaded -- same bits as the
    call with the host array"""
    raw = synth.smooth_field(T, NY, NX, seed=7).astype(dtype)
    ds = minixr.make_dataset(raw, LAT, LON, time=_time(), var="z")
    ds["time"].attrs = {}
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    c.calc_anom("z", window=1, smooth=1, groupby="month")
    anom = _data(c.ds["anom"])
    assert anom.dtype == dtype
    c.run_contrack('anom', float(np.percentile(anom, 92)), '>=', 0.4, 3)
    df = c.run_lifecycle("flag", "anom", indices=True)
    assert len(df) >= 6
    s, n, nb = _statement(anom, df, "age")
    seen = []
    inner = cm.centred_numpy

    def spy(x, *a, **kw):
        seen.append(x is None)
        return inner(x, *a, **kw)
    monkeypatch.setattr(cm, "centred_numpy", spy)
    got = c.calc_centred_composite("anom", df, half_width=HALF, by="age", stat="sum")
    assert seen == [True] and cu.same_bits(_data(got), s)
    keep, c._anom_resident = c._anom_resident, None                            # the host-array path
    again = c.calc_centred_composite("anom", df, half_width=HALF, by="age", stat="sum")
    c._anom_resident = keep
    assert seen == [True, False] and cu.same_bits(_data(again), s)
    got = c.calc_centred_composite("z", df, half_width=HALF, by="age", stat="sum")     # another variable is not the resident slab
    assert seen == [True, False, False] and cu.same_bits(_data(got), _statement(raw, df, "age")[0])
