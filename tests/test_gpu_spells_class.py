"""contrack.calc_spells on the xarray stand-in: events, steps, longest and mean duration of the blocked spells per grid point as
labelled arrays over the flag variable's own dims -- after run_contrack, per time.<groupby>, with the breaks of a gappy time axis
and over a member dimension."""
import numpy as np
import pytest

import freq_util
import golden_util
import minixr
import spell_util
from contrack_amd.contrack import contrack, season_of_month

pytestmark = pytest.mark.gpu

minixr.install_as_xarray()          # only when the real package is absent

KEYS = ('events', 'steps', 'longest', 'duration')
UNITS = {'events': '1', 'steps': 'timesteps', 'longest': 'timesteps', 'duration': 'timesteps'}


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


def _duration_bits(res):
    steps, events = np.asarray(res['steps'].data), np.asarray(res['events'].data)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = steps.astype(np.float64) / events.astype(np.float64)
    got = np.asarray(res['duration'].data)
    assert got.dtype == np.float64 and freq_util.same_bits(got, want)
    assert np.isnan(got[events == 0]).all() and not np.isnan(got[events > 0]).any()


@pytest.mark.parametrize("groupby", [None, 'month', 'season', 'year'])
def test_after_run_contrack(groupby):
    c, g = _tracked()
    flag = g["flag"]
    fda = c.ds['flag']
    month, year = _months_years(np.asarray(c.ds['time'].data))
    for by_id, min_duration in ((True, 1), (False, 2)):
        res = c.calc_spells(groupby=groupby, by_id=by_id, min_duration=min_duration)
        assert sorted(res) == sorted(KEYS)
        assert c.variables == ['anom', 'flag']                                    # nothing is added to the dataset
        if groupby is None:
            dims, uniq = ('latitude', 'longitude'), None
            want = [a[0] for a in spell_util.spells(flag, None, 1, 0, by_id, min_duration)]
        else:
            vals = {'month': month, 'year': year, 'season': season_of_month(month)}[groupby]
            uniq, ids = np.unique(vals, return_inverse=True)
            dims = (groupby, 'latitude', 'longitude')
            want = spell_util.spells(flag, ids, len(uniq), 0, by_id, min_duration)
            if groupby == 'season':
                assert list(uniq) == sorted(set(uniq)) and set(uniq) <= {'DJF', 'JJA', 'MAM', 'SON'}
        assert dims == tuple(groupby if d == 'time' else d for d in fda.dims if d != 'time' or groupby is not None)
        for key, w in zip(KEYS[:3], want):
            r = res[key]
            assert tuple(r.dims) == dims, key
            assert np.asarray(r.data).dtype == np.int64 and np.array_equal(np.asarray(r.data), w), (key, by_id, min_duration)
        for key in KEYS:
            r = res[key]
            assert tuple(r.dims) == dims and r.attrs['units'] == UNITS[key] and 'Calculated from flag' in r.attrs['history'], key
            for d in ('latitude', 'longitude'):
                assert np.array_equal(np.asarray(r.coords[d]), np.asarray(c.ds[d].data)), (key, d)
            if groupby is not None:
                assert list(np.asarray(r.coords[groupby])) == list(uniq), key
        assert np.asarray(res['events'].data).sum() > 0 and np.asarray(res['longest'].data).max() > 1
        _duration_bits(res)


def _dataset_with_flag(flag, lat, lon, dims, time, dtype=np.int32):
    ds = minixr.make_dataset(np.zeros(flag.shape, np.float32), lat, lon, time=time, time_units="days since 2000-10-20")
    order = [("time", "latitude", "longitude").index(d) for d in dims]
    ds["blocks"] = minixr.DataArray(flag.astype(dtype).transpose(order), dims, attrs={"units": "flag"})
    return ds


def test_dim_order_int64_and_streamed():
    g = golden_util.load("odd_65x130")
    flag = g["flag"]
    dims = ("longitude", "time", "latitude")
    c = contrack(ds=_dataset_with_flag(flag, g["lat"], g["lon"], dims, _time(flag.shape[0], 17), np.int64))
    month, _ = _months_years(np.asarray(c.ds['time'].data))
    uniq, ids = np.unique(month, return_inverse=True)
    want = spell_util.spells(flag, ids, len(uniq), 1, True, 2)
    for chunk_steps in (None, 7):
        res = c.calc_spells(flag="blocks", groupby='month', above=1, min_duration=2, chunk_steps=chunk_steps)
        for key, w in zip(KEYS[:3], want):
            assert tuple(res[key].dims) == ("longitude", "month", "latitude")
            assert np.array_equal(np.asarray(res[key].data), w.transpose(2, 0, 1)), (key, chunk_steps)
        _duration_bits(res)
    c.ds["blocks"].data[3, 4, 5] = 2 ** 40
    with pytest.raises(ValueError, match="int32"):
        c.calc_spells(flag="blocks")


def test_gaps_cut_exactly_the_bridging_spell():
    """a DJF-only axis: 12 daily steps to 28 February, then 12 from 1 December.  Pixel (0, 0) is blocked over the last three days of
    February and the first three of December -- one spell of 6 without breaks, two of 3 with segments='gaps'; the spells of pixels
    (1, 1) and (2, 2) lie inside one winter and do not change"""
    time = np.concatenate([np.datetime64("2001-02-17") + np.arange(12), np.datetime64("2001-12-01") + np.arange(12)]).astype("datetime64[ns]")
    flag = np.zeros((24, 3, 4), dtype=np.int32)
    flag[9:15, 0, 0] = 5
    flag[2:7, 1, 1] = 6
    flag[12:20, 2, 2] = 7
    c = contrack(ds=_dataset_with_flag(flag, np.array([50.0, 51.0, 52.0]), np.arange(4.0), ("time", "latitude", "longitude"), time))
    plain = c.calc_spells(flag="blocks")
    gaps = c.calc_spells(flag="blocks", segments='gaps')
    starts = c.calc_spells(flag="blocks", segments=[0, 12])
    for key, a, b in (('events', 1, 2), ('steps', 6, 6), ('longest', 6, 3), ('duration', 6.0, 3.0)):
        p, q = np.asarray(plain[key].data), np.asarray(gaps[key].data)
        assert p[0, 0] == a and q[0, 0] == b, key
        differs = ~((p == q) | (np.isnan(p) & np.isnan(q)))
        assert np.array_equal(np.argwhere(differs), [[0, 0]] if a != b else np.zeros((0, 2), dtype=np.int64)), key
        assert freq_util.same_bits(np.asarray(starts[key].data), q), key
    for key, w in zip(KEYS[:3], spell_util.spells(flag, segments=[0, 12])):
        assert np.array_equal(np.asarray(gaps[key].data), w[0]), key
    # by season: the December half of the cut spell is a DJF event of its own; the group dim takes the time dim's place
    s = c.calc_spells(flag="blocks", groupby='season', segments='gaps')
    assert tuple(s['events'].dims) == ('season', 'latitude', 'longitude') and list(np.asarray(s['events'].coords['season'])) == ['DJF']
    assert np.asarray(s['events'].data)[0, 0, 0] == 2


MEMBER_DIMS = ("latitude", "member", "time", "longitude")
CANON = ("member", "time", "latitude", "longitude")


def _members():
    """three members of (19, 5, 6), the member dim in a non-leading position; member 1 ends and member 2 begins blocked at pixel
    (0, 0) with the same id (and is unblocked there otherwise), which one spell would bridge if the members were not segments of
    their own"""
    M, T, ny, nx = 3, 19, 5, 6
    flag4 = np.stack([spell_util.spell_flags(T, ny, nx, seed=40 + m) for m in range(M)])
    flag4[1:, :, 0, 0] = 0
    flag4[1, -3:, 0, 0] = 2
    flag4[2, :4, 0, 0] = 2
    lat, lon = 40.0 + np.arange(ny), 10.0 * np.arange(nx)
    time = _time(T, 9)
    ds = minixr.make_dataset(np.zeros((T, ny, nx), np.float32), lat, lon, time=time, time_units="days since 2000-10-20")
    ds["member"] = minixr.DataArray(np.array([10, 20, 30]), ("member",), attrs={})
    ds["flag"] = minixr.DataArray(flag4.transpose([CANON.index(d) for d in MEMBER_DIMS]), MEMBER_DIMS)
    c = contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    singles = []
    for m in range(M):
        d1 = minixr.make_dataset(np.zeros((T, ny, nx), np.float32), lat, lon, time=time, time_units="days since 2000-10-20")
        d1["flag"] = minixr.DataArray(flag4[m], ("time", "latitude", "longitude"))
        c1 = contrack(ds=d1)
        c1.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
        singles.append(c1)
    return c, singles, flag4


@pytest.mark.parametrize("groupby", [None, 'month'])
def test_member_dimension(groupby):
    c, singles, flag4 = _members()
    M, T = flag4.shape[:2]
    kw = dict(groupby=groupby, by_id=True, min_duration=2)
    res = c.calc_spells(**kw)
    dims = tuple(groupby if d == "time" else d for d in MEMBER_DIMS if d != "time" or groupby is not None)
    ones = [s.calc_spells(**kw) for s in singles]
    for key in KEYS:
        r = res[key]
        assert tuple(r.dims) == dims, key
        assert np.array_equal(np.asarray(r.coords["member"]), [10, 20, 30])
        for m in range(M):                                                        # every member as that member alone
            part = np.take(np.asarray(r.data), m, axis=dims.index("member"))
            one = ones[m][key]
            sub = tuple(d for d in dims if d != "member")
            assert freq_util.same_bits(part, np.asarray(one.data).transpose([tuple(one.dims).index(d) for d in sub])), (key, m)
    for m in range(M):                                                            # ... which is spell_util on its slab
        ids, G = (None, 1) if groupby is None else (singles[m]._group_ids(groupby)[0], len(singles[m]._group_ids(groupby)[1]))
        for key, w in zip(KEYS[:3], spell_util.spells(flag4[m], ids, G, 0, True, 2)):
            got = np.asarray(ones[m][key].data)
            assert np.array_equal(got, w[0] if groupby is None else w), (key, m)
    # the run of id 2 at pixel (0, 0) over the member break is two spells: 3 steps in member 1, 4 in member 2
    if groupby is None:
        lg = np.asarray(res['longest'].data).transpose([dims.index(d) for d in ("member", "latitude", "longitude")])
        assert lg[1, 0, 0] == 3 and lg[2, 0, 0] == 4
        flat = flag4.reshape((-1,) + flag4.shape[2:])
        assert spell_util.spells(flat, None, 1, 0, True, 2)[2][0, 0, 0] == 7      # what one unbroken series would give
    # pooled: events and steps add up, longest is the maximum
    pooled = c.calc_spells(pool=True, **kw)
    pdims = tuple(d for d in dims if d != "member")
    ax = dims.index("member")
    for key in KEYS:
        assert tuple(pooled[key].dims) == pdims, key
    assert np.array_equal(np.asarray(pooled['events'].data), np.asarray(res['events'].data).sum(axis=ax))
    assert np.array_equal(np.asarray(pooled['steps'].data), np.asarray(res['steps'].data).sum(axis=ax))
    assert np.array_equal(np.asarray(pooled['longest'].data), np.asarray(res['longest'].data).max(axis=ax))
    _duration_bits(pooled)
    _duration_bits(res)
    # chunks of 5 flat steps: the chunk of steps 15..19 spans members 0 and 1 (break at 19), 35..39 members 1 and 2 (break at 38)
    for chunk_steps in (5, 1, 100):
        for pool, ref in ((False, res), (True, pooled)):
            got = c.calc_spells(pool=pool, chunk_steps=chunk_steps, **kw)
            for key in KEYS:
                assert tuple(got[key].dims) == tuple(ref[key].dims)
                assert freq_util.same_bits(np.asarray(got[key].data), np.asarray(ref[key].data)), (key, chunk_steps, pool)
    # the member dimension by name changes nothing; breaks inside the members are kept per member
    named = c.calc_spells(segments="member", **kw)
    cut = c.calc_spells(segments=[0, 7], **kw)
    cut_ones = [s.calc_spells(segments=[0, 7], **kw) for s in singles]
    for key in KEYS:
        assert freq_util.same_bits(np.asarray(named[key].data), np.asarray(res[key].data)), key
        for m in range(M):
            part = np.take(np.asarray(cut[key].data), m, axis=ax)
            one = cut_ones[m][key]
            assert freq_util.same_bits(part, np.asarray(one.data).transpose([tuple(one.dims).index(d) for d in pdims])), (key, m)
