"""GPU-free parts of the streamed / member forms of run_lifecycle and calc_frequency: the rounding-boundary rule in one place
(fragile_rows), lifecycle_columns fed with the records of a streamed call (exact=), the member column and the row order, and the
argument errors the class raises before it touches the library."""
import numpy as np
import pytest

import life_util
import minixr
from contrack_amd import contrack as cm
from contrack_amd._native import LIFE_ROW
from contrack_amd.contrack import fragile_rows, lifecycle_columns, lifecycle_frame

minixr.install_as_xarray()
GOLDEN = life_util.case_names()


class FakeTracker:
    """lifecycle_exact as the library answers it, from numpy's own calls; remembers what it was asked for"""

    def __init__(self, flag, field, wrow, rows):
        self.args, self.rows, self.asked = (flag, field, wrow), rows, []

    def lifecycle_exact(self, idx):
        self.asked.append(np.asarray(idx).copy())
        return life_util.numpy_exact_rows(*self.args, self.rows[idx])


def cases():
    for name in GOLDEN:
        g = life_util.load(name)
        yield name, g["flag"], g["variable"], g["lat"], g["lon"], g["wrow"], life_util.dates_of(g["time"])
    for i in range(40):
        yield ("random%d" % i,) + life_util.random_life_case(i)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_fragile_rows_is_the_rule_of_lifecycle_columns(case):
    name, flag, field, lat, lon, wrow, dates = case
    rows = life_util.numpy_rows(flag, field, wrow)
    fake = FakeTracker(flag, field, wrow, rows)
    with_tracker = lifecycle_columns(rows, lat, lon, dates, tracker=fake)
    idx = fragile_rows(rows)
    assert idx.dtype == np.int64 and np.all(np.diff(idx) > 0)
    if len(idx):
        assert len(fake.asked) == 1 and np.array_equal(fake.asked[0], idx)
    else:
        assert fake.asked == []
    # ... and the records of a streamed call, handed over, give the same columns
    ex = life_util.numpy_exact_rows(flag, field, wrow, rows[idx])
    streamed = lifecycle_columns(rows, lat, lon, dates, exact=(idx, ex))
    assert list(streamed) == list(with_tracker) == ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size']
    for k in streamed:
        assert np.array_equal(streamed[k], with_tracker[k]), k
    assert lifecycle_frame(rows, lat, lon, dates, exact=(idx, ex)) == lifecycle_frame(rows, lat, lon, dates, fake)


def test_fragile_rows_picks_boundaries_only():
    r = np.zeros(4, dtype=LIFE_ROW)
    r["area"], r["swv"], r["swvy"], r["swvx"] = 3.0, 7.0, 7.0 * 2.25, 7.0 * 5.75           # nothing near a boundary
    r["swvy"][1] = 7.0 * 3.0                                                              # an integer centre of mass
    r["swv"][2], r["swvy"][2], r["swvx"][2] = 3.0 * 1.005, 3.0 * 1.005 * 2.25, 3.0 * 1.005 * 5.75     # intensity x.xx5
    r["swv"][3] = 0.0                                                                     # no centre of mass at all
    assert fragile_rows(r).tolist() == [1, 2, 3]
    assert fragile_rows(r[:0]).tolist() == [] and fragile_rows(r[:0]).dtype == np.int64


def hand_rows(entries):
    """(flat t, label) -> rows whose centre of mass is (1.5, 2.5) and whose area tells them apart"""
    r = np.zeros(len(entries), dtype=LIFE_ROW)
    for i, (t, label) in enumerate(entries):
        r[i] = (t, label, -1, 0, 100.0 + i, 2.0, 3.0, 5.0)
    return r[np.lexsort((r["t"], r["label"]))]                                            # the library's order: (label, flat t)


def test_member_column_and_order():
    lat, lon = np.linspace(80, 20, 4), np.arange(0.0, 60.0, 10.0)
    T = 3
    dates = ["d0", "d1", "d2"]
    # ids 7 and 9 live in member 0, 1007 in member 1, and id 7 is repeated in member 2
    rows = hand_rows([(0, 7), (1, 7), (2, 9), (T + 0, 1007), (T + 2, 1007), (2 * T + 1, 7), (2 * T + 0, 7)])
    c = lifecycle_columns(rows, lat, lon, dates, period=T)
    assert list(c) == ['Flag', 'Date', 'Longitude', 'Latitude', 'Intensity', 'Size', 'Member']
    got = list(zip(c["Flag"].tolist(), c["Member"].tolist(), c["Date"].tolist()))
    assert got == [(7, 0, "d0"), (7, 0, "d1"), (7, 2, "d0"), (7, 2, "d1"), (9, 0, "d2"), (1007, 1, "d0"), (1007, 1, "d2")]
    assert got == sorted(got)                                                             # (Flag, member position, Date)
    assert c["Longitude"].tolist() == [20] * 7 and c["Latitude"].tolist() == [60] * 7
    # without a period the same rows are a plain series of 9 steps: no member column
    plain = lifecycle_columns(rows, lat, lon, ["s%d" % t for t in range(3 * T)])
    assert "Member" not in plain and plain["Date"].tolist() == ["s0", "s1", "s6", "s7", "s2", "s3", "s5"]


def test_tiled_dates_do_not_take_the_unsorted_path(monkeypatch):
    """T increasing labels, M members: the rows stay in the library's order and Python's sort is never entered; a time axis that
    is not increasing is sorted by (Flag, member, Date string)"""
    lat, lon = np.linspace(80, 20, 4), np.arange(0.0, 60.0, 10.0)
    rows = hand_rows([(0, 5), (2, 5), (3, 5), (4, 5), (5, 2)])
    import builtins
    monkeypatch.setattr(cm, "sorted", lambda *a, **k: pytest.fail("the Python sort ran"), raising=False)
    c = lifecycle_columns(rows, lat, lon, ["a", "b", "c"], period=3)
    assert list(zip(c["Flag"].tolist(), c["Member"].tolist(), c["Date"].tolist())) == [(2, 1, "c"), (5, 0, "a"), (5, 0, "c"), (5, 1, "a"), (5, 1, "b")]
    monkeypatch.setattr(cm, "sorted", builtins.sorted, raising=False)
    c = lifecycle_columns(rows, lat, lon, ["z", "y", "x"], period=3)
    assert list(zip(c["Flag"].tolist(), c["Member"].tolist(), c["Date"].tolist())) == [(2, 1, "x"), (5, 0, "x"), (5, 0, "z"), (5, 1, "y"), (5, 1, "z")]
    assert c["Size"].tolist() == [104.0, 101.0, 100.0, 103.0, 102.0]                        # the other columns moved with them


# ---- the class refuses before it calls the library ------------------------------------------------------------------------
class Forbidden:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s)" % name)


def dataset(flag_dims, var_dims, sizes=dict(time=4, latitude=5, longitude=8, member=2, level=3)):
    lat = np.linspace(60, 20, sizes["latitude"]).astype(np.float32)
    lon = (np.arange(sizes["longitude"]) * 45.0).astype(np.float32)
    days = (np.datetime64("2000-01-01") + np.arange(sizes["time"])).astype("datetime64[ns]")
    ds = minixr.make_dataset(np.zeros((sizes["time"], len(lat), len(lon)), np.float32), lat, lon, time=days)
    ds["flag"] = minixr.DataArray(np.zeros([sizes[d] for d in flag_dims], np.int32), flag_dims)
    ds["z"] = minixr.DataArray(np.zeros([sizes[d] for d in var_dims], np.float32), var_dims)
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    return c


TLL = ("time", "latitude", "longitude")


@pytest.mark.parametrize("chunk_steps", [None, 2])
@pytest.mark.parametrize("flag_dims,var_dims", [
    (("member", "level") + TLL, ("member", "level") + TLL),              # a 5-D flag
    (("member",) + TLL, ("level",) + TLL),                               # a variable with other dims
    (TLL, ("member",) + TLL),                                            # an extra dim on the variable only
    (("member",) + TLL, TLL),                                            # ... or on the flag only
])
def test_run_lifecycle_argument_errors_come_first(monkeypatch, flag_dims, var_dims, chunk_steps):
    monkeypatch.setattr(cm, "_tracker", lambda device=None: Forbidden())
    c = dataset(flag_dims, var_dims)
    with pytest.raises(ValueError, match="dim"):
        c.run_lifecycle("flag", "z", chunk_steps=chunk_steps)


def test_other_argument_errors_come_first(monkeypatch):
    monkeypatch.setattr(cm, "_tracker", lambda device=None: Forbidden())
    c = dataset(("member", "level") + TLL, TLL)
    with pytest.raises(ValueError, match="dim"):
        c.calc_frequency("flag")
    c = dataset(("member",) + TLL, ("member",) + TLL)
    with pytest.raises(ValueError, match="integer"):
        c.run_lifecycle("z", "z")                                        # a float field as the flag
    with pytest.raises(ValueError, match="integer"):
        c.calc_frequency("z", chunk_steps=2)
