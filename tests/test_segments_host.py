"""Segment breaks on the Python side, without a GPU: which starts run_contrack / track_numpy hand to the tracker ('gaps' on a DJF
time axis, a member dimension flattened and transposed back, the thresholds tiled over members), the validation errors, and the
C entry exported by the built library."""
import importlib

import numpy as np
import pytest

import minixr
from contrack_amd import _native

cm = importlib.import_module("contrack_amd.contrack")

minixr.install_as_xarray()          # only when the real package is absent


class FakeTracker:
    """records the segments, thresholds and slabs it is handed; returns flag = the step index + 1 everywhere (so that the caller's
    reshaping and transposing of the result can be checked)"""

    def __init__(self):
        self.field = None
        self.segments = None
        self.calls = []

    def set_threshold_field(self, field, plane_of_step):
        self.field = (np.array(field), np.array(plane_of_step))

    def clear_threshold_field(self):
        self.field = None

    def set_segments(self, starts):
        self.segments = np.array(starts)

    def clear_segments(self):
        self.segments = None

    def track(self, anom, thr, *a, **k):
        self.calls.append(dict(anom=np.array(anom), thr=None if thr is None else np.array(thr), field=self.field,
                               segments=self.segments, f64=k.get("f64", False)))
        T = anom.shape[0]
        return np.broadcast_to(np.arange(1, T + 1, dtype=np.int32).reshape(-1, 1, 1), anom.shape).copy(), T

    track_resident = None

    def stats(self):
        return {}

    def release_io(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    f = FakeTracker()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: f)
    return f


def djf_days(years):
    out = []
    for y in years:
        out.append(np.arange(np.datetime64("%d-12-01" % y), np.datetime64("%d-03-01" % (y + 1)), dtype="datetime64[D]"))
    return np.concatenate(out)


def grid(ny=5, nx=8):
    return np.linspace(80, 40, ny).astype(np.float32), (np.arange(nx) * 45.0).astype(np.float32)


def test_gap_starts():
    assert cm.gap_starts(np.array([1, 1, 1])).tolist() == [0]
    assert cm.gap_starts(np.array([24, 24, 72, 24, 48])).tolist() == [0, 3, 5]
    assert cm.gap_starts(np.array([], dtype=np.int64)).tolist() == [0]


def test_gaps_on_djf_axis(fake):
    days = djf_days([2000, 2001, 2002])
    lat, lon = grid()
    a = np.zeros((len(days), len(lat), len(lon)), dtype=np.float32)
    c = cm.contrack(ds=minixr.make_dataset(a, lat, lon, time=days.astype("datetime64[ns]")))
    c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments='gaps')
    lens = [len(djf_days([y])) for y in (2000, 2001, 2002)]
    assert fake.calls[-1]["segments"].tolist() == [0, lens[0], lens[0] + lens[1]]
    assert fake.segments is None                                  # cleared afterwards
    assert 'segments = gaps (3)' in c.ds['flag'].attrs['history']


def test_gaps_days_since(fake):
    """a numeric 'days since' time axis, decoded as _get_resolution decodes it"""
    t = np.concatenate([np.arange(0, 90), np.arange(365, 455), np.arange(730, 820)]).astype(np.float64)
    lat, lon = grid()
    a = np.zeros((len(t), len(lat), len(lon)), dtype=np.float32)
    c = cm.contrack(ds=minixr.make_dataset(a, lat, lon, time=t, time_units="days since 1990-01-01"))
    c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments='gaps')
    assert fake.calls[-1]["segments"].tolist() == [0, 90, 180]


def test_unsegmented_attrs_unchanged(fake):
    lat, lon = grid()
    a = np.zeros((6, len(lat), len(lon)), dtype=np.float32)
    c = cm.contrack(ds=minixr.make_dataset(a, lat, lon))
    c.run_contrack('anom', 1.0, '>=', 0.5, 2)
    assert fake.calls[-1]["segments"] is None
    assert 'segments' not in c.ds['flag'].attrs['history']
    c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments=[0, 2])
    assert fake.calls[-1]["segments"].tolist() == [0, 2]


def member_dataset(dims, M=3, T=4, ny=5, nx=8, dtype=np.float32):
    lat, lon = grid(ny, nx)
    base = np.zeros((T, ny, nx), dtype=np.float32)
    days = (np.datetime64("2000-01-01") + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(base, lat, lon, time=days)
    canon = ("member", "time", "latitude", "longitude")
    rng = np.random.default_rng(1)
    x = rng.standard_normal((M, T, ny, nx)).astype(dtype)
    ds['member'] = minixr.DataArray(np.arange(M), ("member",), attrs={})
    ds['z'] = minixr.DataArray(x.transpose([canon.index(d) for d in dims]), dims, attrs={"units": "m", "long_name": "z"})
    return ds, x


@pytest.mark.parametrize("dims", [("member", "time", "latitude", "longitude"), ("longitude", "member", "latitude", "time"),
                                  ("time", "latitude", "longitude", "member")])
def test_member_dim_flattened_and_back(fake, dims):
    ds, x = member_dataset(dims)
    M, T = x.shape[:2]
    c = cm.contrack(ds=ds)
    c.run_contrack('z', 0.5, '>=', 0.5, 2, segments='member')
    call = fake.calls[-1]
    assert call["segments"].tolist() == [0, T, 2 * T]
    assert np.array_equal(call["anom"], x.reshape((M * T,) + x.shape[2:]))
    assert call["thr"].shape == (M * T,)
    flag = c.ds['flag']
    assert tuple(flag.dims) == dims
    canon = ("member", "time", "latitude", "longitude")
    back = np.asarray(flag.data).transpose([dims.index(d) for d in canon])
    want = np.broadcast_to((np.arange(M * T) + 1).reshape(M, T, 1, 1), back.shape)
    assert np.array_equal(back, want)


def test_member_thresholds_tiled(fake):
    ds, x = member_dataset(("member", "time", "latitude", "longitude"))
    M, T = x.shape[:2]
    c = cm.contrack(ds=ds)
    vec = np.array([0.1, 0.2, 0.3, 0.4])
    c.run_contrack('z', vec, '>=', 0.5, 2, segments='member')
    assert np.array_equal(fake.calls[-1]["thr"], np.tile(vec, M))
    # a dayofyear field: the plane of every step, tiled over the members
    doy = minixr.DataArray(np.arange(366 * 5 * 8, dtype=np.float32).reshape(366, 5, 8), ("dayofyear", "latitude", "longitude"),
                           coords={"dayofyear": minixr.DataArray(np.arange(1, 367), ("dayofyear",))})
    c.run_contrack('z', doy, '>=', 0.5, 2, segments='member')
    call = fake.calls[-1]
    assert call["thr"] is None
    pos = call["field"][1]
    assert pos.shape == (M * T,) and np.array_equal(pos, np.tile(pos[:T], M))
    with pytest.raises(ValueError, match="member"):
        c.run_contrack('z', np.zeros((5, 8)), '>=', 0.5, 2, segments='member')


def test_validation(fake):
    lat, lon = grid()
    a = np.zeros((6, len(lat), len(lon)), dtype=np.float32)
    c = cm.contrack(ds=minixr.make_dataset(a, lat, lon))
    for bad in ([1, 3], [0, 3, 3], [0, 4, 2], [0, 6], [[0, 1]], [0.0, 2.5]):
        with pytest.raises(ValueError):
            c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments=bad)
    with pytest.raises(ValueError, match="chunk_steps"):
        c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments=[0, 3], chunk_steps=2)
    with pytest.raises(ValueError, match="no such dimension"):
        c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments='member')
    assert fake.calls == []
    with pytest.raises(ValueError):
        cm.track_numpy(a, np.ones(len(lat), dtype=np.float32), 1.0, '>=', 0.5, 2, segments=[0, 7])
    flag, n = cm.track_numpy(a, np.ones(len(lat), dtype=np.float32), 1.0, '>=', 0.5, 2, segments=np.array([0, 1, 5]))
    assert fake.calls[-1]["segments"].tolist() == [0, 1, 5] and fake.segments is None


def test_track_numpy_composes_with_a_field(fake):
    lat, lon = grid()
    a = np.zeros((6, len(lat), len(lon)), dtype=np.float32)
    cm.track_numpy(a, np.ones(len(lat), dtype=np.float32), np.zeros((len(lat), len(lon))), '>=', 0.5, 2, segments=[0, 3])
    call = fake.calls[-1]
    assert call["thr"] is None and call["field"] is not None and call["segments"].tolist() == [0, 3]
    assert fake.field is None and fake.segments is None


def test_abi_exports_set_segments():
    L = _native.lib()
    assert hasattr(L, "ctk_set_segments")
    assert "ctk_set_segments" in _native.EXPORTS
    assert L.ctk_set_segments(None, None, 0) == -1                 # null handle: CTK_E_INVALID, no device needed
