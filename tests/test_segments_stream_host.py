"""Segment breaks combined with chunk_steps on the Python side, without a GPU: run_contrack hands the streaming call the right
starts ('gaps', a member dimension), reads a member dimension slice by slice -- never building the flattened slab -- and a chunk
that spans two members in two pieces; track_numpy forwards segments and chunk_steps; the new C entries are exported."""
import importlib

import numpy as np
import pytest

import minixr
from contrack_amd import _native
from test_segments_host import djf_days, grid, member_dataset

cm = importlib.import_module("contrack_amd.contrack")

minixr.install_as_xarray()          # only when the real package is absent


class FakeStreamTracker:
    """track_stream pulls the slab through the reader in chunks, as the library does, and records what it was handed; flag = the
    flat step index + 1 everywhere.  It has no track(): a caller that materialises the slab for a one-call entry fails."""

    def __init__(self):
        self.field = None
        self.calls = []

    def set_threshold_field(self, field, plane_of_step):
        self.field = (np.array(field), np.array(plane_of_step))

    def clear_threshold_field(self):
        self.field = None

    def set_segments(self, starts):
        raise AssertionError("the streaming call takes its segments as an argument, not from the handle")

    def track_stream(self, source, thr, cmp_op, wrow, overlap, persistence, twosided=True, sink=None, shape=None, dtype=None, chunk_steps=0,
                     segments=None):
        if callable(source):
            T, ny, nx = shape
            got = np.full(shape, np.nan, dtype=dtype)
            requests = []
            step = chunk_steps or T
            for t0 in range(0, T, step):
                nt = min(step, T - t0)
                requests.append((t0, nt))
                source(t0, nt, got[t0:t0 + nt])
        else:
            got, requests = np.array(source), None
            T = got.shape[0]
        self.calls.append(dict(anom=got, thr=None if thr is None else np.array(thr), field=self.field, requests=requests,
                               segments=None if segments is None else np.array(segments), chunk_steps=chunk_steps))
        return np.broadcast_to(np.arange(1, T + 1, dtype=np.int32).reshape(-1, 1, 1), got.shape).copy(), T

    def stats(self):
        return {}

    def release_io(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    f = FakeStreamTracker()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: f)
    return f


class Counting:
    """wraps a DataArray: counts isel calls and the largest piece read, refuses to be read as a whole"""

    def __init__(self, da):
        self._da = da
        self.dims, self.shape, self.dtype = da.dims, da.data.shape, da.data.dtype
        self.pieces = []

    @property
    def data(self):
        raise AssertionError("the whole variable was materialised")

    def isel(self, **kw):
        part = self._da.isel(**kw)
        self.pieces.append((dict(kw), part.data.shape))
        return part


@pytest.mark.parametrize("dims", [("member", "time", "latitude", "longitude"), ("longitude", "member", "latitude", "time"),
                                  ("time", "latitude", "longitude", "member")])
def test_member_dim_streams_without_the_flattened_slab(fake, monkeypatch, dims):
    ds, x = member_dataset(dims, M=3, T=4)
    M, T = x.shape[:2]
    c = cm.contrack(ds=ds)
    c._ensure_set_up()
    counting = Counting(ds['z'])
    real_getitem = type(c.ds).__getitem__
    monkeypatch.setattr(type(c.ds), "__getitem__", lambda self, key: counting if key == 'z' else real_getitem(self, key))
    c.run_contrack('z', 0.5, '>=', 0.5, 2, segments='member', chunk_steps=3)          # chunks [0,3) [3,6) [6,9) [9,12): two span members
    call = fake.calls[-1]
    assert call["segments"].tolist() == [0, T, 2 * T] and call["chunk_steps"] == 3
    assert call["requests"] == [(0, 3), (3, 3), (6, 3), (9, 3)]
    assert np.array_equal(call["anom"], x.reshape((M * T,) + x.shape[2:]))         # flat step m * T + t is member m, step t
    assert call["thr"].shape == (M * T,)
    # read member by member, a chunk across two members in two pieces, no piece longer than a chunk
    assert [p[0]["member"] for p in counting.pieces] == [0, 0, 1, 1, 2, 2]
    assert [(p[0]["time"].start, p[0]["time"].stop) for p in counting.pieces] == [(0, 3), (3, 4), (0, 2), (2, 4), (0, 1), (1, 4)]
    assert max(int(np.prod(p[1])) for p in counting.pieces) <= 3 * x.shape[2] * x.shape[3]
    flag = c.ds['flag']
    assert tuple(flag.dims) == dims
    canon = ("member", "time", "latitude", "longitude")
    back = np.asarray(flag.data).transpose([dims.index(d) for d in canon])
    assert np.array_equal(back, np.broadcast_to((np.arange(M * T) + 1).reshape(M, T, 1, 1), back.shape))
    assert 'segments = member (3)' in flag.attrs['history']


def test_member_thresholds_tiled_when_streaming(fake):
    ds, x = member_dataset(("member", "time", "latitude", "longitude"))
    M, T = x.shape[:2]
    c = cm.contrack(ds=ds)
    vec = np.array([0.1, 0.2, 0.3, 0.4])
    c.run_contrack('z', vec, '>=', 0.5, 2, segments='member', chunk_steps=5)
    assert np.array_equal(fake.calls[-1]["thr"], np.tile(vec, M))
    doy = minixr.DataArray(np.arange(366 * 5 * 8, dtype=np.float32).reshape(366, 5, 8), ("dayofyear", "latitude", "longitude"),
                           coords={"dayofyear": minixr.DataArray(np.arange(1, 367), ("dayofyear",))})
    c.run_contrack('z', doy, '>=', 0.5, 2, segments='member', chunk_steps=5)
    call = fake.calls[-1]
    assert call["thr"] is None and fake.field is None
    pos = call["field"][1]
    assert pos.shape == (M * T,) and np.array_equal(pos, np.tile(pos[:T], M))
    n = len(fake.calls)
    with pytest.raises(ValueError, match="member"):                # a numpy threshold field with a member dimension stays refused
        c.run_contrack('z', np.zeros((5, 8)), '>=', 0.5, 2, segments='member', chunk_steps=5)
    assert len(fake.calls) == n


def test_gaps_with_chunk_steps_forwards_the_starts(fake):
    days = djf_days([2000, 2001, 2002])
    lat, lon = grid()
    a = np.random.default_rng(3).standard_normal((len(days), len(lat), len(lon))).astype(np.float32)
    c = cm.contrack(ds=minixr.make_dataset(a, lat, lon, time=days.astype("datetime64[ns]")))
    c.run_contrack('anom', 1.0, '>=', 0.5, 2, segments='gaps', chunk_steps=50)          # (no ValueError any more)
    lens = [len(djf_days([y])) for y in (2000, 2001, 2002)]
    call = fake.calls[-1]
    assert call["segments"].tolist() == [0, lens[0], lens[0] + lens[1]] and call["chunk_steps"] == 50
    assert np.array_equal(call["anom"], a)
    assert 'segments = gaps (3)' in c.ds['flag'].attrs['history']
    c.run_contrack('anom', 1.0, '>=', 0.5, 2, chunk_steps=50)                           # without segments: the call as it was
    assert fake.calls[-1]["segments"] is None


def test_track_numpy_forwards_segments_and_chunk_steps(fake):
    lat, lon = grid()
    a = np.zeros((6, len(lat), len(lon)), dtype=np.float32)
    w = np.ones(len(lat), dtype=np.float32)
    flag, n = cm.track_numpy(a, w, 1.0, '>=', 0.5, 2, segments=np.array([0, 1, 5]), chunk_steps=4)
    call = fake.calls[-1]
    assert call["segments"].tolist() == [0, 1, 5] and call["chunk_steps"] == 4 and call["thr"].shape == (6,)
    cm.track_numpy(a, w, np.zeros((len(lat), len(lon))), '>=', 0.5, 2, segments=[0, 3], chunk_steps=0)
    call = fake.calls[-1]
    assert call["thr"] is None and call["field"] is not None and call["segments"].tolist() == [0, 3] and fake.field is None
    with pytest.raises(ValueError):
        cm.track_numpy(a, w, 1.0, '>=', 0.5, 2, segments=[0, 7], chunk_steps=4)
    cm.track_numpy(a.astype(np.float64), w, 1.0, '>=', 0.5, 2, chunk_steps=4)
    assert fake.calls[-1]["segments"] is None and fake.calls[-1]["anom"].dtype == np.float64


def test_abi_exports_the_segment_entries():
    L = _native.lib()
    for name in ("ctk_track_stream_seg_f32", "ctk_track_stream_seg_f64", "ctk_track_stream_seg_cb", "ctk_track_sharded_seg_f32_dev",
                 "ctk_track_sharded_seg_f64_dev"):
        assert hasattr(L, name) and name in _native.EXPORTS
    st = np.array([0, 1], dtype=np.int64)
    assert L.ctk_track_stream_seg_f32(None, None, 2, 1, 1, None, 0, None, 0.5, 1, 1, None, None, 0, st.ctypes.data, 2) == -1      # null handle
