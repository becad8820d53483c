"""Threshold fields on the Python side, without a GPU: what track_numpy and the class hand to the tracker for a threshold that
varies by grid point -- numpy broadcasting against the variable, the transpose by name of a DataArray over ('dayofyear', lat, lon),
the alignment of its spatial labels with the dataset's, and the plane of every step.  The tracker is a recording stand-in."""
import importlib

import numpy as np
import pytest

import minixr

cm = importlib.import_module("contrack_amd.contrack")       # (the package attribute `contrack` is the class)

minixr.install_as_xarray()          # only when the real package is absent


class FakeTracker:
    """records what the class / track_numpy pass; returns an all-zero flag"""

    def __init__(self):
        self.field = None
        self.calls = []

    def set_threshold_field(self, field, plane_of_step):
        self.field = (np.array(field), np.array(plane_of_step))

    def clear_threshold_field(self):
        self.calls.append(("clear",))

    def _ret(self, kind, shape, thr):
        self.calls.append((kind, None if thr is None else np.array(thr), self.field))
        return np.zeros(shape, dtype=np.int32), 0

    def track(self, anom, thr, *a, **k):
        return self._ret("track", anom.shape, thr)

    def track_stream(self, source, thr, *a, shape=None, **k):
        out = np.empty(shape, dtype=np.float32 if k.get("dtype") == np.float32 else np.float64)
        source(0, shape[0], out)
        return self._ret("stream", shape, thr)

    def stats(self):
        return {}

    def release_io(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    f = FakeTracker()
    monkeypatch.setattr(cm, "_tracker", lambda device=None: f)
    return f


def _wrow(ny):
    return np.ones(ny, dtype=np.float32)


@pytest.mark.parametrize("shape, planes", [((5, 7), 1), ((1, 5, 7), 1), ((5, 1), 1), ((1, 7), 1), ((4, 5, 7), 4), ((4, 5, 1), 4)])
def test_track_numpy_broadcasts_a_field_as_numpy_does(fake, shape, planes):
    T, ny, nx = 4, 5, 7
    rng = np.random.default_rng(1)
    anom = rng.standard_normal((T, ny, nx)).astype(np.float32)
    thr = rng.standard_normal(shape)
    cm.track_numpy(anom, _wrow(ny), thr, ">=", 0.5, 1)
    kind, passed_thr, (field, pos) = fake.calls[0]
    assert kind == "track" and passed_thr is None and fake.calls[-1] == ("clear",)
    assert field.shape == (planes, ny, nx) and field.dtype == thr.dtype
    want = np.broadcast_to(thr, (T, ny, nx))
    assert np.array_equal(field[pos], want)
    assert pos.shape == (T,) and (planes > 1 or not pos.any())


@pytest.mark.parametrize("thr", [0.5, np.float64(0.5), np.full(4, 0.25), np.full((4, 1, 1), 0.25), np.float32(0.5)])
def test_track_numpy_keeps_the_per_step_path(fake, thr):
    anom = np.zeros((4, 5, 7), dtype=np.float32)
    cm.track_numpy(anom, _wrow(5), thr, ">=", 0.5, 1)
    assert len(fake.calls) == 1
    kind, passed_thr, field = fake.calls[0]
    assert kind == "track" and field is None and passed_thr.shape == (4,)


def test_track_numpy_refuses_a_field_that_does_not_broadcast(fake):
    anom = np.zeros((4, 5, 7), dtype=np.float32)
    for bad in (np.zeros((5, 6)), np.zeros((3, 5, 7)), np.zeros((2, 4, 5, 7)), np.zeros((1, 1, 5, 7))):
        with pytest.raises(ValueError):
            cm.track_numpy(anom, _wrow(5), bad, ">=", 0.5, 1)
    assert fake.calls == []


def _ds(T=40, ny=6, nx=8, dims=("time", "latitude", "longitude"), t0="2001-12-10"):
    rng = np.random.default_rng(2)
    a = rng.standard_normal((T, ny, nx)).astype(np.float32)
    lat = np.linspace(75.0, 30.0, ny).astype(np.float32)
    lon = (np.arange(nx) * 45.0).astype(np.float32)
    time = (np.datetime64(t0) + np.arange(T)).astype("datetime64[ns]")
    ds = minixr.make_dataset(a, lat, lon, time=time)
    ds["time"].attrs = {}
    if dims != ("time", "latitude", "longitude"):
        order = [("time", "latitude", "longitude").index(d) for d in dims]
        ds["anom"] = minixr.DataArray(a.transpose(order), dims, attrs={"units": "m", "long_name": "Z500 anomaly"})
    c = cm.contrack(ds=ds)
    c.set_up(time_name="time", longitude_name="longitude", latitude_name="latitude")
    doy = np.asarray(__import__("pandas").DatetimeIndex(time).dayofyear)
    return c, a, lat, lon, doy


def _doy_threshold(lat, lon, dims=("longitude", "dayofyear", "latitude"), reverse_lat=True, doys=np.arange(1, 367), dtype=np.float64):
    rng = np.random.default_rng(3)
    tll = rng.standard_normal((len(doys), len(lat), len(lon))).astype(dtype)       # (dayofyear, lat, lon) in the dataset's lat order
    lat_c = lat[::-1] if reverse_lat else lat
    data = tll[:, ::-1] if reverse_lat else tll
    order = [("dayofyear", "latitude", "longitude").index(d) for d in dims]
    coords = {"dayofyear": minixr.DataArray(doys, ("dayofyear",)), "latitude": minixr.DataArray(lat_c, ("latitude",)),
              "longitude": minixr.DataArray(lon, ("longitude",))}
    return minixr.DataArray(np.ascontiguousarray(data.transpose(order)), dims, coords=coords), tll


@pytest.mark.parametrize("chunk", [None, 7])
def test_class_dayofyear_field_transposed_by_name_and_lat_aligned(fake, chunk):
    c, a, lat, lon, doy = _ds()
    thr, tll = _doy_threshold(lat, lon)
    c.run_contrack(variable="anom", threshold=thr, gorl=">=", overlap=0.5, persistence=1, chunk_steps=chunk)
    kind, passed_thr, (field, pos) = fake.calls[0]
    assert kind == ("track" if chunk is None else "stream") and passed_thr is None and fake.calls[-1] == ("clear",)
    assert field.shape == (366, len(lat), len(lon))
    assert np.array_equal(pos, doy - 1)
    assert np.array_equal(field[pos], tll[doy - 1])                  # every step against the plane of its day of year
    assert np.asarray(c.flag).shape == a.shape


def test_class_dayofyear_field_with_a_missing_spatial_dim_broadcasts(fake):
    c, a, lat, lon, doy = _ds()
    doys = np.arange(1, 367)
    vals = np.random.default_rng(4).standard_normal((len(lat), 366))
    thr = minixr.DataArray(vals, ("latitude", "dayofyear"), coords={"dayofyear": minixr.DataArray(doys, ("dayofyear",)),
                                                                    "latitude": minixr.DataArray(lat, ("latitude",))})
    c.run_contrack(variable="anom", threshold=thr, gorl=">", overlap=0.5, persistence=1)
    _, _, (field, pos) = fake.calls[0]
    assert np.array_equal(field[pos], np.broadcast_to(vals.T[doy - 1][:, :, None], a.shape))


def test_class_dayofyear_field_errors(fake):
    c, a, lat, lon, doy = _ds()
    thr, _ = _doy_threshold(lat, lon, doys=np.arange(1, 300))                 # December steps are missing
    with pytest.raises(KeyError):
        c.run_contrack(variable="anom", threshold=thr, gorl=">=", overlap=0.5, persistence=1)
    thr, _ = _doy_threshold(lat + np.float32(0.5), lon)                         # other latitudes
    with pytest.raises(ValueError):
        c.run_contrack(variable="anom", threshold=thr, gorl=">=", overlap=0.5, persistence=1)
    thr, _ = _doy_threshold(lat, lon[:-1])                                      # fewer longitudes
    with pytest.raises(ValueError):
        c.run_contrack(variable="anom", threshold=thr, gorl=">=", overlap=0.5, persistence=1)
    no_doy = minixr.DataArray(np.zeros((len(lat), len(lon))), ("latitude", "longitude"))
    with pytest.raises(ValueError):
        c.run_contrack(variable="anom", threshold=no_doy, gorl=">=", overlap=0.5, persistence=1)
    extra = minixr.DataArray(np.zeros((2, 366, len(lat), len(lon))), ("member", "dayofyear", "latitude", "longitude"))
    with pytest.raises(ValueError):
        c.run_contrack(variable="anom", threshold=extra, gorl=">=", overlap=0.5, persistence=1)
    assert [k for k in fake.calls if k[0] != "clear"] == []


def test_class_numpy_field_broadcasts_in_the_variables_dim_order(fake):
    dims = ("latitude", "time", "longitude")
    c, a, lat, lon, doy = _ds(dims=dims)
    T, ny, nx = a.shape
    f = np.random.default_rng(5).standard_normal((ny, 1, nx)).astype(np.float32)      # (lat, 1, lon): one plane for every step
    c.run_contrack(variable="anom", threshold=f, gorl="<", overlap=0.5, persistence=1)
    _, passed_thr, (field, pos) = fake.calls[0]
    assert passed_thr is None and field.shape == (1, ny, nx) and not pos.any()
    assert np.array_equal(field[0], f[:, 0, :])
    full = np.random.default_rng(6).standard_normal((ny, T, nx))                        # the variable's own shape: one plane per step
    c.run_contrack(variable="anom", threshold=full, gorl="<", overlap=0.5, persistence=1)
    _, _, (field, pos) = fake.calls[2]
    assert np.array_equal(field[pos], full.transpose(1, 0, 2))


def test_class_scalar_and_1d_dayofyear_paths_unchanged(fake):
    c, a, lat, lon, doy = _ds()
    c.run_contrack(variable="anom", threshold=0.5, gorl=">=", overlap=0.5, persistence=1)
    thr1 = minixr.DataArray(np.linspace(0, 1, 366), ("dayofyear",), coords={"dayofyear": minixr.DataArray(np.arange(1, 367), ("dayofyear",))})
    c.run_contrack(variable="anom", threshold=thr1, gorl=">=", overlap=0.5, persistence=1)
    assert [k[0] for k in fake.calls] == ["track", "track"]
    assert fake.calls[0][2] is None and fake.calls[1][2] is None
    assert np.array_equal(fake.calls[1][1], np.linspace(0, 1, 366)[doy - 1])
