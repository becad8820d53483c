"""bench.py --dump-outputs without a GPU: dump_outputs() on a host-backed stand-in for the tracker (the flag slab in host memory,
device pointers as offsets into it), read back in several chunks; and the 64 MB bound for every workload of the bench."""
import ctypes as C
import os

import numpy as np
import pytest

import bench

BASE = 1 << 20          # fake device address of the slab's first byte


class HostSlab:
    def __init__(self, flag):
        self.flag = np.ascontiguousarray(flag, dtype=np.int32)

    def d2h(self, arr, src):
        off = (src.value - BASE) // 4
        arr[...] = self.flag.reshape(-1)[off:off + arr.size].reshape(arr.shape)


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


@pytest.mark.parametrize("chunk_px", [7 * 6 * 5, 3 * 6 * 5, 1])
def test_dump_outputs_reads_the_whole_slab(tmp_path, chunk_px):
    T, ny, nx = 7, 6, 5
    wl = dict(T=T, ny=ny, nx=nx)
    flag = np.random.default_rng(3).integers(0, 4, size=(T, ny, nx)).astype(np.int32) * (1 << 29)
    info = bench.dump_outputs(HostSlab(flag), C.c_void_p(BASE), wl, 11, str(tmp_path), chunk_px=chunk_px)
    got = _load(tmp_path)
    assert sorted(info["files"]) == sorted(n + ".npy" for n in got)
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["n_tracked"].tolist() == [11.0]
    assert np.array_equal(got["flag_per_step"][:, 0], np.count_nonzero(flag, axis=(1, 2)))
    assert np.array_equal(got["flag_per_step"][:, 1], flag.sum(axis=(1, 2), dtype=np.int64))
    t = got["flag_sample_t"].astype(np.int64)
    assert np.array_equal(t, np.arange(T))                          # a small slab fits the sample whole
    assert np.array_equal(got["flag_sample"], flag[t])


def test_dump_outputs_sample_is_fixed(tmp_path):
    T, ny, nx = 400, 181, 360                                       # more timesteps than the sample holds
    wl = dict(T=T, ny=ny, nx=nx)
    flag = np.zeros((T, ny, nx), dtype=np.int32)
    flag[:, 0, 0] = np.arange(T)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(HostSlab(flag), C.c_void_p(BASE), wl, 0, str(a))
    bench.dump_outputs(HostSlab(flag), C.c_void_p(BASE), wl, 0, str(b), chunk_px=ny * nx * 3)
    ga, gb = _load(a), _load(b)
    assert all(np.array_equal(ga[k], gb[k]) for k in ga)
    t = ga["flag_sample_t"]
    assert 1 <= len(t) < T and np.all(np.diff(t) > 0)
    assert np.array_equal(ga["flag_sample"][:, 0, 0], t)


@pytest.mark.parametrize("name", sorted(bench.WORKLOADS))
def test_dump_outputs_stay_below_64_mb(name):
    wl = bench.WORKLOADS[name]
    T, px = wl["T"], wl["ny"] * wl["nx"]
    k = min(T, max(1, bench.DUMP_SAMPLE_BYTES // (px * 8)))
    assert 8 * (1 + 2 * T + k * px + k) <= 64 << 20
