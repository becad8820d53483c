"""The composite over flagged time steps, measured in one process on one device (profiles/NOTES.md).  The flags are those of a tracked
`synth` slab (threshold 160 '>=', overlap 0.5, persistence 5), the field is the slab itself, float32; groups: none, 'season' (4 ids in
runs of a quarter of a 360-step year, DJF wrapping) and 'dayofyear' (365 ids, a new one at every step).  Best of `reps`.
  (a) k_composite alone between HIP events (Tracker.time_composite), against plain 16-byte load streams over the same two buffers
      (Tracker.stream_ceiling) -- with the bytes the kernel has to ask for at most (flags + field) and the flagged fraction
  (b) Tracker.composite on host arrays at the default chunk (about 256 MB of field), host clock; against plain copies of the same
      bytes from pinned (registered) host memory in the same chunks -- the floor -- and against Tracker.lifecycle_stream on the same
      two slabs, which moves them through the same pipeline
  (c) the same call with the field resident (Tracker.anomalies(keep_resident=True) of the slab): only the flags travel
One JSON line per shape.  Usage: python tools/composite_probe.py [T ny nx [reps]]      (default: 2707 181 360, then 480 721 1440; 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native, synth                                         # noqa: E402
from contrack_amd.contrack import row_weights                                   # noqa: E402

argv = sys.argv[1:]
shapes = [tuple(int(v) for v in argv[:3])] if len(argv) >= 3 else [(2707, 181, 360), (480, 721, 1440)]
reps = int(argv[3]) if len(argv) >= 4 else 5


def timed(fn):
    fn()                                                                       # warm-up: code objects, allocations, pinned buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(min(ms), 2)


def groupings(T):
    step = np.arange(T)
    yield "none", None, 1
    yield "season", ((step % 360 + 30) // 90 % 4).astype(np.int32), 4
    yield "dayofyear", (step % 365).astype(np.int32), 365


def probe(trk, T, ny, nx):
    L = _native.lib()
    lat, lon = synth.grid(ny, nx)
    wrow = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    nb = T * ny * nx * 4
    d_in, d_flag = trk.malloc(nb), trk.malloc(nb)
    d_sum, d_n = trk.malloc(365 * ny * nx * 8), trk.malloc(365 * ny * nx * 4)
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, wrow, 0.5, 5, True, d_flag)
        field, flag = np.empty((T, ny, nx), dtype=np.float32), np.empty((T, ny, nx), dtype=np.int32)
        trk.d2h(field, d_in)
        trk.d2h(flag, d_flag)
        plan = _native.composite_plan(4, ny * nx)
        res = dict(shape=[T, ny, nx], reps=reps, n_tracked=n_tracked, flagged_fraction=round(float(np.mean(flag > 0)), 5), plan=plan,
                   gb_two_slabs=round(2 * nb / 1e9, 3))
        # (a) the kernel alone
        loads = trk.stream_ceiling(d_flag, nb, 0, reps) + trk.stream_ceiling(d_in, nb, 0, reps)
        res["a_plain_load_streams_ms"] = round(loads, 3)
        for name, ids, G in groupings(T):
            best, _ = trk.time_composite(d_flag, d_in, T, ny, nx, d_sum, d_n, group=ids, ngroups=G, reps=reps)
            res["a_kernel_ms_" + name] = round(best, 3)
            res["a_ratio_to_loads_" + name] = round(best / loads, 3)
            res["a_gbps_of_two_slabs_" + name] = round(2 * nb / best / 1e6, 1)
        # (b) host arrays, streamed
        chunk = max(1, min(T, (256 << 20) // (ny * nx * 4)))
        res["chunk_steps"] = chunk
        for name, ids, G in groupings(T):
            res["b_composite_ms_" + name] = timed(lambda: trk.composite(flag, field, ids, G))
        res["b_stream_times"] = {k: round(v, 2) for k, v in trk.stream_times().items()}
        res["b_lifecycle_stream_ms"] = timed(lambda: trk.lifecycle_stream(flag, field, wrow))
        for buf in (flag, field):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor():
            for t0 in range(0, T, chunk):
                trk.h2d(d_flag, flag[t0:t0 + chunk])
                trk.h2d(d_in, field[t0:t0 + chunk])
        res["b_pinned_copies_ms"] = timed(floor)
        for buf in (flag, field):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
        res["b_composite_over_copies"] = round(res["b_composite_ms_none"] / res["b_pinned_copies_ms"], 3)
        res["b_lifecycle_over_copies"] = round(res["b_lifecycle_stream_ms"] / res["b_pinned_copies_ms"], 3)
        # (c) the field resident: the anomaly of the slab against a one-group climatology stays in HBM
        anom, _ = trk.anomalies(field, np.zeros(T, np.int32), 1, keep_resident=True)
        s_res, n_res = trk.composite(flag, None, None, 1)
        s_two, n_two = trk.composite(flag, anom, None, 1)
        res["c_identical"] = bool(np.array_equal(n_res, n_two) and np.array_equal(s_res.view(np.uint64), s_two.view(np.uint64)))
        res["c_resident_ms"] = timed(lambda: trk.composite(flag, None, None, 1))
        res["c_two_slabs_ms"] = timed(lambda: trk.composite(flag, anom, None, 1))
        print(json.dumps(res), flush=True)
    finally:
        for p in (d_in, d_flag, d_sum, d_n):
            trk.free(p)


with _native.Tracker(0) as trk:
    for shape in shapes:
        probe(trk, *shape)
