"""The time filter beside its yardsticks in one process (profiles/NOTES.md): ms, best of `reps` after a warm-up.
Per configuration, on a float32 slab in device memory:
  kernel      the filter kernel alone between HIP events (ctk_debug_time_filter)
  call        Tracker.time_filter_dev on the host clock: the upload of the tap table, the kernel, the synchronisation
  copy        (a) the plain 16-byte copy kernel over the same two buffers, as many bytes as the filter reads (HIP events)
Per slab:
  anom_K      (b) Tracker.anomalies_resident(segments=[0]) at smooth = K for K = 2 and 16, one group, the climatology handed in, the
              result left resident, host clock: k_anom_ring on the same slab (x resident as the level mean, so nothing is uploaded but
              one plane of climatology and T group ids)
Configurations: box K = 2 and K = 16 at stride 1 (the windows of (b)), box K = 4 at stride 4 (daily means of 6-hourly steps), Lanczos
low-pass K = 21, 61, 121 at stride 1, K = 61 with the plain form forced.
With `stream` the host-array entry (Tracker.time_filter, chunks of about 256 MB) beside plain copies of the same bytes between
registered host memory and the device: one slab in, the result out.
One JSON line per configuration.
Usage: python tools/filter_probe.py [T ny nx [reps [stream]]]      (default: 2707 181 360 5 stream)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native
from contrack_amd.contrack import lanczos_weights

argv = sys.argv[1:]
T, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5
stream = (argv[4] if len(argv) >= 5 else "stream") == "stream"
rng = np.random.default_rng(1)
x = np.empty((T, ny, nx), dtype=np.float32)
for t0 in range(0, T, 64):
    x[t0:t0 + 64] = 50.0 * rng.standard_normal(x[t0:t0 + 64].shape, dtype=np.float32) + 5500.0


def timed(fn):
    fn()                                                                       # warm-up: code objects, allocations, pinned buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(best=round(min(ms), 3), median=round(float(np.median(ms)), 3), worst=round(max(ms), 3))


CONFIGS = [("box2", 2, 1, -1), ("box16", 16, 1, -1), ("daily_box4_stride4", 4, 4, -1), ("lanczos21", lanczos_weights(21, 0.1), 1, -1),
           ("lanczos61", lanczos_weights(61, 1 / 30.0), 1, -1), ("lanczos121", lanczos_weights(121, 1 / 60.0), 1, -1),
           ("lanczos61_plain", lanczos_weights(61, 1 / 30.0), 1, 0)]

with _native.Tracker(0) as trk:
    L = _native.lib()
    d_x, d_out = trk.malloc(x.nbytes), trk.malloc(x.nbytes)
    try:
        trk.h2d(d_x, x)
        # (b) the existing ring kernel on the same slab
        trk.level_mean(x[:, None], [1.0], keep_resident=True, want_out=False)
        group = np.zeros(T, dtype=np.int32)
        clim = np.full((1, ny, nx), 5500.0, dtype=np.float32)
        anom = {}
        for K in (2, 16):
            anom[K] = timed(lambda: trk.anomalies_resident(group, 1, smooth=K, clim=clim, segments=[0], keep_resident=True, want_anom=False))
            assert trk.debug_anom_form() == 1
        for name, weights, stride, forced in CONFIGS:
            K = weights if np.ndim(weights) == 0 else len(weights)
            trk.debug_set_filter(0, 0, forced)
            kw = dict(stride=stride)
            T_out = trk.time_filter_dev(d_x, T, ny, nx, weights, d_out, **kw)
            launch = trk.debug_filter_launch()
            read_bytes = x.nbytes
            res = dict(config=name, shape=[T, ny, nx], K=int(K), stride=stride, T_out=T_out, reps=reps, form="ring" if launch["form"] == 1 else "plain",
                       threads=launch["threads"], tile=launch["tile"], lds=launch["lds"],
                       kernel=[round(v, 3) for v in trk.time_filter_kernel(d_x, T, ny, nx, weights, d_out, reps=reps, **kw)],
                       call=timed(lambda: trk.time_filter_dev(d_x, T, ny, nx, weights, d_out, **kw)),
                       copy=[round(v, 3) for v in trk.time_filter_kernel(d_x, T, ny, nx, weights, d_out, copy_bytes=read_bytes, reps=reps, **kw)])
            if K in anom:
                res["anom_same_K"] = anom[K]
            print(json.dumps(res), flush=True)
        trk.debug_set_filter(0, 0, -1)
        if stream:
            out = np.empty_like(x)
            w = lanczos_weights(21, 0.1)
            res = dict(config="host_array", shape=[T, ny, nx], reps=reps,
                       lanczos21=timed(lambda: trk.time_filter(x, w, chunk_steps=0, out=out)))
            daily = np.empty((len(_native.filter_layout(T, 4, 4)[0]), ny, nx), dtype=np.float32)
            res["daily_box4_stride4"] = timed(lambda: trk.time_filter(x, 4, stride=4, chunk_steps=0, out=daily))
            for buf in (x, out):
                _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))
            res["lanczos21_registered"] = timed(lambda: trk.time_filter(x, w, chunk_steps=0, out=out))

            def floor():
                trk.h2d(d_x, x)
                trk.d2h(out, d_out)
            res["pinned_copies_in_and_out"] = timed(floor)
            res["pinned_copy_in"] = timed(lambda: trk.h2d(d_x, x))
            for buf in (x, out):
                _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
            print(json.dumps(res), flush=True)
    finally:
        trk.free(d_x)
        trk.free(d_out)
