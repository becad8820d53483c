"""calc_anom on a host slab, four ways in one process (profiles/NOTES.md): ms per call, best and median of `reps` after a warm-up, host
clock around calls that end in a synchronisation.
  (a) Tracker.anomalies                      -- ctk_anom_*: k_anom reads x, group and clim `smooth` times per output
  (b) Tracker.anomalies(segments=[0])        -- ctk_anom_seg_*: the same host path with the LDS ring form, same bits
      both with the climatology handed in and the result left resident: the upload of the slab and the anomaly kernel, nothing else;
      h2d = the upload alone (a plain copy of the pageable slab into device memory), so a - h2d and b - h2d are the kernels
  (c) Tracker.anomalies_stream from the host array, no climatology given: the slab in twice, the anomalies out once, in chunks
  (d) plain copies of the same bytes between pinned (registered) host memory and the device: two slabs in, one out -- the floor of (c)
One JSON line per smoothing (1, the default; 2; 16).  Daily steps from 1981-01-01, groups = day of year, window 31, float32.
Usage: python tools/anom_probe.py [T ny nx [reps]]      (default: 2707 181 360 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native

argv = sys.argv[1:]
T, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5
W = 31
stamps = np.datetime64("1981-01-01") + np.arange(T)
group = (stamps - stamps.astype("datetime64[Y]")).astype(np.int32)          # 0 .. 365
G = int(group.max()) + 1
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
    return dict(best=round(min(ms), 2), median=round(float(np.median(ms)), 2), worst=round(max(ms), 2))


with _native.Tracker(0) as trk:
    L = _native.lib()
    out = np.empty_like(x)
    d = trk.malloc(x.nbytes)
    try:
        _, clim = trk.anomalies(x, group, G, window=W, smooth=1, want_anom=False, want_clim=True)
        for buf in (x, out):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor():
            trk.h2d(d, x)
            trk.h2d(d, x)
            trk.d2h(out, d)
        ms_floor = timed(floor)
        for buf in (x, out):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
        ms_h2d = timed(lambda: trk.h2d(d, x))                                     # (pageable again, as (a) and (b) take it)
        for smooth in (1, 2, 16):
            a = trk.anomalies(x, group, G, window=W, smooth=smooth, clim=clim)[0]
            b = trk.anomalies(x, group, G, window=W, smooth=smooth, clim=clim, segments=[0])[0]
            form = trk.debug_anom_form()
            c = trk.anomalies_stream(x, group, G, window=W, smooth=smooth, sink=out)[0]
            same = bool(np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True))
            del a, b, c
            res = dict(shape=[T, ny, nx], groups=G, window=W, smooth=smooth, reps=reps, form="ring" if form == 1 else "plain", identical=same,
                       a_anomalies=timed(lambda: trk.anomalies(x, group, G, window=W, smooth=smooth, clim=clim, want_anom=False, keep_resident=True)),
                       b_segments=timed(lambda: trk.anomalies(x, group, G, window=W, smooth=smooth, clim=clim, want_anom=False, keep_resident=True, segments=[0])),
                       a_again=timed(lambda: trk.anomalies(x, group, G, window=W, smooth=smooth, clim=clim, want_anom=False, keep_resident=True)),
                       h2d=ms_h2d, c_stream=timed(lambda: trk.anomalies_stream(x, group, G, window=W, smooth=smooth, sink=out)), d_pinned_copies=ms_floor)
            print(json.dumps(res), flush=True)
    finally:
        trk.free(d)
