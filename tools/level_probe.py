"""The vertical mean (ctk_level_mean_*), four measurements in one process (profiles/NOTES.md), best of `reps` after a warm-up; one JSON
line each.
  1 kernel:   k_level_mean alone (HIP events) on a float32 (steps, 8, ny, nx) field in device memory, all 8 levels selected, against the
              plain 16-byte load stream over the same buffer (ctk_debug_stream_ceiling mode 0) charged (K + 1) / K of its time for
              the store: fraction = stream * (K + 1) / K / kernel
  2 stream:   the streamed host-array call (pageable array in, array out) against plain copies of the same bytes in the same chunks
              between pinned (registered) host memory and the device, one after the other
  3 subset:   nlev = 37 with 10 selected against nlev = 10 with 10 selected, same steps and grid: unselected levels do not cross PCIe
  4 chain:    level_mean(keep_resident) + anomalies_resident against level_mean to the host + anomalies from the host (segments=[0]:
              the same anomaly kernel), anomalies to the host in both
Usage: python tools/level_probe.py [steps ny nx [reps]]      (default: 2707 181 360 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native

argv = sys.argv[1:]
steps, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5
K = 8
rng = np.random.default_rng(1)


def random_field(shape):
    x = np.empty(shape, dtype=np.float32)
    for t0 in range(0, shape[0], 16):
        x[t0:t0 + 16] = rng.standard_normal(x[t0:t0 + 16].shape, dtype=np.float32)
    return x


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
    x = random_field((steps, K, ny, nx))
    w = np.array([12.5, 25, 25, 25, 37.5, 50, 50, 25], dtype=np.float64)
    plane = ny * nx * 4
    out = np.empty((steps, ny, nx), dtype=np.float32)
    d_x, d_o = trk.malloc(x.nbytes), trk.malloc(out.nbytes)
    try:
        # ---- 1 ---------------------------------------------------------------------------------------------------------------
        trk.h2d(d_x, x)
        k_best, k_mean = trk.time_level_mean(d_x, steps, K, ny, nx, w, d_o, reps=reps)       # one untimed launch + reps timed ones, as the stream
        s_best = trk.stream_ceiling(d_x, x.nbytes, write=False, reps=reps)
        by_xcd = {}                                               # (beside the comparison: not part of the fraction)
        for mode in (0, 1, 256):                                  # workgroups to XCDs: launch order, eighths (the rule here), tiles of 256
            trk.debug_set_level(mode)
            by_xcd[str(mode)] = round(trk.time_level_mean(d_x, steps, K, ny, nx, w, d_o, reps=reps)[0], 3)
        trk.debug_set_level()
        charged = s_best * (K + 1) / K
        print(json.dumps(dict(measurement="1 kernel", shape=[steps, K, ny, nx], gb_in=round(x.nbytes / 1e9, 2), form=trk.debug_level_form(),
                              unroll=_native.level_plan(4, K, ny * nx, steps)["unroll"], xcd=_native.level_plan(4, K, ny * nx, steps)["xcd"], kernel_ms_by_xcd_mode=by_xcd, kernel_ms=round(k_best, 3), kernel_mean_ms=round(k_mean, 3),
                              load_stream_ms=round(s_best, 3), stream_charged_ms=round(charged, 3),
                              fraction=round(charged / k_best, 3), tb_per_s_in=round(x.nbytes / k_best / 1e9, 2))), flush=True)
        # ---- 2 ---------------------------------------------------------------------------------------------------------------
        chunk = max(1, (256 << 20) // (K * plane))
        for buf in (x, out):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor():
            for c0 in range(0, steps, chunk):
                trk.h2d(d_x, x[c0:c0 + chunk])
                trk.d2h(out[c0:c0 + chunk], d_o)
        ms_floor = timed(floor)
        for buf in (x, out):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))

        def stream():
            _native.check(L.ctk_level_mean_stream_f32(trk.handle, x.ctypes.data, steps, K, ny, nx, w.ctypes.data, 0, out.ctypes.data, 0, 0))
        ms_stream = timed(stream)
        print(json.dumps(dict(measurement="2 stream", shape=[steps, K, ny, nx], chunk_steps=chunk, streamed=ms_stream, pinned_copies=ms_floor,
                              above_floor=round(ms_stream["best"] / ms_floor["best"] - 1, 3), stream_ms={k: round(v, 1) for k, v in trk.stream_times().items()})), flush=True)
        # ---- 4 (the same field) ----------------------------------------------------------------------------------------------
        stamps = np.datetime64("1981-01-01") + np.arange(steps)
        group = (stamps - stamps.astype("datetime64[Y]")).astype(np.int32)
        G, W, S = int(group.max()) + 1, 31, 2

        def chain():
            trk.level_mean(x, w, keep_resident=True, want_out=False)
            return trk.anomalies_resident(group, G, window=W, smooth=S)[0]

        def round_trip():
            return trk.anomalies(trk.level_mean(x, w), group, G, window=W, smooth=S, segments=[0])[0]
        same = bool(np.array_equal(chain(), round_trip(), equal_nan=True))
        ms_chain, ms_trip = timed(chain), timed(round_trip)
        ms_h2d, ms_d2h = timed(lambda: trk.h2d(d_o, out)), timed(lambda: trk.d2h(out, d_o))           # the slab, pageable, one way each
        print(json.dumps(dict(measurement="4 chain", shape=[steps, K, ny, nx], identical=same, resident_chain=ms_chain, host_round_trip=ms_trip,
                              difference_ms=round(ms_trip["best"] - ms_chain["best"], 2), slab_h2d=ms_h2d, slab_d2h=ms_d2h)), flush=True)
    finally:
        trk.free(d_x)
        trk.free(d_o)
    del x, out
    # ---- 3 -------------------------------------------------------------------------------------------------------------------
    s3 = max(1, min(steps, 256))
    wide, w37 = random_field((s3, 37, ny, nx)), np.zeros(37)
    w37[14:24] = 1.0
    narrow = np.ascontiguousarray(wide[:, 14:24])
    a, b = trk.level_mean(wide, w37), trk.level_mean(narrow, np.ones(10))
    ms37, ms10 = timed(lambda: trk.level_mean(wide, w37)), timed(lambda: trk.level_mean(narrow, np.ones(10)))
    ms37b = timed(lambda: trk.level_mean(wide, w37))
    print(json.dumps(dict(measurement="3 subset", steps=s3, grid=[ny, nx], identical=bool(np.array_equal(a, b, equal_nan=True)), nlev37_sel10=ms37, nlev10_sel10=ms10,
                          nlev37_again=ms37b, ratio=round(min(ms37["best"], ms37b["best"]) / ms10["best"], 3))), flush=True)
