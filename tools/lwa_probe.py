"""The local wave activity (ctk_lwa_*), three measurements in one process (profiles/NOTES.md), float32, both hemispheres, the default
lat_bounds, best of `reps` after a warm-up; one JSON line each, every figure beside a yardstick taken in the same process.
  1 stages:   k_lwa_contour and k_lwa_integral each alone (HIP events, the memset before each included) on a (steps, ny, nx) field in
              device memory, against a plain copy kernel (one 16-byte load and one 16-byte store per lane) over the same two buffers
  2 host:     the host-array call (pageable array in, array out) against plain copies of the bytes that travel (the rows the domains
              span in, the rows the active rows span out) in the same chunks between pinned (registered) host memory and the device
  3 chain:    lwa(keep_resident) + track_resident against lwa + track of the host result (the 90th percentile of the field, '>')
Usage: python tools/lwa_probe.py [steps ny nx [reps]]      (default: 2707 181 360 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native
from contrack_amd.contrack import lwa_rows, row_weights

argv = sys.argv[1:]
steps, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5
rng = np.random.default_rng(1)
lat = np.linspace(90.0, -90.0, ny)
res = 180.0 / (ny - 1)


def height():
    """5700 - 800 sin^2(lat) + weather that is smooth along longitude, N(0, 150)"""
    z = np.empty((steps, ny, nx), dtype=np.float32)
    prof = (5700.0 - 800.0 * np.sin(np.deg2rad(lat)) ** 2).astype(np.float32)[None, :, None]
    k = max(1, nx // 24)
    for t0 in range(0, steps, 16):
        n = rng.standard_normal(z[t0:t0 + 16].shape, dtype=np.float32)
        c = np.cumsum(n, axis=2)
        n = (np.roll(c, -k, axis=2) - c) / np.float32(np.sqrt(k))               # a box of k columns (the wrap-around column aside)
        n[:, :, -k:] = n[:, :, :k]
        z[t0:t0 + 16] = prof + np.float32(150.0) * n
    return z


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
    z = height()
    out = np.empty_like(z)
    row, plane = nx * 4, ny * nx * 4
    tab = lwa_rows(lat)
    act = np.flatnonzero(tab["active"])
    r0, r1, a0, a1 = int(tab["dom_rows"].min()), int(tab["dom_rows"].max()) + 1, int(act.min()), int(act.max()) + 1
    longest = int(np.diff(tab["dom_off"]).max())
    d_x, d_o = trk.malloc(z.nbytes), trk.malloc(z.nbytes)
    try:
        # ---- 1 ---------------------------------------------------------------------------------------------------------------
        trk.h2d(d_x, z)
        copy_ms = round(trk.time_lwa(d_x, steps, ny, nx, None, d_o, 0, reps=reps)[0], 3)
        for part in ("total", "anticyclonic"):
            sel = trk.time_lwa(d_x, steps, ny, nx, tab, d_o, 1, part=part, reps=reps)
            integ = trk.time_lwa(d_x, steps, ny, nx, tab, d_o, 2, part=part, reps=reps)
            trk.d2h(out[:1], d_o)
            band = out[0][tab["active"] != 0]
            print(json.dumps(dict(measurement="1 stages", shape=[steps, ny, nx], part=part, active_rows=int(len(act)), longest_domain=longest,
                                  nonzero_share=round(float(np.count_nonzero(band)) / max(band.size, 1), 3), form=trk.debug_lwa_form(),
                                  plan=_native.lwa_plan(4, longest, nx, 2, steps), contour_ms=round(sel[0], 3), contour_mean_ms=round(sel[1], 3),
                                  integral_ms=round(integ[0], 3), integral_mean_ms=round(integ[1], 3), copy_ms=copy_ms,
                                  contour_over_copy=round(sel[0] / copy_ms, 2), integral_over_copy=round(integ[0] / copy_ms, 2))), flush=True)
        # ---- 2 ---------------------------------------------------------------------------------------------------------------
        chunk = max(1, min(steps, (256 << 20) // plane))
        args, _keep = _native._lwa_rows(tab, ny)
        flat_in, flat_out = z.reshape(-1), out.reshape(-1)
        for buf in (z, out):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor():
            for c0 in range(0, steps, chunk):
                nt = min(chunk, steps - c0)
                trk.h2d(d_x, flat_in[:nt * (r1 - r0) * nx])
                trk.d2h(flat_out[:nt * (a1 - a0) * nx], d_o)

        def upload():
            for c0 in range(0, steps, chunk):
                trk.h2d(d_x, flat_in[:min(chunk, steps - c0) * (r1 - r0) * nx])
        ms_floor, ms_up = timed(floor), timed(upload)
        for buf in (z, out):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))

        def call():
            _native.check(L.ctk_lwa_f32(trk.handle, z.ctypes.data, steps, ny, nx, *args, 0, out.ctypes.data, None, 0, 0))
        ms_call = timed(call)
        print(json.dumps(dict(measurement="2 host", shape=[steps, ny, nx], chunk_steps=chunk, rows_in=[r0, r1], rows_out=[a0, a1],
                              mb_in=round(steps * (r1 - r0) * row / 1e6, 1), mb_out=round(steps * (a1 - a0) * row / 1e6, 1), call=ms_call,
                              pinned_copies=ms_floor, pinned_upload_alone=ms_up, ratio=round(ms_call["best"] / ms_floor["best"], 3),
                              stream_ms={k: round(v, 1) for k, v in trk.stream_times().items()})), flush=True)
    finally:
        trk.free(d_x)
        trk.free(d_o)
    # ---- 3 -------------------------------------------------------------------------------------------------------------------
    wrow = row_weights(lat.astype(np.float32), np.float32(res), np.float32(360.0 / nx))
    host = trk.lwa(z, tab, part=1)
    level = float(np.percentile(host[::max(1, steps // 64)][:, tab["active"] != 0], 90))
    thr = np.full(steps, level)
    op = _native.CMP_OPS[">"]

    def chain():
        trk.lwa(z, tab, part=1, keep_resident=True, want_out=False)
        return trk.track_resident(thr, op, wrow, 0.0, 1)

    def round_trip():
        return trk.track(trk.lwa(z, tab, part=1), thr, op, wrow, 0.0, 1)
    fa, na = chain()
    fa = np.array(fa)                                                          # (the tracker hands out pooled result arrays)
    fb, nb = round_trip()
    same = bool(na == nb and np.array_equal(fa, fb))
    ms_chain, ms_trip = timed(chain), timed(round_trip)
    print(json.dumps(dict(measurement="3 chain", shape=[steps, ny, nx], identical=same, tracked=int(na), threshold=round(level, 1), resident_chain=ms_chain,
                          host_round_trip=ms_trip, difference_ms=round(ms_trip["best"] - ms_chain["best"], 2))), flush=True)
