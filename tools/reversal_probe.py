"""The gradient-reversal index (ctk_reversal_*), three measurements in one process (profiles/NOTES.md), float32, best of `reps` after a
warm-up; one JSON line each, every figure beside a yardstick taken in the same process.
  1 kernel:   k_reversal alone (HIP events) on a (steps, ny, nx) field in device memory -- default parameters with two and with three
              criteria, both hemispheres and the northern one alone, under every workgroup-to-XCD mapping -- against a plain copy
              kernel (one 16-byte load and one 16-byte store per lane) over the same two buffers: fraction = copy / kernel
  2 host:     the host-array call (pageable array in, array out) against plain copies of the bytes that travel (the rows some active
              row reads in, the rows the active rows span out) in the same chunks between pinned (registered) host memory and the
              device, one after the other
  3 chain:    reversal(keep_resident) + track_resident against reversal + track of the host result (threshold 0, '>')
Usage: python tools/reversal_probe.py [steps ny nx [reps]]      (default: 2707 181 360 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native
from contrack_amd.contrack import reversal_limits, reversal_rows, row_weights

argv = sys.argv[1:]
steps, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5
rng = np.random.default_rng(1)
lat = np.linspace(90.0, -90.0, ny)
res = 180.0 / (ny - 1)


def height():
    """5600 - 900 sin^2(lat) + weather that is smooth along longitude, N(0, 150): 10-20 % of the band blocked"""
    z = np.empty((steps, ny, nx), dtype=np.float32)
    prof = (5600.0 - 900.0 * np.sin(np.deg2rad(lat)) ** 2).astype(np.float32)[None, :, None]
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


def table(hemisphere, ghgs2=None):
    return reversal_limits(reversal_rows(lat, 15.0, (30, 75), hemisphere, ghgs2 is not None), 0.0, -10.0, ghgs2)


def ranges(tab):
    act = np.flatnonzero(tab["eq"] >= 0)
    read = np.concatenate([act, tab["eq"][act], tab["po"][act]] + ([tab["eq2"][act]] if tab["eq2"] is not None else []))
    return int(read.min()), int(read.max()) + 1, int(act.min()), int(act.max()) + 1


with _native.Tracker(0) as trk:
    L = _native.lib()
    z = height()
    out = np.empty_like(z)
    row, plane = nx * 4, ny * nx * 4
    d_x, d_o = trk.malloc(z.nbytes), trk.malloc(z.nbytes)
    try:
        # ---- 1 ---------------------------------------------------------------------------------------------------------------
        trk.h2d(d_x, z)
        copy_ms = {}
        for mode in (0, 1):
            trk.debug_set_reversal(mode)
            copy_ms[str(mode)] = round(trk.time_reversal(d_x, steps, ny, nx, None, d_o, reps=reps)[0], 3)
        trk.debug_set_reversal()
        copy_best = min(copy_ms.values())
        for hemisphere in ("both", "north"):
            for ghgs2 in (None, -5.0):
                tab = table(hemisphere, ghgs2)
                by_xcd = {}
                for mode in (0, 1, 64):                               # workgroups to XCDs: launch order, eighths (the rule here), tiles of 64
                    trk.debug_set_reversal(mode)
                    by_xcd[str(mode)] = round(trk.time_reversal(d_x, steps, ny, nx, tab, d_o, reps=reps)[0], 3)
                trk.debug_set_reversal()
                k_best, k_mean = trk.time_reversal(d_x, steps, ny, nx, tab, d_o, reps=reps)
                trk.d2h(out[:1], d_o)
                act = tab["eq"] >= 0
                print(json.dumps(dict(measurement="1 kernel", shape=[steps, ny, nx], hemisphere=hemisphere, ghgs2=ghgs2, active_rows=int(act.sum()),
                                      blocked_share=round(float(np.count_nonzero(out[0][act])) / max(out[0][act].size, 1), 3), form=trk.debug_reversal_form(),
                                      plan=_native.reversal_plan(4, ny, nx, steps), kernel_ms_by_xcd_mode=by_xcd, kernel_ms=round(k_best, 3),
                                      kernel_mean_ms=round(k_mean, 3), copy_ms_by_xcd_mode=copy_ms, fraction_of_copy=round(copy_best / k_best, 3),
                                      tb_per_s_in_plus_out=round(2 * z.nbytes / k_best / 1e9, 2))), flush=True)
        # ---- 2 ---------------------------------------------------------------------------------------------------------------
        chunk = max(1, min(steps, (256 << 20) // plane))
        for hemisphere in ("both", "north"):
            tab = table(hemisphere)
            r0, r1, a0, a1 = ranges(tab)
            ptrs, _keep = _native._reversal_rows(tab, ny)
            flat_in, flat_out = z.reshape(-1), out.reshape(-1)
            for buf in (z, out):
                _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

            def floor():
                for c0 in range(0, steps, chunk):
                    nt = min(chunk, steps - c0)
                    trk.h2d(d_x, flat_in[:nt * (r1 - r0) * nx])
                    trk.d2h(flat_out[:nt * (a1 - a0) * nx], d_o)
            ms_floor = timed(floor)
            for buf in (z, out):
                _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))

            def call():
                _native.check(L.ctk_reversal_f32(trk.handle, z.ctypes.data, steps, ny, nx, *ptrs, 0, out.ctypes.data, 0, 0))
            ms_call = timed(call)
            print(json.dumps(dict(measurement="2 host", shape=[steps, ny, nx], hemisphere=hemisphere, chunk_steps=chunk, rows_in=[r0, r1], rows_out=[a0, a1],
                                  mb_in=round(steps * (r1 - r0) * row / 1e6, 1), mb_out=round(steps * (a1 - a0) * row / 1e6, 1), call=ms_call,
                                  pinned_copies=ms_floor, ratio=round(ms_call["best"] / ms_floor["best"], 3),
                                  stream_ms={k: round(v, 1) for k, v in trk.stream_times().items()})), flush=True)
    finally:
        trk.free(d_x)
        trk.free(d_o)
    # ---- 3 -------------------------------------------------------------------------------------------------------------------
    tab = table("both")
    wrow = row_weights(lat.astype(np.float32), np.float32(res), np.float32(360.0 / nx))
    thr = np.zeros(steps)
    op = _native.CMP_OPS[">"]

    def chain():
        trk.reversal(z, tab, keep_resident=True)
        return trk.track_resident(thr, op, wrow, 0.5, 5)

    def round_trip():
        return trk.track(trk.reversal(z, tab), thr, op, wrow, 0.5, 5)
    fa, na = chain()
    fa = np.array(fa)                                                          # (the tracker hands out pooled result arrays)
    fb, nb = round_trip()
    same = bool(na == nb and np.array_equal(fa, fb))
    ms_chain, ms_trip = timed(chain), timed(round_trip)
    print(json.dumps(dict(measurement="3 chain", shape=[steps, ny, nx], identical=same, tracked=int(na), resident_chain=ms_chain, host_round_trip=ms_trip,
                          difference_ms=round(ms_trip["best"] - ms_chain["best"], 2))), flush=True)
