"""Reductions over space per time step (ctk_band_*, k_band, k_band_sect) on a realistic flag: the flag that track_dev makes of a
device-generated synth_fill slab (the bench's workload: threshold 160 '>=', overlap 0.5, persistence 5).

    python tools/band_probe.py [T ny nx [reps]]          default: 2707 x 181 x 360 and 480 x 721 x 1440, best of 5, one process

Per shape, one JSON line:
  (a) the kernel alone between HIP events (ctk_debug_time_band), full-plane band, no field, columns only -- beside its yardsticks on
      the same device buffer: k_freq with one group (ctk_debug_time_freq) and the plain 16-byte load stream
      (ctk_debug_stream_ceiling); then the sweep of the rows in flight (1 .. 16) and the general form;
  (b) the kernel's other shapes: the 50-75N band, a float32 field (the tracked slab itself), 4 sectors, and both;
  (c) the streamed host-array call (Tracker.band, columns and 4 sectors) against Tracker.frequency on the same array and against plain
      copies of the same bytes from pinned (registered) host memory in the same chunks -- the floor; the same with the field.
The results of (c) are compared with each other (array against device entry) by bits."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native, synth                                        # noqa: E402
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


def probe(trk, T, ny, nx):
    L = _native.lib()
    lat, lon = synth.grid(ny, nx)
    wrow = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    w = wrow.astype(np.float64)
    nb = T * ny * nx * 4
    d_in, d_flag, d_cnt = trk.malloc(nb), trk.malloc(nb), trk.malloc(ny * nx * 4)
    names = "cnt area wx sec_cnt sec_area sec_wx".split()
    d_out = {k: trk.malloc(T * nx * 8) for k in names}
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, wrow, 0.5, 5, True, d_flag)
        _, nonzero = trk.checksum_i32(d_flag, T * ny * nx)
        rows = np.nonzero((lat >= 50) & (lat <= 75))[0]
        band = (int(rows[0]), int(rows[-1]) + 1)
        sects = [(0, nx // 4), (nx // 4, nx // 4), (nx // 2, nx // 4), (nx - nx // 8, nx // 4)]          # the last one wraps
        res = dict(shape=[T, ny, nx], reps=reps, n_tracked=n_tracked, flagged_fraction=round(nonzero / (T * ny * nx), 5), gb=round(nb / 1e9, 3),
                   band_rows=list(band), plan=_native.debug_band_plan(T, nx))
        # (a) the kernel alone beside its yardsticks
        res["a_load16_ms"] = round(trk.stream_ceiling(d_flag, nb, 0, reps), 4)
        res["a_k_freq_ms"] = round(trk.time_freq(d_flag, T, ny, nx, d_cnt, reps=reps)[0], 4)
        kband = lambda **kw: round(trk.time_band(d_flag, kw.pop("x", None), T, ny, nx, kw.pop("rows", (0, ny)), w, d_out, reps=reps, **kw)[0], 4)
        res["a_k_band_ms"] = kband()
        res["a_k_band_over_k_freq"] = round(res["a_k_band_ms"] / res["a_k_freq_ms"], 3)
        res["a_k_band_over_load16"] = round(res["a_k_band_ms"] / res["a_load16_ms"], 3)
        res["a_k_band_tbs"] = round(nb / res["a_k_band_ms"] / 1e9, 3)
        sweep = {}
        for form in (0, 1):
            for r in (1, 2, 4, 8, 16):
                trk.debug_set_band(form, r)
                sweep["%s_rows%d" % ("vec" if form == 0 else "general", r)] = kband()
        trk.debug_set_band()
        res["a_sweep_ms"] = sweep
        # (b) the kernel's other shapes
        res["b_band_50_75_ms"] = kband(rows=band)
        res["b_field_ms"] = kband(x=d_in)
        res["b_sectors_ms"] = kband(sectors=sects)
        res["b_sectors_only_ms"] = kband(sectors=sects, columns=False)
        res["b_band_field_sectors_ms"] = kband(rows=band, x=d_in, sectors=sects)
        # (c) host arrays, streamed
        flag, field = np.empty((T, ny, nx), dtype=np.int32), np.empty((T, ny, nx), dtype=np.float32)
        trk.d2h(flag, d_flag)
        trk.d2h(field, d_in)
        chunk = max(1, min(T, (256 << 20) // (ny * nx * 4)))
        res["chunk_steps"] = chunk
        res["c_band_ms"] = timed(lambda: trk.band(flag, (0, ny), w, None, sects))
        res["c_band_stream_times"] = {k: round(v, 2) for k, v in trk.stream_times().items()}
        res["c_band_sectors_only_ms"] = timed(lambda: trk.band(flag, (0, ny), w, None, sects, columns=False))
        res["c_frequency_ms"] = timed(lambda: trk.frequency(flag))
        res["c_band_field_ms"] = timed(lambda: trk.band(flag, band, w, field, sects))
        for buf in (flag, field):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor(two):
            for t0 in range(0, T, chunk):
                trk.h2d(d_flag, flag[t0:t0 + chunk])
                if two:
                    trk.h2d(d_in, field[t0:t0 + chunk])
        res["c_pinned_copies_ms"] = timed(lambda: floor(False))
        res["c_pinned_copies_two_slabs_ms"] = timed(lambda: floor(True))
        for buf in (flag, field):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
        res["c_band_over_copies"] = round(res["c_band_ms"] / res["c_pinned_copies_ms"], 3)
        res["c_frequency_over_copies"] = round(res["c_frequency_ms"] / res["c_pinned_copies_ms"], 3)
        res["c_band_field_over_copies"] = round(res["c_band_field_ms"] / res["c_pinned_copies_two_slabs_ms"], 3)
        trk.h2d(d_flag, flag)
        trk.h2d(d_in, field)
        host = trk.band(flag, band, w, field, sects, chunk_steps=max(1, chunk // 3))
        dev = trk.band_dev(d_flag, d_in, T, ny, nx, band, w, sects)
        res["c_identical"] = bool(all(np.array_equal(host[k].view(np.uint64) if host[k].dtype == np.float64 else host[k],
                                                     dev[k].view(np.uint64) if dev[k].dtype == np.float64 else dev[k]) for k in dev))
        res["c_count_is_frequency"] = bool(np.array_equal(trk.band(flag, (0, ny), w)["cnt"].sum(axis=0, dtype=np.int64),
                                                          trk.frequency(flag)[0].sum(axis=0, dtype=np.int64)))
        print(json.dumps(res), flush=True)
    finally:
        for p in [d_in, d_flag, d_cnt] + list(d_out.values()):
            trk.free(p)


def main():
    trk = _native.Tracker(0)
    try:
        for T, ny, nx in shapes:
            probe(trk, T, ny, nx)
    finally:
        trk.close()


if __name__ == "__main__":
    main()
