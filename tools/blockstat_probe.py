"""Per-block peak and extent (ctk_blockstat*, k_blockstat) on a realistic flag: the flag that track_dev makes of a device-generated
synth_fill slab (the bench's workload: threshold 160 '>=', overlap 0.5, persistence 5 at 1 deg / 20 at 0.25 deg), the slab itself as
the field, and every life-cycle row of that flag as the table.  Everything in one process, best of REPS, so that every figure has its
yardstick from the same session.

Per shape (SHAPES="T,ny,nx;...", default 2707 x 181 x 360 and 480 x 721 x 1440):
  (a) k_blockstat alone (HIP events, ctk_debug_time_blockstat): shape only, peaks only, both; beside it, in the same process,
      the plain stream of 16-byte loads over the flag slab alone and over both slabs (the hook with a null table), k_composite on the
      same two slabs (ctk_debug_time_composite) and k_subset with hits on every second frame row (ctk_debug_time_subset, count only):
      over_loads = kernel / load stream over the buffers the kernel is given;
  (b) host arrays (slabs up to HOST_MAX_GB): ctk_blockstat_f32 on the host arrays at the default chunk, and plain copies of the same
      bytes between pinned (registered) host memory and the device in the same chunks -- the floor.
One JSON line per shape.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/blockstat_probe.py` for the kernel statistics."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native                                       # noqa: E402
from contrack_amd.contrack import row_weights, subset_table             # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
HOST_MAX_GB = float(os.environ.get("HOST_MAX_GB", "4"))


def timed(fn, reps):
    fn()                                                                       # warm-up: code objects, allocations, pinned buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(min(ms), 3)


def main():
    L = _native.lib()
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", "2707,181,360;480,721,1440").split(";")]
    for T, ny, nx in shapes:
        trk = _native.Tracker(0)
        npix = ny * nx
        nb = T * npix * 4
        d_x, d_flag = trk.malloc(nb), trk.malloc(nb)
        trk.synth_fill(d_x, T, ny, nx, seed=0)
        lat = np.linspace(90.0, -90.0, ny, dtype=np.float32)
        w = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
        n_tracked = trk.track_dev(d_x, T, ny, nx, np.full(T, 160.0), 0, w, 0.5, 5 if ny <= 181 else 20, True, d_flag)
        rows = trk.lifecycle_dev(d_flag, d_x, T, ny, nx, w)
        _, nonzero = trk.checksum_i32(d_flag, T * npix)
        table = subset_table(rows["label"], rows["t"], T)
        half = subset_table(rows["label"][::2], rows["t"][::2], T)
        longest = int(np.diff(table[0]).max())
        plan = _native.blockstat_plan(("shape", "peaks"), longest, ny, nx, steps=T)
        out = dict(shape=[T, ny, nx], reps=REPS, n_tracked=int(n_tracked), entries=int(len(table[1])), longest_slice=longest,
                   flagged_fraction=round(nonzero / (T * npix), 5), gb_per_slab=round(nb / 1e9, 3), lds_bytes=plan["lds"], lds_entries=plan["lds_entries"])
        out["loads_flag_ms"] = round(trk.time_blockstat(d_flag, None, T, ny, nx, None, reps=REPS)[0], 4)
        out["loads_both_ms"] = round(trk.time_blockstat(d_flag, d_x, T, ny, nx, None, reps=REPS)[0], 4)
        d_sum, d_n = trk.malloc(npix * 8), trk.malloc(npix * 4)
        out["k_composite_ms"] = round(trk.time_composite(d_flag, d_x, T, ny, nx, d_sum, d_n, reps=REPS)[0], 4)
        out["k_subset_half_rows_hits_ms"] = round(trk.time_subset(d_flag, T, ny, nx, half, None, want_hits=True, reps=REPS)[0], 4)
        kern = {}
        for name, want, floor in (("shape", "shape", "loads_flag_ms"), ("peaks", "peaks", "loads_both_ms"), ("both", ("shape", "peaks"), "loads_both_ms")):
            best, mean = trk.time_blockstat(d_flag, d_x, T, ny, nx, table, want, reps=REPS)
            form, vec, grid = trk.debug_blockstat_launch()
            kern[name] = dict(ms=round(best, 4), mean_ms=round(mean, 4), form=_native.BLOCKSTAT_FORMS[form], vec=vec, workgroups=grid,
                              over_loads=round(best / out[floor], 3), over_k_composite=round(best / out["k_composite_ms"], 3),
                              over_k_subset=round(best / out["k_subset_half_rows_hits_ms"], 3))
        out["k_blockstat"] = kern
        out["dev_call_ms"] = timed(lambda: trk.blockstat_dev(d_flag, d_x, T, ny, nx, table), REPS)
        if nb <= HOST_MAX_GB * 1e9:
            flag, x = np.empty((T, ny, nx), dtype=np.int32), np.empty((T, ny, nx), dtype=np.float32)
            trk.d2h(flag, d_flag)
            trk.d2h(x, d_x)
            dev_rows = trk.blockstat_dev(d_flag, d_x, T, ny, nx, table)
            chunk = max(1, min(T, (256 << 20) // (npix * 4)))
            out["chunk_steps"] = chunk
            got = {}

            def call():
                got["rows"] = trk.blockstat(flag, table, x)
            out["host_blockstat_ms"] = timed(call, REPS)
            out["host_stream_ms"] = {k: round(v, 1) for k, v in trk.stream_times().items()}
            out["host_equal_dev"] = bool(got["rows"].tobytes() == dev_rows.tobytes())
            out["pixels_counted"], out["pixels_flagged"] = int(got["rows"]["n"].sum()), int(nonzero)
            for buf in (flag, x):
                _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

            def floor():
                for c0 in range(0, T, chunk):
                    trk.h2d(d_flag, flag[c0:c0 + chunk])
                    trk.h2d(d_x, x[c0:c0 + chunk])
            out["pinned_copies_ms"] = timed(floor, REPS)
            for buf in (flag, x):
                _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
            out["host_blockstat_over_copies"] = round(out["host_blockstat_ms"] / out["pinned_copies_ms"], 3)
            del flag, x
        print(json.dumps(out), flush=True)
        for p in (d_sum, d_n, d_flag, d_x):
            trk.free(p)
        trk.close()


if __name__ == "__main__":
    main()
