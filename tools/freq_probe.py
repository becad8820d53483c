"""Blocking frequency (ctk_frequency*, k_freq) on a realistic flag: the flag that track_dev makes of a device-generated synth_fill slab
(the bench's workload: threshold 160 '>=', overlap 0.5, persistence 5 at 1 deg / 20 at 0.25 deg).

Per shape (SHAPES="T,ny,nx;...", default 2707 x 181 x 360, 480 x 721 x 1440 and 14 600 x 721 x 1440), daily steps from 1979-01-01:
  k_freq ms (best and mean of REPS launches between HIP events, ctk_debug_time_freq) and TB/s at 4 bytes per pixel, ungrouped and
  grouped by month, for the library's slice rule (slice 0) and every slice of SLICES, plain and nontemporal (the default) 16-byte loads;
  load16: a plain 16-byte load stream over the same bytes (ctk_debug_stream_ceiling mode 0, best of REPS);
  dev_call: ctk_frequency_dev as a caller sees it (counts zeroed, kernel, stream synchronised), mean of REPS;
  host entries (slabs up to HOST_MAX_GB): ctk_frequency on the host array (default chunks), ungrouped and by month, against numpy
  np.where(flag > 0, 1, 0).sum(0) and a per-month numpy loop on the same array; the results are compared.
One JSON line per shape.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/freq_probe.py` for the kernel statistics."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native                       # noqa: E402
from contrack_amd.contrack import row_weights           # noqa: E402

REPS = int(os.environ.get("REPS", "10"))
SLICES = [int(v) for v in os.environ.get("SLICES", "4,8,16,32,64,128,256").split(",") if v]
HOST_MAX_GB = float(os.environ.get("HOST_MAX_GB", "4"))


def wall_ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", "2707,181,360;480,721,1440;14600,721,1440").split(";")]
    for T, ny, nx in shapes:
        trk = _native.Tracker(0)
        npix = ny * nx
        nb = T * npix * 4
        d_in, d_flag = trk.malloc(nb), trk.malloc(nb)
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        lat = np.linspace(90.0, -90.0, ny, dtype=np.float32)
        w = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, w, 0.5, 5 if ny <= 181 else 20, True, d_flag)
        _, nonzero = trk.checksum_i32(d_flag, T * npix)
        days = np.datetime64("1979-01-01") + np.arange(T)
        month = (days.astype("datetime64[M]").astype(np.int64) % 12).astype(np.int32)
        d_cnt = trk.malloc(12 * npix * 4)
        out = dict(shape=[T, ny, nx], reps=REPS, n_tracked=n_tracked, flagged_fraction=nonzero / (T * npix), gb=nb / 1e9)
        tbs = lambda ms: nb / (ms * 1e-3) / 1e12
        out["load16_ms"] = trk.stream_ceiling(d_in, nb, 0, reps=REPS)
        out["load16_tbs"] = tbs(out["load16_ms"])
        sweep = {}
        for sl in [0] + SLICES:
            for nt in (False, True):
                trk.debug_set_freq(sl, nt)
                for gname, grp in (("all", None), ("month", month)):
                    best, mean = trk.time_freq(d_flag, T, ny, nx, d_cnt, group=grp, ngroups=None if grp is None else 12, reps=REPS)
                    sweep["%s_s%d_%s" % (gname, sl, "nt" if nt else "plain")] = dict(best_ms=best, mean_ms=mean, tbs=tbs(best))
        trk.debug_set_freq(0)
        out["k_freq"] = sweep
        # the library's default: the slice rule, nontemporal loads
        out["k_freq_ms"] = sweep["all_s0_nt"]["best_ms"]
        out["k_freq_tbs"] = sweep["all_s0_nt"]["tbs"]
        out["k_freq_of_load16"] = out["load16_ms"] / sweep["all_s0_nt"]["best_ms"]
        out["k_freq_month_ms"] = sweep["month_s0_nt"]["best_ms"]
        out["k_freq_month_tbs"] = sweep["month_s0_nt"]["tbs"]
        out["dev_call_ms"] = wall_ms(lambda: trk.frequency_dev(d_flag, T, ny, nx, counts_dev=d_cnt), REPS)
        out["dev_call_month_ms"] = wall_ms(lambda: trk.frequency_dev(d_flag, T, ny, nx, group=month, ngroups=12, counts_dev=d_cnt), REPS)
        trk.free(d_in)
        if nb <= HOST_MAX_GB * 1e9:
            flag = np.empty((T, ny, nx), dtype=np.int32)
            trk.d2h(flag, d_flag)
            r = max(1, REPS // 3)
            host = trk.frequency(flag)
            out["host_ms"] = wall_ms(lambda: trk.frequency(flag), r)
            out["host_month_ms"] = wall_ms(lambda: trk.frequency(flag, month, 12), r)
            out["host_input_phase_ms"] = trk.timings()["h2d"]
            t0 = time.perf_counter()
            want = np.where(flag > 0, 1, 0).sum(0)
            out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want_m = np.stack([np.where(flag[month == m] > 0, 1, 0).sum(0) for m in range(12)])
            out["numpy_month_ms"] = (time.perf_counter() - t0) * 1e3
            out["host_equal_numpy"] = bool(np.array_equal(host[0], want) and np.array_equal(trk.frequency(flag, month, 12), want_m))
            del flag
        print(json.dumps(out), flush=True)
        trk.free(d_cnt)
        trk.free(d_flag)
        trk.close()


if __name__ == "__main__":
    main()
