"""Threshold field (k_threshold_field) against the scalar threshold kernel (k_threshold_v7) on the same slab and handle.

Per shape (SHAPES="T,ny,nx;T,ny,nx", default the bench slab 2707 x 181 x 360 and 480 x 721 x 1440), on a device-generated slab:
  scalar       per-step thresholds                                   -> k_threshold_v7
  doy          a 366-plane float32 field, DJF day-of-year planes     -> k_threshold_field, steps in plane-major order
  full         a (T, ny, nx) float32 field: 8 B/px read
  load8        a plain 16-byte load stream over T * ny * nx * 8 bytes (ctk_debug_stream_ceiling mode 0)
Times are the handle's HIP-event timers around the threshold kernel (mean over REPS passes); run it under
`rocprofv3 --kernel-trace --stats -- python tools/thr_field_probe.py` for the per-kernel statistics.  One JSON line per shape."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native                       # noqa: E402
from contrack_amd.contrack import row_weights           # noqa: E402

REPS = int(os.environ.get("REPS", "10"))


def planes(n, ny, nx, seed):
    rng = np.random.default_rng(seed)
    y = np.linspace(0.0, np.pi, ny, dtype=np.float32)[None, :, None]
    x = np.linspace(0.0, 2 * np.pi, nx, endpoint=False, dtype=np.float32)[None, None, :]
    ph = rng.uniform(0.0, 2 * np.pi, (n, 2, 1, 1)).astype(np.float32)
    return (np.float32(160.0) + np.float32(40.0) * np.sin(2 * y + ph[:, 0]) * np.cos(3 * x + ph[:, 1])).astype(np.float32)


def thr_ms(trk, call):
    for _ in range(2):
        call()
    trk.timing_sums(reset=True)
    for _ in range(REPS):
        call()
    per, _ = trk.timing_sums(reset=True)
    return per["k_threshold"]


def main():
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", "2707,181,360;480,721,1440").split(";")]
    for T, ny, nx in shapes:
        trk = _native.Tracker(0)
        trk.set_timing(2)
        nb = T * ny * nx * 4
        d_in, d_out, d_ld = trk.malloc(nb), trk.malloc(nb), trk.malloc(2 * nb)
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        lat = np.linspace(90.0, -90.0, ny, dtype=np.float32)
        w = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
        d = np.datetime64("2000-12-01") + (np.arange(T) % 90)
        doy0 = (d - d.astype("datetime64[Y]")).astype(int).astype(np.int32)
        run = lambda thr: trk.track_dev(d_in, T, ny, nx, thr, 0, w, 0.5, 5, True, d_out)
        out = dict(shape=[T, ny, nx], reps=REPS)
        out["scalar_ms"] = thr_ms(trk, lambda: run(np.full(T, 160.0)))
        doy = planes(366, ny, nx, 1)
        trk.set_threshold_field(doy, doy0)
        out["doy_ms"] = thr_ms(trk, lambda: run(None))
        base = planes(16, ny, nx, 2)
        trk.set_threshold_field(base[np.arange(T) % 16], np.arange(T, dtype=np.int32))
        out["full_ms"] = thr_ms(trk, lambda: run(None))
        trk.clear_threshold_field()
        out["load8_ms"] = trk.stream_ceiling(d_ld, 2 * nb, 0, reps=REPS)
        out["doy_over_scalar"] = out["doy_ms"] / out["scalar_ms"]
        out["full_of_load8_stream"] = out["load8_ms"] / out["full_ms"]
        print(json.dumps(out), flush=True)
        for p in (d_in, d_out, d_ld):
            trk.free(p)
        trk.close()


if __name__ == "__main__":
    main()
