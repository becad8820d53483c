"""Segment breaks (ctk_set_segments) on a device-resident slab: what one segmented call costs against the unsegmented call on the
same slab and against a loop of one ctk_track_*_dev call per segment (what a caller had to do before).

Layouts (LAYOUTS="a,b,c", default all):
  a  2707 x 181 x 360 float32, 30 DJF winters (segments of 90 / 91 steps)
  b  CESM grid 192 x 288 float64, 40 members of 1000 steps
  c  14 600 x 721 x 1440 float32, 10 years of 1460 steps
The slab is synth_fill's field (float64: the same values widened), threshold 160 '>=', overlap 0.5, persistence 5 (20 at 0.25 deg).
Timing: HIP events recorded on the handle's stream around each variant (the calls return after the pass: the events bracket it
completely), WARMUP untimed rounds, then REPS rounds in which the three variants run in turn (alternated, so that drift hits all
alike).  Reported: median and minimum ms per variant and the ratios of the medians.  One JSON line with every layout.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/segments_probe.py` for the kernel statistics."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native                       # noqa: E402
from contrack_amd.contrack import row_weights           # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
WARMUP = int(os.environ.get("WARMUP", "3"))

LAYOUTS = {
    "a": dict(T=2707, ny=181, nx=360, f64=False, persistence=5, nseg=30, name="2707x181x360 f32, 30 winters"),
    "b": dict(T=40000, ny=192, nx=288, f64=True, persistence=5, nseg=40, name="40 members x 1000 x 192x288 f64"),
    "c": dict(T=14600, ny=721, nx=1440, f64=False, persistence=20, nseg=10, name="14600x721x1440 f32, 10 years"),
}


class HipEvents:
    """hipEventRecord on the handle's stream through the HIP runtime the library itself uses"""

    def __init__(self, trk):
        self.hip = C.CDLL("libamdhip64.so")
        _native.lib().ctk_stream.restype = C.c_void_p
        _native.lib().ctk_stream.argtypes = [C.c_void_p]
        self.stream = C.c_void_p(_native.lib().ctk_stream(trk._h))
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.e0)) == 0 and self.hip.hipEventCreate(C.byref(self.e1)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.e0, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.e1, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return float(ms.value)

    def close(self):
        self.hip.hipEventDestroy(self.e0)
        self.hip.hipEventDestroy(self.e1)


def fill(trk, d_in, T, ny, nx, f64):
    if not f64:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        return
    per = 1000
    tmp = trk.malloc(per * ny * nx * 4)
    buf = np.empty((per, ny, nx), dtype=np.float32)
    for t0 in range(0, T, per):
        nt = min(per, T - t0)
        trk.synth_fill(tmp, nt, ny, nx, seed=0, t0=t0)
        trk.d2h(buf[:nt], tmp)
        trk.h2d(C.c_void_p(d_in.value + t0 * ny * nx * 8), buf[:nt].astype(np.float64))
    trk.free(tmp)


def run(key):
    L = LAYOUTS[key]
    T, ny, nx, f64 = L["T"], L["ny"], L["nx"], L["f64"]
    esz = 8 if f64 else 4
    starts = np.array([int(round(k * T / L["nseg"])) for k in range(L["nseg"])], dtype=np.int64)
    bounds = list(zip(starts.tolist(), starts[1:].tolist() + [T]))
    trk = _native.Tracker(0)
    d_in, d_out = trk.malloc(T * ny * nx * esz), trk.malloc(T * ny * nx * 4)
    fill(trk, d_in, T, ny, nx, f64)
    lat = np.linspace(90.0, -90.0, ny, dtype=np.float32)
    w = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    thr = np.full(T, np.float64(np.float32(160.0)))
    args = (0, w, 0.5, L["persistence"], True)
    res = {}

    def unseg():
        res["unseg"] = trk.track_dev(d_in, T, ny, nx, thr, *args, d_out, f64=f64)

    def seg():
        trk.set_segments(starts)
        try:
            res["seg"] = trk.track_dev(d_in, T, ny, nx, thr, *args, d_out, f64=f64)
        finally:
            trk.clear_segments()

    def loop():
        for a, b in bounds:
            trk.track_dev(C.c_void_p(d_in.value + a * ny * nx * esz), b - a, ny, nx, thr[a:b], *args,
                          C.c_void_p(d_out.value + a * ny * nx * 4), f64=f64)

    ev = HipEvents(trk)
    variants = [("unsegmented", unseg), ("segmented", seg), ("per_segment_loop", loop)]
    for _ in range(WARMUP):
        for _, fn in variants:
            fn()
    times = {k: [] for k, _ in variants}
    for _ in range(REPS):
        for k, fn in variants:
            times[k].append(ev.time(fn))
    ev.close()
    st = trk.stats()
    out = dict(layout=key, name=L["name"], shape=[T, ny, nx], f64=f64, segments=len(starts), reps=REPS, warmup=WARMUP,
               n_tracked_unsegmented=res["unseg"], n_tracked_segmented=res["seg"], fused_pass_last=st["fused_pass"])
    for k in times:
        out[k + "_ms_median"] = float(np.median(times[k]))
        out[k + "_ms_min"] = float(np.min(times[k]))
    out["segmented_over_unsegmented"] = out["segmented_ms_median"] / out["unsegmented_ms_median"]
    out["loop_over_segmented"] = out["per_segment_loop_ms_median"] / out["segmented_ms_median"]
    trk.free(d_in)
    trk.free(d_out)
    trk.close()
    return out


def main():
    keys = [k for k in os.environ.get("LAYOUTS", "a,b,c").split(",") if k]
    rows = [run(k) for k in keys]
    print(json.dumps(dict(probe="segments", layouts=rows)))


if __name__ == "__main__":
    main()
