"""ctk_std_field_* on a synthetic float32 slab in device memory (ctk_debug_time_std_field): ms per call, against the floor of its two
passes -- one plain 16-byte read stream of the band, times two -- and against ctk_percentile_field_* on the same slab in the same
process (ctk_debug_time_percentile_field, which also times the read stream).  With --cpu also np.nanstd(pool, axis=0) of ONE group's
pool on the host, compared with that group's plane bit for bit, scaled by the number of groups and labelled as scaled.  One JSON line
per case (profiles/NOTES.md).  One process, best of `reps`.  Daily steps from 1981-01-01, groups = day of year (366), window 31.
Usage: python tools/std_probe.py [--cpu] [T ny nx y0 y1 [reps]]      (default: 2707 181 360 0 181 5; the large case:
14600 721 1440 0 241 5, the band 30-90N)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native

argv = [a for a in sys.argv[1:] if a != "--cpu"]
cpu = "--cpu" in sys.argv[1:]
T, ny, nx, y0, y1 = (int(v) for v in argv[:5]) if len(argv) >= 5 else (2707, 181, 360, 0, 181)
reps = int(argv[5]) if len(argv) >= 6 else 5
W, q = 31, 0.9
stamps = np.datetime64("1981-01-01") + np.arange(T)
doy = (stamps - stamps.astype("datetime64[Y]")).astype(int)          # 0 .. 365
G = int(doy.max()) + 1
group = doy.astype(np.int32)
small = (y1 - y0) * nx * G * 8 <= 1 << 30                            # the fields are brought to the host only where they are small
with _native.Tracker(0) as trk:
    d = trk.malloc(T * ny * nx * 4)
    try:
        trk.synth_fill(d, T, ny, nx, seed=1)
        field, ms_std, tile = trk.time_std_field(d, T, ny, nx, y0, y1, group, G, window=W, ddof=0, skipna=True, reps=reps, want_field=small)
        _, ms_plain, _ = trk.time_std_field(d, T, ny, nx, y0, y1, group, G, window=W, ddof=0, skipna=False, reps=reps, want_field=False)
        _, ms_w1, _ = trk.time_std_field(d, T, ny, nx, y0, y1, group, G, window=1, ddof=0, skipna=True, reps=reps, want_field=False)
        longest = trk.debug_std_field_form()[1]
        _, _, ms_pf, _, ms_read, form = trk.time_percentile_field(d, T, ny, nx, y0, y1, group, G, q, window=W, reps=reps, want_fields=False)
        res = dict(shape=[T, ny, nx], rows=[y0, y1], groups=G, window=W, plan=_native.debug_std_field_plan(G, W, True), tile=tile,
                   ms_std_field=round(ms_std, 3), ms_std_field_no_skipna=round(ms_plain, 3), ms_std_field_window_1=round(ms_w1, 3),
                   ms_read_stream=round(ms_read, 3), ms_two_streams=round(2 * ms_read, 3), times_two_streams=round(ms_std / (2 * ms_read), 1),
                   ms_percentile_field=round(ms_pf, 3), percentile_form="ring" if form == 1 else "direct",
                   updates_per_pass=int(T) * W * (y1 - y0) * nx)
        if field is not None:
            res.update(nan=int(np.isnan(field).sum()), min=float(np.nanmin(field)), max=float(np.nanmax(field)))
        if cpu and field is not None:
            g = G // 2
            members = sorted({(g + dd) % G for dd in range(-(W // 2), (W - 1) // 2 + 1)})
            ts = np.nonzero(np.isin(group, members))[0]
            plane = np.empty((ny, nx), dtype=np.float32)
            pool = np.empty((len(ts), y1 - y0, nx), dtype=np.float64)
            for i, t in enumerate(ts):
                trk.d2h(plane, _native.C.c_void_p(d.value + int(t) * ny * nx * 4))
                pool[i] = plane[y0:y1]
            t0 = time.perf_counter()
            ref = np.nanstd(pool, axis=0)
            one = time.perf_counter() - t0
            res.update(cpu_one_group_s=round(one, 4), cpu_scaled_by_groups_s=round(one * G, 2), cpu_group_identical=bool(np.array_equal(ref, field[g], equal_nan=True)))
        print(json.dumps(res), flush=True)
    finally:
        trk.free(d)
