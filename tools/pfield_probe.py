"""ctk_percentile_field_* on a synthetic slab in device memory (ctk_debug_time_percentile_field): ms per call of the form ctk_pfield_plan
chooses, of the direct form forced on the same input in the same process, and of one plain 16-byte read stream of the band; whether
the two fields are identical.  With --cpu also np.nanquantile(pool, q, axis=0) of ONE group's pool on the host (what
tests/pfield_util.want_field does per group), scaled by the number of groups and labelled as scaled.  One JSON line per case
(profiles/NOTES.md).  Daily steps from 1981-01-01, groups = day of year (366), window 31, q = 0.9.
Usage: python tools/pfield_probe.py [--cpu] [T ny nx y0 y1 [reps]]      (default: 2707 181 360 0 181 2)"""
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
reps = int(argv[5]) if len(argv) >= 6 else 2
W, q = 31, 0.9
stamps = np.datetime64("1981-01-01") + np.arange(T)
doy = (stamps - stamps.astype("datetime64[Y]")).astype(int)          # 0 .. 365
G = int(doy.max()) + 1
group = doy.astype(np.int32)
steps = np.bincount(group, minlength=G)
longest = max(int(sum(steps[(g + d) % G] for d in range(-(W // 2), (W - 1) // 2 + 1))) for g in range(G)) if W < G else T
with _native.Tracker(0) as trk:
    d = trk.malloc(T * ny * nx * 4)
    try:
        trk.synth_fill(d, T, ny, nx, seed=1)
        a, b, ms_chosen, ms_direct, ms_read, form = trk.time_percentile_field(d, T, ny, nx, y0, y1, group, G, q, window=W, reps=reps)
        res = dict(shape=[T, ny, nx], rows=[y0, y1], groups=G, window=W, q=q, longest_pool=longest, plan=_native.debug_percentile_field_plan(4, longest, G, W),
                   form="ring" if form == 1 else "direct", ms_chosen=round(ms_chosen, 3), ms_direct_forced=round(ms_direct, 3), ms_read_stream=round(ms_read, 3),
                   identical=bool(np.array_equal(a, b, equal_nan=True)), nan=int(np.isnan(a).sum()), min=float(np.nanmin(a)), max=float(np.nanmax(a)))
        if cpu:
            g = G // 2
            members = sorted({(g + dd) % G for dd in range(-(W // 2), (W - 1) // 2 + 1)})
            ts = np.nonzero(np.isin(group, members))[0]
            plane = np.empty((ny, nx), dtype=np.float32)
            pool = np.empty((len(ts), y1 - y0, nx), dtype=np.float64)
            for i, t in enumerate(ts):
                trk.d2h(plane, _native.C.c_void_p(d.value + int(t) * ny * nx * 4))
                pool[i] = plane[y0:y1]
            t0 = time.perf_counter()
            ref = np.nanquantile(pool, q, axis=0)
            one = time.perf_counter() - t0
            res.update(cpu_one_group_s=round(one, 3), cpu_scaled_by_groups_s=round(one * G, 1), cpu_group_identical=bool(np.array_equal(ref, a[g], equal_nan=True)))
        print(json.dumps(res), flush=True)
    finally:
        trk.free(d)
