"""ctk_percentile_groups_f32 at BASELINE configs[2] (14 600 x 721 x 1440 float32, band 30-90N = rows 0..240, 6-hourly steps, 365
calendar days, window 31, q = 0.1) on a synthetic slab in device memory: ms per call, ms of one plain 16-byte read of the band (times
the number of sweeps = the floor), ms of every sweep, ms of today's scalar percentile's kernels.  One JSON line per case
(profiles/NOTES.md).  Usage: python tools/pctl_probe.py [T ny nx y1]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native

T, ny, nx, y1 = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (14600, 721, 1440, 241)
with _native.Tracker(0) as trk:
    d = trk.malloc(T * ny * nx * 4)
    try:
        trk.synth_fill(d, T, ny, nx, seed=1)
        days = ((np.arange(T) // 4) % 365).astype(np.int32)
        cases = [("G365_W31", days, 365, 31), ("G365_W1", days, 365, 1)]
        if T * y1 * nx < 2 ** 32:                         # (one group of every step: its uint32 counters must hold the whole band)
            cases.append(("G1_W1", np.zeros(T, np.int32), 1, 1))
        for name, group, G, W in cases:
            vals, ms_call, ms_read, ms_scalar, ms_sweeps = trk.time_percentile_groups(d, T, ny, nx, 0, y1, group, G, 0.1, window=W, reps=2)
            print(json.dumps(dict(case=name, shape=[T, ny, nx], band_rows=y1, ms_call=round(ms_call, 3), ms_read=round(ms_read, 3),
                                  sweeps=len(ms_sweeps), ms_floor=round(ms_read * len(ms_sweeps), 3), ms_sweeps=[round(v, 3) for v in ms_sweeps],
                                  ms_scalar_percentile=round(ms_scalar, 3), min=float(np.nanmin(vals)), max=float(np.nanmax(vals)),
                                  nan=int(np.isnan(vals).sum()))), flush=True)
    finally:
        trk.free(d)
