"""run_lifecycle reductions on host arrays, resident and streamed, in one process (profiles/NOTES.md): ms per call, best and median of
`reps` after a warm-up, host clock around calls that end in a synchronisation.  The flags are those of a tracked `synth` slab
(threshold 160 '>=', overlap 0.5, persistence 5), the field is the slab itself, float32.
  (a) Tracker.lifecycle                 -- ctk_lifecycle_f32: two whole-slab copies from pageable memory, then the reductions
  (b) Tracker.lifecycle_stream          -- ctk_lifecycle_stream_f32 at the default chunk (about 256 MB of field), pick = fragile_rows;
                                           ctk_stream_times of the last call goes with it
  (b') the same through reader callbacks that copy from the arrays into the library's pinned buffers
  (c) plain copies of the same 2 x slab bytes from pinned (registered) host memory in the same chunk sizes: the floor of (b)
The rows of (a) and (b) are compared (t, label, shift, area equal; the sums to 1e-12), and so are the frames after the exact rows.
One JSON line.  Usage: python tools/life_stream_probe.py [T ny nx [reps]]      (default: 2707 181 360 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native, synth                                         # noqa: E402
from contrack_amd.contrack import fragile_rows, lifecycle_frame, row_weights    # noqa: E402

argv = sys.argv[1:]
T, ny, nx = (int(v) for v in argv[:3]) if len(argv) >= 3 else (2707, 181, 360)
reps = int(argv[3]) if len(argv) >= 4 else 5


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
    lat, lon = synth.grid(ny, nx)
    wrow = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
    nb = T * ny * nx * 4
    d_in, d_flag = trk.malloc(nb), trk.malloc(nb)
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, wrow, 0.5, 5, True, d_flag)
        field, flag = np.empty((T, ny, nx), dtype=np.float32), np.empty((T, ny, nx), dtype=np.int32)
        trk.d2h(field, d_in)
        trk.d2h(flag, d_flag)
        chunk = max(1, min(T, (256 << 20) // (ny * nx * 4)))
        dates = ["%06d" % t for t in range(T)]

        rows_a = trk.lifecycle(flag, field, wrow)
        frame_a = lifecycle_frame(rows_a, lat, lon, dates, trk)
        rows_b, idx, ex = trk.lifecycle_stream(flag, field, wrow, pick=fragile_rows)
        path, _ = trk.debug_lifecycle_path(T)
        same = bool(all(np.array_equal(rows_a[k], rows_b[k]) for k in ("t", "label", "shift", "area")) and
                    all(np.allclose(rows_a[k], rows_b[k], rtol=1e-12, atol=1e-9) for k in ("swv", "swvy", "swvx")) and
                    lifecycle_frame(rows_b, lat, lon, dates, exact=(idx, ex)) == frame_a)

        def fread(t0, nt, out):
            out[...] = flag[t0:t0 + nt]

        def vread(t0, nt, out):
            out[...] = field[t0:t0 + nt]

        res = dict(shape=[T, ny, nx], reps=reps, n_tracked=n_tracked, rows=len(rows_a), exact_rows=len(idx), chunk_steps=chunk, identical=same,
                   given_up=path["given_up"], gb_each_way=nb / 1e9)
        res["a_lifecycle"] = timed(lambda: trk.lifecycle(flag, field, wrow))
        res["b_stream"] = timed(lambda: trk.lifecycle_stream(flag, field, wrow, pick=fragile_rows))
        res["b_stream_times"] = {k: round(v, 2) for k, v in trk.stream_times().items()}
        res["b_stream_no_pick"] = timed(lambda: trk.lifecycle_stream(flag, field, wrow))
        res["b_readers"] = timed(lambda: trk.lifecycle_stream(fread, vread, wrow, shape=flag.shape, dtype=np.float32, pick=fragile_rows))
        res["b_readers_times"] = {k: round(v, 2) for k, v in trk.stream_times().items()}
        res["a_again"] = timed(lambda: trk.lifecycle(flag, field, wrow))
        for buf in (flag, field):
            _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

        def floor():
            for t0 in range(0, T, chunk):
                trk.h2d(d_flag, flag[t0:t0 + chunk])
                trk.h2d(d_in, field[t0:t0 + chunk])
        res["c_pinned_copies"] = timed(floor)
        for buf in (flag, field):
            _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
        res["b_over_a"] = round(res["b_stream"]["best"] / res["a_lifecycle"]["best"], 3)
        res["b_over_c"] = round(res["b_stream"]["best"] / res["c_pinned_copies"]["best"], 3)
        print(json.dumps(res), flush=True)
    finally:
        trk.free(d_in)
        trk.free(d_flag)
