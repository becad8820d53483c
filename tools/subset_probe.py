"""Selection of tracks or rows of a flag slab (ctk_subset*, k_subset) on a realistic flag: the flag that track_dev makes of a
device-generated synth_fill slab (the bench's workload: threshold 160 '>=', overlap 0.5, persistence 5 at 1 deg / 20 at 0.25 deg) and
the life-cycle rows of that flag.  Everything in one process, best of REPS, integers only, so that every figure has its yardstick from
the same session.

Per shape (SHAPES="T,ny,nx;...", default 2707 x 181 x 360 and 480 x 721 x 1440):
  (a) k_subset alone (HIP events, ctk_debug_time_subset) into a second buffer: by id with up to 440 of the tracked ids (the bitmap), by
      row with every second row of the frame, the same with hits, and count only (no output buffer; by id with hits, by row with hits);
      beside them the plain 16-byte copy kernel over the same two buffers (the hook with a null table) and k_freq on the same flag
      (ctk_debug_time_freq): fraction = copy / kernel;
  (b) host arrays (slabs up to HOST_MAX_GB): ctk_subset on the host array at the default chunk, and plain copies of the same bytes in
      and out between pinned (registered) host memory and the device in the same chunks, one after the other -- the floor; the result
      is compared with np.isin / np.where on the same array.
One JSON line per shape.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/subset_probe.py` for the kernel statistics."""
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
N_IDS = int(os.environ.get("N_IDS", "440"))


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
        d_in, d_flag, d_out = trk.malloc(nb), trk.malloc(nb), trk.malloc(nb)
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        lat = np.linspace(90.0, -90.0, ny, dtype=np.float32)
        w = row_weights(lat, np.float32(180.0 / (ny - 1)), np.float32(360.0 / nx))
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, w, 0.5, 5 if ny <= 181 else 20, True, d_flag)
        rows = trk.lifecycle_dev(d_flag, d_in, T, ny, nx, w)
        trk.free(d_in)
        _, nonzero = trk.checksum_i32(d_flag, T * npix)
        ids = np.unique(rows["label"])[:N_IDS]
        by_id = subset_table(ids)
        by_row = subset_table(rows["label"][::2], rows["t"][::2], T)
        d_maps = trk.malloc(npix * 4)
        out = dict(shape=[T, ny, nx], reps=REPS, n_tracked=int(n_tracked), frame_rows=int(len(rows)), flagged_fraction=round(nonzero / (T * npix), 5),
                   gb=round(nb / 1e9, 3), ids=int(len(ids)), max_id=int(ids.max()) if len(ids) else 0, rows=int(len(by_row[1])),
                   longest_slice=int(np.diff(by_row[0]).max()))
        out["copy_ms"] = round(trk.time_subset(d_flag, T, ny, nx, None, d_out, reps=REPS)[0], 4)
        out["k_freq_ms"] = round(trk.time_freq(d_flag, T, ny, nx, d_maps, reps=REPS)[0], 4)
        forms = {}
        for name, table, dst, hits in (("by_id", by_id, d_out, False), ("by_id_hits", by_id, d_out, True), ("by_row", by_row, d_out, False),
                                       ("by_row_hits", by_row, d_out, True), ("count_by_id_hits", by_id, None, True), ("count_by_row_hits", by_row, None, True),
                                       ("by_id_in_place_invert_of_nothing", subset_table([]), d_flag, False)):
            # (the last one keeps every f > 0: in place it leaves the flag as it is, so the figures after it measure the same slab)
            best, mean = trk.time_subset(d_flag, T, ny, nx, table, dst, invert=dst is d_flag, want_hits=hits, reps=REPS)
            form, vec, grid = trk.debug_subset_launch()
            forms[name] = dict(ms=round(best, 4), mean_ms=round(mean, 4), form=_native.SUBSET_FORMS[form], vec=vec, workgroups=grid,
                               fraction_of_copy=round(out["copy_ms"] / best, 3), over_k_freq=round(best / out["k_freq_ms"], 3),
                               tb_per_s=round((nb if dst is None else 2 * nb) / best / 1e9, 3))
        out["k_subset"] = forms
        out["dev_call_ms"] = timed(lambda: trk.subset_dev(d_flag, T, ny, nx, by_id, d_out, want_hits=False), REPS)
        if nb <= HOST_MAX_GB * 1e9:
            flag = np.empty((T, ny, nx), dtype=np.int32)
            res = np.empty_like(flag)
            trk.d2h(flag, d_flag)
            chunk = max(1, min(T, (256 << 20) // (npix * 4)))
            out["chunk_steps"] = chunk
            c = _native._SubsetCall(by_id, False, 'id', False)

            def call():
                _native.check(L.ctk_subset(trk.handle, flag.ctypes.data, T, ny, nx, *c.table, res.ctypes.data, *c.counts(), 0))
            out["host_subset_ms"] = timed(call, REPS)
            out["host_stream_ms"] = {k: round(v, 1) for k, v in trk.stream_times().items()}
            t0 = time.perf_counter()
            want = np.where(np.isin(flag, by_id[1]), flag, 0)
            out["numpy_isin_where_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out["host_equal_numpy"] = bool(np.array_equal(res, want) and int(c.n.value) == int(np.count_nonzero(want)))
            for buf in (flag, res):
                _native.check(L.ctk_host_register(trk.handle, buf.ctypes.data, buf.nbytes))

            def floor():
                for c0 in range(0, T, chunk):
                    trk.h2d(d_flag, flag[c0:c0 + chunk])
                    trk.d2h(res[c0:c0 + chunk], d_flag)
            out["pinned_copies_ms"] = timed(floor, REPS)
            for buf in (flag, res):
                _native.check(L.ctk_host_unregister(trk.handle, buf.ctypes.data))
            out["host_subset_over_copies"] = round(out["host_subset_ms"] / out["pinned_copies_ms"], 3)
            del flag, res, want
        print(json.dumps(out), flush=True)
        for p in (d_maps, d_flag, d_out):
            trk.free(p)
        trk.close()


if __name__ == "__main__":
    main()
