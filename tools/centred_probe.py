"""The block-centred composite, measured in one process on one device (profiles/NOTES.md).  The field is a `synth` slab, float32; the
stamps are the centres of mass of its own tracked blocks (threshold 160 '>=', overlap 0.5, persistence 5; run_lifecycle's rows with
their grid indices), the window +-20 x +-40 degrees, the bins by='age' (one per time step since onset) and one bin.  Best of `reps`.
  (a) the kernel alone between HIP events (Tracker.time_centred): the rule's form, and each of the two forms forced (k_centred, the
      plain one, and k_centred_fed, feeder waves and an owner), against
      - the same windows of the same stamps read by a plain gather with one lane per (stamp, cell), in no order, that keeps nothing
        (time_centred(floor=True): the library's yardstick kernel k_centred_floor) -- what the loads cost when nothing depends on
        anything;
      - k_composite over the whole slab with the blocks' flags (Tracker.time_composite), the grid-point composite of the same data
  (b) Tracker.centred on the host array at the default chunk (about 256 MB of field), host clock; against plain copies of as many
      bytes as actually travel (the chunks that carry stamps, their bands of latitude rows) from pinned (registered) host memory,
      in pieces of the same sizes -- the floor -- and against the copy of the whole slab
  (c) the same call with the field resident (Tracker.anomalies(keep_resident=True) of the slab): no field bytes travel
One JSON line per shape.  Usage: python tools/centred_probe.py [T ny nx [reps]]      (default: 2707 181 360, then 480 721 1440; 5)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native, synth                                         # noqa: E402
from contrack_amd.contrack import centred_stamps, lifecycle_bins, lifecycle_columns, row_weights      # noqa: E402

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


def travelling(t, row, keep, T, ny, hy, chunk):
    """[(first element row, rows)] per chunk that carries stamps, in (T * ny) rows of the slab: what ctk_centred_f32 uploads"""
    pieces = []
    for c0 in range(0, T, chunk):
        sel = keep & (t >= c0) & (t < c0 + chunk)
        if sel.any():
            y0, y1 = max(int(row[sel].min()) - hy, 0), min(int(row[sel].max()) + hy, ny - 1)
            pieces.append((min(chunk, T - c0), y1 - y0 + 1))
    return pieces


def probe(trk, T, ny, nx):
    L = _native.lib()
    lat, lon = synth.grid(ny, nx)
    dlat, dlon = 180.0 / (ny - 1), 360.0 / nx
    wrow = row_weights(lat, np.float32(dlat), np.float32(dlon))
    hy, hx = int(round(20.0 / dlat)), int(round(40.0 / dlon))
    nb = T * ny * nx * 4
    d_in, d_flag = trk.malloc(nb), trk.malloc(nb)
    bufs = [d_in, d_flag]
    try:
        trk.synth_fill(d_in, T, ny, nx, seed=0)
        n_tracked = trk.track_dev(d_in, T, ny, nx, np.full(T, 160.0), 0, wrow, 0.5, 5, True, d_flag)
        rows = trk.lifecycle_dev(d_flag, d_in, T, ny, nx, wrow)
        cols = lifecycle_columns(rows, lat, lon, ["%06d" % k for k in range(T)], indices=True)
        t, row, col, flag_id = centred_stamps(cols["Step"], cols["Row"], cols["Col"], cols["Flag"])
        age, nage = lifecycle_bins(flag_id, t, "age")
        one = np.zeros(len(t), dtype=np.int32)
        cells = (2 * hy + 1) * (2 * hx + 1)
        d_sum, d_n = trk.malloc(max(nage * cells * 8, ny * nx * 8)), trk.malloc(max(nage * cells * 4, ny * nx * 4))
        bufs += [d_sum, d_n]
        res = dict(shape=[T, ny, nx], reps=reps, n_tracked=n_tracked, stamps=len(t), window=[2 * hy + 1, 2 * hx + 1], cells=cells, age_bins=nage,
                   stamps_in_largest_age_bin=int(np.bincount(age).max()), gb_slab=round(nb / 1e9, 3),
                   gb_gathered=round(len(t) * cells * 4 / 1e9, 4))
        # (a) the kernel alone
        def kernel_ms(bins, nbins, form=-1, unroll=-1, threads=-1):
            trk.debug_set_centred(form, unroll, threads)
            try:
                return round(trk.time_centred(d_in, T, ny, nx, t, row, col, bins, nbins, hy, hx, d_sum, d_n, reps=reps)[0], 4)
            finally:
                trk.debug_set_centred(-1, -1, -1)
        for name, bins, nbins in (("age", age, nage), ("one_bin", one, 1)):
            res["plan_" + name] = _native.centred_plan(4, nbins, hy, hx, int(np.bincount(bins).max()), len(bins))
            res["a_kernel_ms_" + name] = kernel_ms(bins, nbins)
            res["a_plain_form_ms_" + name] = kernel_ms(bins, nbins, form=0)
            res["a_fed_form_ms_" + name] = kernel_ms(bins, nbins, form=1)
        # between the two: the first 16 ages (16 bins of many stamps each), where the rule's bound on the workgroups lies
        young = np.where(age < 16, age, -1).astype(np.int32)
        res["stamps_age_below_16"] = int(np.count_nonzero(young >= 0))
        res["plan_age_below_16"] = _native.centred_plan(4, 16, hy, hx, int(np.bincount(young[young >= 0]).max()), res["stamps_age_below_16"])
        res["a_kernel_ms_age_below_16"] = kernel_ms(young, 16)
        res["a_plain_form_ms_age_below_16"] = kernel_ms(young, 16, form=0)
        res["a_fed_form_ms_age_below_16"] = kernel_ms(young, 16, form=1)
        floor, _ = trk.time_centred(d_in, T, ny, nx, t, row, col, one, 1, hy, hx, d_sum, d_n, floor=True, reps=reps)
        res["a_gather_floor_ms"] = round(floor, 4)
        for name in ("age", "one_bin"):
            res["a_ratio_to_floor_" + name] = round(res["a_kernel_ms_" + name] / floor, 2)
        for u in (8, 16):                                                      # the plain form's batch: what a narrower one costs
            res["a_plain_form_ms_one_bin_batch%d" % u] = kernel_ms(one, 1, form=0, unroll=u)
        res["a_plain_form_ms_one_bin_256_cells"] = kernel_ms(one, 1, form=0, threads=256)      # four waves of a bin on one CU
        res["a_k_composite_ms"] = round(trk.time_composite(d_flag, d_in, T, ny, nx, d_sum, d_n, reps=reps)[0], 4)
        # (b) the host array, streamed
        field = np.empty((T, ny, nx), dtype=np.float32)
        trk.d2h(field, d_in)
        chunk = max(1, min(T, (256 << 20) // (ny * nx * 4)))
        pieces = travelling(t, row, age >= 0, T, ny, hy, chunk)
        moved = sum(nt * r for nt, r in pieces) * nx * 4
        res.update(chunk_steps=chunk, chunks=-(-T // chunk), chunks_uploaded=len(pieces), gb_uploaded=round(moved / 1e9, 3))
        for name, bins, nbins in (("age", age, nage), ("one_bin", one, 1)):
            res["b_centred_ms_" + name] = timed(lambda: trk.centred(field, t, row, col, bins, nbins, hy, hx))
        res["b_stream_times"] = {k: round(v, 2) for k, v in trk.stream_times().items()}
        _native.check(L.ctk_host_register(trk.handle, field.ctypes.data, field.nbytes))
        flat = field.reshape(-1)

        def floor_copies():
            at = 0
            for nt, r in pieces:
                n = nt * r * nx
                trk.h2d(d_flag, flat[at:at + n])
                at += n

        def whole():
            for t0 in range(0, T, chunk):
                trk.h2d(d_flag, field[t0:t0 + chunk])
        res["b_pinned_copies_of_the_bands_ms"] = timed(floor_copies)
        res["b_pinned_copies_of_the_slab_ms"] = timed(whole)
        _native.check(L.ctk_host_unregister(trk.handle, field.ctypes.data))
        res["b_centred_over_band_copies"] = round(res["b_centred_ms_one_bin"] / max(res["b_pinned_copies_of_the_bands_ms"], 1e-3), 3)
        # (c) the field resident: the anomaly of the slab against a one-group climatology stays in HBM
        anom, _ = trk.anomalies(field, np.zeros(T, np.int32), 1, keep_resident=True)
        s_res, n_res = trk.centred(None, t, row, col, age, nage, hy, hx)
        s_two, n_two = trk.centred(anom, t, row, col, age, nage, hy, hx)
        res["c_identical"] = bool(np.array_equal(n_res, n_two) and np.array_equal(s_res.view(np.uint64), s_two.view(np.uint64)))
        res["c_resident_ms_age"] = timed(lambda: trk.centred(None, t, row, col, age, nage, hy, hx))
        res["c_resident_ms_one_bin"] = timed(lambda: trk.centred(None, t, row, col, one, 1, hy, hx))
        res["c_host_array_ms_age"] = timed(lambda: trk.centred(anom, t, row, col, age, nage, hy, hx))
        print(json.dumps(res), flush=True)
    finally:
        trk.debug_set_centred(-1, -1, -1)
        for p in bufs:
            trk.free(p)


with _native.Tracker(0) as trk:
    for shape in shapes:
        probe(trk, *shape)
