"""Blocked spells per grid point (ctk_spells*, k_spell) on a realistic flag: the flag that track_dev makes of a device-generated
synth_fill slab (the bench's workload: threshold 160 '>=', overlap 0.5, persistence 5 at 1 deg / 20 at 0.25 deg).  Everything in one
process, best of REPS, so that every figure has its yardstick from the same session.

Per shape (SHAPES="T,ny,nx;...", default 2707 x 181 x 360 and 480 x 721 x 1440), daily steps from 1979-01-01:
  (a) k_spell alone (HIP events, ctk_debug_time_spell) with the library's slice rule, ungrouped and by month, by_id 1 and 0; k_freq on
      the same buffer (ctk_debug_time_freq); load16: a plain 16-byte load stream over the same bytes (ctk_debug_stream_ceiling);
  (b) the slice sweep: k_spell at every slice of SLICES, and the share of spells that cross a slice end at each (counted on the host
      from the flag: a spell with onset t and duration d crosses when (t % slice) + d > slice);
  (c) host arrays (slabs up to HOST_MAX_GB): ctk_spells and ctk_frequency on the host array at the default chunk, and plain copies of
      the same bytes from pinned (registered) host memory in the same chunks -- the floor; the spell maps are compared with a numpy
      run-length count on the same array.
One JSON line per shape.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/spell_probe.py` for the kernel statistics."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from contrack_amd import _native                       # noqa: E402
from contrack_amd.contrack import row_weights           # noqa: E402

REPS = int(os.environ.get("REPS", "5"))
SLICES = [int(v) for v in os.environ.get("SLICES", "4,8,16,32,64,128,256").split(",") if v]
HOST_MAX_GB = float(os.environ.get("HOST_MAX_GB", "4"))


def timed(fn, reps):
    fn()                                                                       # warm-up: code objects, allocations, pinned buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(min(ms), 3)


def spell_table(flag):
    """(pixel, onset step, duration) of every spell of the slab under by_id: run boundaries along time with numpy"""
    T = flag.shape[0]
    f = flag.reshape(T, -1)
    on = f > 0
    start = on.copy()
    start[1:] &= f[1:] != f[:-1]                                               # flagged and not the id of the step before
    end = on.copy()
    end[:-1] &= f[:-1] != f[1:]
    pix, t0 = np.nonzero(start.T)                                              # pixel-major: the k-th start of a pixel meets its k-th end
    pix1, t1 = np.nonzero(end.T)
    assert np.array_equal(pix, pix1)
    return pix, t0, t1 - t0 + 1


def maps_numpy(shape, pix, d):
    npix = shape[1] * shape[2]
    ev = np.bincount(pix, minlength=npix)
    st = np.bincount(pix, weights=d, minlength=npix).astype(np.int64)
    lg = np.zeros(npix, dtype=np.int64)
    np.maximum.at(lg, pix, d)
    return tuple(a.reshape(shape[1:]) for a in (ev, st, lg))


def main():
    L = _native.lib()
    shapes = [tuple(int(v) for v in s.split(",")) for s in os.environ.get("SHAPES", "2707,181,360;480,721,1440").split(";")]
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
        d_maps = trk.malloc(3 * 12 * npix * 4)
        out = dict(shape=[T, ny, nx], reps=REPS, n_tracked=n_tracked, flagged_fraction=round(nonzero / (T * npix), 5), gb=round(nb / 1e9, 3))
        tbs = lambda ms: round(nb / (ms * 1e-3) / 1e12, 3)
        # (a) the kernels alone, the library's rules
        out["load16_ms"] = round(trk.stream_ceiling(d_flag, nb, 0, reps=REPS), 4)
        out["load16_tbs"] = tbs(out["load16_ms"])
        for gname, grp in (("all", None), ("month", month)):
            best, _ = trk.time_freq(d_flag, T, ny, nx, d_maps, group=grp, ngroups=None if grp is None else 12, reps=REPS)
            out["k_freq_%s_ms" % gname] = round(best, 4)
            for by_id in (1, 0):
                best, _ = trk.time_spells(d_flag, T, ny, nx, d_maps, group=grp, ngroups=None if grp is None else 12, by_id=by_id, reps=REPS)
                out["k_spell_%s_by%d_ms" % (gname, by_id)] = round(best, 4)
        out["k_spell_ms"] = out["k_spell_all_by1_ms"]
        out["k_spell_tbs"] = tbs(out["k_spell_ms"])
        out["k_spell_over_k_freq"] = round(out["k_spell_ms"] / out["k_freq_all_ms"], 3)
        out["k_spell_over_load16"] = round(out["k_spell_ms"] / out["load16_ms"], 3)
        # (b) the slice sweep
        sweep = {}
        for sl in SLICES:
            trk.set_spell_debug(sl)
            best, mean = trk.time_spells(d_flag, T, ny, nx, d_maps, reps=REPS)
            sweep["s%d" % sl] = dict(best_ms=round(best, 4), mean_ms=round(mean, 4))
        trk.set_spell_debug(0)
        out["slice_sweep"] = sweep
        out["dev_call_ms"] = timed(lambda: trk.spells_dev(d_flag, T, ny, nx), REPS)
        trk.free(d_in)
        if nb <= HOST_MAX_GB * 1e9:
            flag = np.empty((T, ny, nx), dtype=np.int32)
            trk.d2h(flag, d_flag)
            pix, t0, d = spell_table(flag)
            out["spells"] = int(t0.size)
            out["mean_duration"] = round(float(d.mean()), 3) if d.size else None
            for sl in SLICES:
                sweep["s%d" % sl]["crossing_share"] = round(float(np.mean((t0 % sl) + d > sl)), 4) if d.size else 0.0
            # (c) host arrays, streamed
            chunk = max(1, min(T, (256 << 20) // (npix * 4)))
            out["chunk_steps"] = chunk
            got = trk.spells(flag)
            out["host_spells_ms"] = timed(lambda: trk.spells(flag), REPS)
            out["host_spells_input_phase_ms"] = round(trk.stream_times()["input_phase"], 3)
            out["host_frequency_ms"] = timed(lambda: trk.frequency(flag), REPS)
            out["host_spells_month_ms"] = timed(lambda: trk.spells(flag, month, 12), REPS)
            out["host_frequency_month_ms"] = timed(lambda: trk.frequency(flag, month, 12), REPS)
            _native.check(L.ctk_host_register(trk.handle, flag.ctypes.data, flag.nbytes))

            def floor():
                for c0 in range(0, T, chunk):
                    trk.h2d(d_flag, flag[c0:c0 + chunk])
            out["pinned_copies_ms"] = timed(floor, REPS)
            _native.check(L.ctk_host_unregister(trk.handle, flag.ctypes.data))
            out["host_spells_over_frequency"] = round(out["host_spells_ms"] / out["host_frequency_ms"], 3)
            out["host_spells_over_copies"] = round(out["host_spells_ms"] / out["pinned_copies_ms"], 3)
            want = maps_numpy(flag.shape, pix, d)
            out["host_equal_numpy"] = bool(all(np.array_equal(g[0], w_) for g, w_ in zip(got, want)))
            del flag
        print(json.dumps(out), flush=True)
        trk.free(d_maps)
        trk.free(d_flag)
        trk.close()


if __name__ == "__main__":
    main()
