"""The slabs of tests/test_gpu_tail_forms.py have the run, id and pass counts they claim, and together with the large shapes of
tests/test_gpu_tail_forms_large.py they reach every filter, rank, extent, run-value, write and count form on both sides of every
branch the selection lets a slab reach (tests/tail_forms.py restates the selection in ctk_forms.h and the kernels' edges, and
is compared here with what the library itself decides: ctk_debug_forms).  No GPU needed."""
import numpy as np
import pytest
from scipy import ndimage

import cpu_tables
import tail_forms as tf


def test_restatement_edges():
    # rows per chunk: 1 deg, 0.25 deg, a wide row, tall chunks of long slabs, the 2^24 workgroup cap
    assert tf.relabel_rows(6, 181, 360) == 11 and tf.relabel_rows(6, 721, 1440) == 2 and tf.relabel_rows(6, 19, 4608) == 1
    assert tf.relabel_rows(14600, 721, 1440) == 6 and tf.relabel_rows(438000, 192, 288) == 96
    assert tf.relabel_rows(1 << 24, 4, 4) == 4 and tf.relabel_rows(1 << 24, 8, 1024) == 8
    # k_relabel_v5 at 1 deg in one 20 KB image; k_relabel_v4 once a one-row image no longer fits 20 KB
    f = tf.write_form(6, 181, 360)
    assert (f["kernel"], f["rb"], f["sub"], f["kb"], f["batched"]) == (5, 11, 11, 20, True)
    assert tf.write_form(6, 19, 4416)["kernel"] == 5 and tf.write_form(6, 19, 4480)["kernel"] == 4
    # 14 600 x 721 x 1440: 6-row chunks in two 24 KB images, three loops of table loads; 438 000 x 192 x 288: 96 rows in 6 images of 20 KB
    f = tf.write_form(14600, 721, 1440)
    assert (f["kernel"], f["rb"], f["sub"], f["kb"], f["batched"]) == (5, 6, 3, 24, False)
    f = tf.write_form(438000, 192, 288)
    assert (f["kernel"], f["rb"], f["kb"]) == (5, 96, 20) and (f["rb"] + f["sub"] - 1) // f["sub"] > 2
    # the generic kernel: rows that are no multiple of four pixels, a misaligned flag, 2^24 workgroups
    assert tf.write_form(6, 21, 362)["kernel"] == 0 and tf.write_form(6, 181, 360, aligned=False)["kernel"] == 0
    assert tf.write_form(1 << 24, 4, 4)["kernel"] == 0 and tf.write_form((1 << 24) - 1, 4, 4)["kernel"] == 5
    # ... which no shard reaches: within MAX_SHARD_T steps the rows rule keeps every launch below 2^24 workgroups
    for ny, nx in ((1, 4), (4, 4), (64, 4), (721, 1440), (65535, 4)):
        rb = tf.relabel_rows(tf.MAX_SHARD_T, ny, nx)
        assert tf.MAX_SHARD_T * ((ny + rb - 1) // rb) < (1 << 24)
    # tab_batched splits at 200 000 workgroups: a stream block of 200 000 one-chunk steps loads in three loops, the rest batched
    assert [tf.write_form(262144, 4, 4, nt=nt)["batched"] for _, nt in tf.stream_blocks(262144, 200000)] == [False, True]
    assert tf.relabel_shape([tf.write_form(262144, 4, 4, nt=nt) for _, nt in tf.stream_blocks(262144, 200000)]) == \
        (4 << 24) | (4 << 8) | tf.R_BATCHED | tf.R_LOOPS | tf.R_KB20
    # the chunk copy: fast path and at most 1024 chunks a step
    assert tf.chunk_copy(6, 181, 360) and not tf.chunk_copy(6, 21, 362) and not tf.chunk_copy(6, 181, 360, aligned=False)
    assert tf.chunk_copy(6, 1024, 4096) and not tf.chunk_copy(6, 1025, 4096)
    # extents, run values, counts
    assert [tf.extent_form(T, nx) for T, nx in ((2048, 360), (2049, 360), (2049, 1024), (2049, 1023))] == [256, 1024, 128, 1024]
    assert tf.extent_form(6, 360, 64) == 64 and tf.extent_form(6, 360, 1024) == tf.EXTENT_BLK
    assert tf.runval_threads(65537, 65537 * 1023, True) == 64 and tf.runval_threads(65537, 65537 * 1024, True) == 256
    assert tf.runval_threads(65536, 10, True) == 256 and tf.runval_threads(65537, 10, False) == 256
    assert [tf.alive_form(4, n, 256) for n in (1024, 1025)] == ["alive:count", "alive:sum"]
    assert [tf.alive_form(4, n, 64) for n in (256, 257)] == ["alive:count", "alive:sum"]
    assert tf.write_count(262144) == tf.W_1 and tf.write_count(262145) == tf.W_FULL
    # filter and rank forms of the fused pass, and how a handle's history moves them
    h = tf.Handle(256)
    assert h.fused(4097, 100) == (tf.F_BLK | tf.F_RANK_MERGED, tf.C_F, 24)
    assert h.fused(4098, 100)[0] == tf.F_2PC | tf.F_RANK_MERGED and h.fused(4098, 100, seg=True)[0] == tf.F_2PC_SEG | tf.F_RANK_MERGED
    assert h.fused(2, 100) == (tf.F_RANK_MERGED, tf.C_F, 0) and h.unite_needed(2) and not h.unite_needed(3)
    assert h.fused(8, tf.RANK_EDGE)[0] == tf.F_BLK | tf.F_RANK_MERGED and h.fused(8, tf.RANK_EDGE + 1)[0] == tf.F_BLK | tf.F_RANK_SPLIT
    h.after(dict(fused_pass=0, off_fused_path_reason=64, filter_passes=35, labels_3d=70), 24)
    assert h.async_passes == 48 and h.fused(36, 100) == (tf.F_PASS | tf.F_RANK_MERGED, tf.C_1, 48) and h.unite_needed(36)
    h.after(dict(fused_pass=1, off_fused_path_reason=0, filter_passes=35, labels_3d=2000000), 48)
    assert h.async_passes == 37 and h.fused(36, 100) == (tf.F_PASS | tf.F_RANK_MERGED, tf.C_FULL, 37)
    h.after(dict(fused_pass=1, off_fused_path_reason=0, filter_passes=3, labels_3d=10), 37)
    assert h.async_passes == 10 and h.fused(36, 100) == (tf.F_BLK | tf.F_RANK_MERGED, tf.C_F, 10)


@pytest.mark.parametrize("case", tf.CASES, ids=lambda c: c["name"])
def test_case_reaches_its_forms(case):
    m = tf.mask_of(case)
    assert m.shape == (case["T"], case["ny"], case["nx"])
    got = tf.case_forms(case, m)
    assert case["reach"] <= got, sorted(case["reach"] - got)
    if "nlab" in case:
        # one-pixel (or two-step) ids that touch nothing else: their count is the number of 3-D components of the mask with
        # 8-connected planes and same-pixel links in time
        st = np.zeros((3, 3, 3), dtype=bool)
        st[1] = True
        st[0, 1, 1] = st[2, 1, 1] = True
        _, n = ndimage.label(m, structure=st)
        assert n == case["nlab"]


@pytest.mark.parametrize("case", [c for c in tf.CASES if c["name"].startswith(("v5_", "v4_"))], ids=lambda c: c["name"])
def test_chunk_edges(case, oracle_lib):
    """every edge of the chunk's run values on both sides, in chunks of both planes; the oracle labels the planes as scipy does"""
    m = tf.mask_of(case)
    rb = tf.relabel_rows(case["T"], case["ny"], case["nx"])
    runs = tf.chunk_runs(m, rb)
    cap = tf.RV5 if case["name"].startswith("v5") else tf.RVCAP
    assert {tf.CTK_CV, tf.CTK_CV + 1, cap, cap + 1} <= set(runs.ravel().tolist())
    for t in (0, 3):
        _, n = oracle_lib.label(m[t:t + 1], 0)
        assert n == ndimage.label(m[t], structure=np.ones((3, 3), dtype=int))[1] > 0
    assert (runs[0] > 0).any() and not m[:, 0].any() and not m[:, -1].any()           # (pole rows empty)


def test_cascade_passes():
    """the numpy Jacobi iteration over cpu_tables' tables needs T - 1 passes for the cascade (T - 2 that remove a bar, one that
    changes nothing): more than the 24 one fused pass launches, fewer than the 48 the next one launches"""
    c = tf.CASE_BY_NAME["cascade"]
    m = tf.mask_of(c).astype(bool)
    tb = cpu_tables.build_tables(m, np.ones(c["ny"], np.int64), np.zeros(c["ny"], np.int64))
    n = tf.jacobi_passes(tb)
    assert n == c["cascade"] == c["T"] - 1 and 24 < n < 48
    # the bars all go, the stubs stay
    assert all(ncomp == (2 if t else 1) for t, ncomp in enumerate(tb["ncomp"]))


def test_jacobi_restatement_on_a_short_cascade():
    """five steps: X_1, X_2, X_3 removed in passes 1, 2, 3; pass 4 changes nothing"""
    m = tf.cascade_slab(5).astype(bool)
    tb = cpu_tables.build_tables(m, np.ones(m.shape[1], np.int64), np.zeros(m.shape[1], np.int64))
    assert tf.jacobi_passes(tb) == 4
    assert tf.jacobi_passes(tb, seg_edge=np.array([0, 0, 1, 0, 0])) == 2            # a segment edge at step 2 stops the cascade


@pytest.mark.parametrize("name", sorted(tf.LARGE))
def test_large_shape_reaches_its_forms(name):
    want = tf.LARGE[name][3]
    got = tf.large_forms(name)
    assert want <= got, sorted(want - got)


def test_filter_edges():
    """the filter-edge slab has the component and pair counts it claims at every edge timestep, and its bars are removed by the
    sequential filter (their backward overlap with the live dots is 1/3)"""
    c = tf.CASE_BY_NAME["filter_edges"]
    m = tf.mask_of(c).astype(bool)
    tb = cpu_tables.build_tables(m, np.ones(c["ny"], np.int64), np.zeros(c["ny"], np.int64))
    npairs = np.bincount([p[0] for p in tb["pairs"]], minlength=c["T"])
    for t, nb, nc in tf.FILTER_EDGES:
        assert tb["ncomp"][t - 1] == nb and tb["ncomp"][t] == nc and npairs[t] == nc
    assert tf.jacobi_passes(tb) >= 2


def test_cases_reach_every_form():
    """the forms the cases are meant to reach (each checked against the restatement above) cover every encoding of the statistics
    and every kernel edge of the restatement"""
    got = set()
    for c in tf.CASES:
        got |= c["reach"]
    for v in tf.LARGE.values():
        got |= v[3]
    assert got == set(tf.FORMS), (sorted(set(tf.FORMS) - got), sorted(got - set(tf.FORMS)))


# ---- the restatement against the library's own rules (contrack_amd/csrc/ctk_forms.h, through ctk_debug_forms) -------------------
BASELINE_SHAPES = [(90, 181, 360), (2707, 181, 360), (480, 721, 1440), (14600, 721, 1440), (7300, 721, 1440), (58400, 721, 1440),
                   (438000, 192, 288), (54750, 192, 288)]


def _write_shapes():
    out = BASELINE_SHAPES + [(c["T"], c["ny"], c["nx"]) for c in tf.CASES] + [v[:3] for v in tf.LARGE.values()]
    out += [(6, 19, 4416), (6, 19, 4480), (6, 19, 4608), (6, 21, 362), (6, 1024, 4096), (6, 1025, 4096), (6, 65535, 4), (tf.MAX_SHARD_T, 65, 4)]
    # the rows loop: launches of 130 000 / 130 001 workgroups before and after a step of rb, and its 2^24 cap
    for ny, nx in ((721, 1440), (181, 360), (192, 288), (64, 4)):
        for rb in range(1, 13):
            nchunk = (ny + rb - 1) // rb
            out += [(130000 // nchunk + d, ny, nx) for d in (0, 1)]
    out += [((1 << 24) + d, ny, nx) for d in (-1, 0) for ny, nx in ((4, 4), (8, 1024), (1, 4))]
    out += [((1 << 24) // 2 + d, 8, 4) for d in (-1, 0, 1)]
    return sorted(set(out))


def test_write_plan_agrees_with_the_library():
    from contrack_amd import _native
    kernels = set()
    for T, ny, nx in _write_shapes():
        W = (nx + 63) // 64
        for aligned in (True, False):
            whole = tf.write_form(T, ny, nx, aligned)
            nchunk = (ny + whole["rb"] - 1) // whole["rb"]
            # the whole shard, stream blocks on both sides of tab_batched's 200 000 workgroups, an empty block
            for nt in sorted({T, min(T, 1), 0, min(T, 199999 // nchunk + 1), min(T, 199999 // nchunk + 2)}):
                f = tf.write_form(T, ny, nx, aligned, nt=nt)
                p = _native.forms(T, ny, nx, nt=nt, aligned16=aligned)
                key = (T, ny, nx, aligned, nt)
                assert p["write_rb"] == f["rb"] == tf.relabel_rows(T, ny, nx), key
                assert p["write_kernel"] == (-1 if f["kernel"] is None else f["kernel"]), key
                assert p["write_shape"] == tf.relabel_shape([f]), key
                assert bool(p["chunk_copy"]) == tf.chunk_copy(T, ny, nx, aligned), key
                if f["kernel"] == 5:
                    assert (p["write_sub"], p["write_kb"], bool(p["write_batched"])) == (f["sub"], f["kb"], f["batched"]), key
                    assert p["write_lds"] == tf._tables(f["rb"], W) + tf._a16(tf.RV5 * 4) + 16 + f["sub"] * nx * 4 <= f["kb"] * 1024, key
                if f["kernel"] == 4:
                    assert p["write_lds"] == tf._tables(f["rb"], W) + tf.RVCAP * 4, key
                if f["kernel"] in (4, 5):
                    assert p["write_grid"] == nt * nchunk, key
                kernels.add(f["kernel"])
    assert kernels == {5, 4, 0, None}


def test_small_kernel_rules_agree_with_the_library():
    from contrack_amd import _native
    for T in (6, 2048, 2049, 65536, 65537):
        for nx in (360, 1023, 1024, 1440):
            for forced in (0, 64, 128, 256, 1024):
                assert _native.forms(T, 8, nx, forced_extent=forced)["extent_form"] == tf.extent_form(T, nx, forced), (T, nx, forced)
        for per in (1, 1023, 1024):
            for path in (0, 1, 2):                                       # staged, fused, time-sharded
                for forced in (0, 64, 128, 256):
                    p = _native.forms(T, 8, 64, total_runs=T * per, path=path, forced_run_values=forced, forced_compact_init=forced)
                    assert p["runval_threads"] == tf.runval_threads(T, T * per, path == 1, forced), (T, per, path, forced)
                    # k_compact_init: a rule and the override in the fused pass only
                    assert p["compact_init_threads"] == ((forced or (64 if T > 65536 else 256)) if path == 1 else 256), (T, path, forced)
    for n in (0, 262144, 262145):
        assert _native.forms(6, 8, 64, n_labels=n)["count_staged"] == tf.write_count(n)


def test_fused_filter_plan_agrees_with_the_library():
    from contrack_amd import _native
    n = 0
    for T in (1, 2, 3, 36, 4096, 4097, 4098, 1665, 1666):
        for passes in (1, 2, 10, 24, 25, 32, 33, 48, 240, 300):
            for last_nlab in (0, 1000000, 1000001):
                for runs in (0, 100, tf.RANK_EDGE, tf.RANK_EDGE + 1):
                    for n_cus in (104, 256):
                        for seg in (False, True):
                            for pslot in (0, 128):
                                h = tf.Handle(n_cus)
                                h.async_passes, h.last_nlab = passes, last_nlab
                                bits, cnt, NP = h.fused(T, runs, seg)
                                p = _native.forms(T, 8, 64, async_passes=passes, last_nlab=last_nlab, total_runs=runs, n_cus=n_cus, seg=seg, pslot=pslot)
                                key = (T, passes, last_nlab, runs, n_cus, seg, pslot)
                                unite = 0 if not h.unite_needed(T) else (tf.F_UNITE_SLOTS if pslot else tf.F_UNITE)
                                assert p["filter_bits"] == bits | unite | (NP << 16), key
                                assert (p["filter_passes"], p["count_fused"]) == (NP, cnt), key
                                assert p["filter_unite"] == {0: 0, tf.F_UNITE_SLOTS: 1, tf.F_UNITE: 2}[unite], key
                                assert p["filter_bits_sync"] == ((tf.F_SYNC_SEG if seg else tf.F_SYNC) if T > 2 else 0) | tf.F_UNITE, key
                                n += 1
    assert n > 8000
    # a handle whose wait once gave up launches one kernel per pass; a round of the time-sharded path has the same two edges
    assert _native.forms(36, 8, 64, no_sys=1)["filter_bits"] & tf.F_PASS and not _native.forms(36, 8, 64, no_sys=1)["filter_sys"]
    for T, want in ((4096, 0), (4097, 1)):
        p = _native.forms(T, 8, 64, async_passes=24, n_cus=256)
        assert (p["round_blk"], p["round_two_pc"], p["round_nb"]) == (1, want, (T + tf.PB_G - 1) // tf.PB_G)
    assert not _native.forms(4096, 8, 64, async_passes=25)["round_blk"] and not _native.forms(4096, 8, 64, no_sys=1)["round_blk"]
