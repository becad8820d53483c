// ctk_forms.h -- which kernel instance a launch takes, with how many threads, how much LDS and how many rows per chunk: every such
// rule of the pass once, as a pure function of the numbers it depends on (internal).
//
// Host only: no HIP, no ctk_handle, no heap, no statics.  The launch functions of ctk_api.hip / ctk_sharded.hip ask here, map the
// answer to the template instance with one switch and write the CTK_S_* statistic from the same value; ctk_debug_forms
// (include/contrack_hip_debug.h) returns the same answers to the tests without a device.  The constants the rules share with the
// kernels (CTK_RB, RC_ROWS, CTK_LDS_RUNS, CTK_LDS_NY, CTK_CV_MAXCHUNK, EX_TW, PB_G, CTK_RL_BLOCKS, CTK_MAX_JACOBI) are in ctk_device.h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include "ctk_device.h"

// the path a launch belongs to: the staged entries (ctk_shard_*, also the synchronous resolution of a one-call track), the fused
// one-call pass (resolve_async), the time-sharded path (ctk_track_sharded_*)
enum CtkPath { CTK_PATH_STAGED = 0, CTK_PATH_FUSED = 1, CTK_PATH_SHARDED = 2 };

// 4 waves per 256-thread workgroup, one row per wave; >> 256 CUs, grid-stride over the rest
inline int ctk_grid_for_rows(int64_t nrows) { return (int)std::min<int64_t>(std::max<int64_t>((nrows + 3) / 4, 1), 256 * 16); }

// ------------------------------------------------------------------------------------------------
// threshold
// ------------------------------------------------------------------------------------------------
enum CtkThrKind {
    CTK_THR_V7 = 0,          // k_threshold_v7<OP, U> (k_threshold_probe<OP, U> in the mask placement check)
    CTK_THR_V6,              // k_threshold_v6<OP, 8>
    CTK_THR_F32,             // k_threshold<OP, float>
    CTK_THR_F64,             // k_threshold<OP, double>
    CTK_THR_FIELD_VEC,       // k_threshold_field<OP, 4>
    CTK_THR_FIELD_GEN        // k_threshold_field_g<OP, slab type, field type>
};
#define CTK_THR_XCD_TILE 64  // chunk -> XCD tiles of 64 (xcd_chunk; NOTES round 4)
struct CtkThrForm {
    int kind;
    int u7;                  // V7: loads per lane and step (4 .. 8)
    int rbt;                 // V7 / FIELD_VEC: rows per workgroup
    int r6, nchunk_t;        // V6: rows per chunk, chunks per timestep
    int64_t nchunks;         // V6: chunks of the launch
    unsigned grid;
};
// timesteps [t0, t0 + nt) of a slab; aligned16: the address of its first step is a multiple of 16 bytes; field: the compare
// value is the threshold field (its own kernels)
inline CtkThrForm ctk_threshold_form(int64_t nt, int ny, int nx, int W, bool f64, bool aligned16, bool field)
{
    CtkThrForm f = {};
    // rows per workgroup of the float4 kernels (swept on their first form, k_threshold_v4, on MI355X: 2707 x 181 x 360: 8..64
    // rows 0.128-0.137 ms (4 rows 0.195); 480 x 721 x 1440: 2..32 rows 0.345-0.366 ms -- flat, 16 it is)
    f.rbt = std::min(ny, CTK_RB);
    const int64_t nblk4 = nt * ((ny + f.rbt - 1) / f.rbt);                             // one workgroup per (timestep, rbt rows)
    const bool v4 = !f64 && (nx % 4 == 0) && aligned16 && nblk4 < (1 << 24);           // < 2^32 work-items
    f.u7 = 8;
    f.r6 = std::max(1, 64 / W); f.nchunk_t = (ny + f.r6 - 1) / f.r6;
    f.nchunks = nt * f.nchunk_t;
    f.grid = (unsigned)ctk_grid_for_rows(nt * ny);
    if (field) { f.kind = v4 ? CTK_THR_FIELD_VEC : CTK_THR_FIELD_GEN; if (v4) f.grid = (unsigned)nblk4; return f; }
    if (!f64 && W <= 64 && !v4) {        // ballot form: float32, rows of at most 64 words, where the float4 form does not apply
        f.kind = CTK_THR_V6;
        f.grid = (unsigned)std::min<int64_t>((f.nchunks + 3) / 4, 16384);
    } else if (f64) f.kind = CTK_THR_F64;
    else if (!v4) f.kind = CTK_THR_F32;
    else {
        f.kind = CTK_THR_V7;
        f.grid = (unsigned)nblk4;
        // loads per lane and step such that the steps of a full chunk carry the fewest idle loads
        const int L = (f.rbt * W * 16 + 255) / 256;
        int best = 1 << 30;
        for (int u = 8; u >= 4; u--) { const int waste = (L + u - 1) / u * u - L; if (waste < best) { best = waste; f.u7 = u; } }
    }
    return f;
}

// ------------------------------------------------------------------------------------------------
// row count
// ------------------------------------------------------------------------------------------------
// one workgroup per timestep: few timesteps of a tall grid leave the chip empty and the rows of a plane in a long chain
// (480 x 721 x 1440: 52 us with 4 waves per plane) -- more waves per plane then (first form of the kernel only)
// (71 VGPRs: three 512-thread workgroups per CU, one round for <= 768 planes; 1024 threads ran in two rounds)
// (throughput regime, small planes -- 438 000 x 192 x 288: 128 threads 1.39 -> 0.86 ms, 64: 1.02)
inline int ctk_rowcount_threads(int64_t T, int ny, int W)
{
    return (W <= 64 && ny <= RC_ROWS && ny > 256 && T <= 2048) ? 512 : ((T > 65536 && (int64_t)ny * W <= 2048) ? 128 : 256);
}
// row groups k_rowcount's first form keeps in flight (its instance k_rowcount<RCU>): as many as the plane needs in ONE step of its waves,
// of 4 / 6 / 8 -- 181 x 360 with 256 threads: ten rows a wave and group, five groups, RCU = 6, 60 VGPRs instead of the 73 of RCU = 8:
// eight workgroups per CU, what the kernel's SGPR limit was set for, instead of six; k_rowcount 14.3 -> 12.1 us at 2707 x 181 x 360 (NOTES).
// (The other forms do not use it.)
inline int ctk_rowcount_groups(int threads, int ny, int W)
{
    if (W > 64) return 8;
    const int per_group = (threads / 64) * (64 / W), need = (ny + per_group - 1) / per_group;
    return need <= 4 ? 4 : need <= 6 ? 6 : 8;
}
// the plane takes k_rowcount's first form, the only one that reads RCU (the kernel's own guard)
inline bool ctk_rowcount_first_form(int ny, int W) { return W <= 64 && ny <= RC_ROWS; }

// ------------------------------------------------------------------------------------------------
// 2-D labelling.  The variants take disjoint sets of timesteps (by run count; nruns == 0 goes to the small one).
// ------------------------------------------------------------------------------------------------
// runs the k_label2d_lds instances carry (their RUNS / RUNS_BELOW template arguments at the launch)
#define CTK_LBL_V0B_RUNS 768
#define CTK_LBL_V0_RUNS 832
#define CTK_LBL_V1_RUNS 1024
#define CTK_LBL_V2_RUNS 2048
struct CtkVariantSet { bool v1, v2, v3, glb, one, v1hi; };
inline bool ctk_variants_any(const CtkVariantSet &v) { return v.v1 || v.v2 || v.v3 || v.glb || v.one || v.v1hi; }
struct CtkLabelShape {
    // (v1hi: small planes in long shards are labelled by the 20 KB variant, which carries 832 runs -- the planes with 833 .. 1024 runs
    // then need the 1024-run variant behind it; v0_ok depends on the shape alone, so a speculative launch and the later check agree)
    // (round 6: the same for planes of 961 .. 1088 words -- 181 x 360 -- with 768 runs and 20.3 KB: eight workgroups per CU instead of the six
    // of the 25.6 KB variant, k_label2d 52.5 -> 49 us at 2707 x 181 x 360)
    bool v0b, v0_ok;
    uint32_t v0_runs;
};
inline CtkLabelShape ctk_label_shape(int64_t T, int ny, int W)
{
    CtkLabelShape s;
    s.v0b = ny <= 256 && (int64_t)ny * W > 960 && (int64_t)ny * W <= 1088;
    s.v0_ok = (T > 65536 && ny <= 256 && (int64_t)ny * W <= 960) || s.v0b;
    s.v0_runs = s.v0b ? CTK_LBL_V0B_RUNS : CTK_LBL_V0_RUNS;
    return s;
}
// planes no LDS variant takes
inline bool ctk_label_need_glb(uint32_t max_runs_step, int ny) { return max_runs_step > CTK_LDS_RUNS || ny > CTK_LDS_NY; }
// what the speculative launch takes from the set the previous call left
inline CtkVariantSet ctk_label_speculative(const CtkVariantSet &spec_set, const CtkLabelShape &sh)
{
    CtkVariantSet v = spec_set;
    v.v1hi = spec_set.v1hi && sh.v0_ok;
    return v;
}
// CTK_S_LABEL_FORMS bits of one launch of the set (512: a speculative launch ran on too small buffers)
#define CTK_LABEL_DISCARDED 512
inline int64_t ctk_label_form_bits(const CtkVariantSet &vs, const CtkLabelShape &sh)
{
    return (vs.one ? 1 : 0) | (vs.v1 ? (sh.v0b ? 2 : sh.v0_ok ? 4 : 8) : 0) | (vs.v1hi ? (sh.v0b ? 16 : 32) : 0) | (vs.v2 ? 64 : 0) |
           (vs.v3 ? 128 : 0) | (vs.glb ? 256 : 0);
}
struct CtkLabelPlan {
    CtkVariantSet missing;   // to launch now, behind what ran speculatively (`launched`)
    CtkVariantSet next;      // the next call's speculative set
};
// after the run scan.  Few timesteps of a busy grid (T <= 512 workgroups: the chip holds them all at once even at two per CU): ONE
// launch of the largest LDS variant for every timestep instead -- 1024 threads per plane finish a plane sooner than 256 or 512, and
// the fork / join of the side streams (two events, ~20 us of stream time at 480 x 721 x 1440) disappears.
inline CtkLabelPlan ctk_label_plan(int64_t T, int ny, const CtkLabelShape &sh, uint32_t max_runs_step, const CtkVariantSet &launched)
{
    const bool glb = ctk_label_need_glb(max_runs_step, ny);
    const bool v2 = max_runs_step > CTK_LBL_V1_RUNS, v3 = max_runs_step > CTK_LBL_V2_RUNS;
    const bool prefer_one = T <= 512 && max_runs_step > CTK_LBL_V1_RUNS;
    const bool none_lds = !launched.v1 && !launched.v2 && !launched.v3 && !launched.one;
    CtkVariantSet need = {true, v2, v3, glb, false, sh.v0_ok && max_runs_step > sh.v0_runs};
    // (launched.one: the large variant took every timestep it can take)
    if ((prefer_one && none_lds) || launched.one) need = {false, false, false, glb, true, false};
    CtkLabelPlan p;
    p.missing = {need.v1 && !launched.v1, need.v2 && !launched.v2, need.v3 && !launched.v3, need.glb && !launched.glb, need.one && !launched.one,
                 need.v1hi && !launched.v1hi};
    if (prefer_one) p.next = {false, false, false, need.glb, true, need.v1hi};
    else p.next = {true, v2, v3, need.glb, false, need.v1hi};
    return p;
}

// ------------------------------------------------------------------------------------------------
// overlap: k_overlap<OVB, TH, WPE>; the form is its statistic code OVB * 10000 + TH * 10 + WPE (CTK_S_OVERLAP_FORM; + CTK_OVERLAP_SEG for
// the builds that read the segment edge table)
// ------------------------------------------------------------------------------------------------
#define CTK_OVERLAP_CODE(OVB, TH, WPE) ((OVB) * 10000 + (TH) * 10 + (WPE))
#define CTK_OVERLAP_SEG 1000000
// (register budgets that allow more waves per SIMD -- 5, 6, 8 instead of the 3 that 135 VGPRs leave at OVB = 5 -- were
// measured, before and after the kernel's live state was cut from 135 to 117 VGPRs: the spills cost more than the occupancy
// returns -- 39 us at 4 waves per SIMD, 44 at 5, 60 at 6)
// few large planes: more waves per plane (480 x 721 x 1440: 256 threads 60 us, 1024 -- one workgroup per CU at 101 VGPRs,
// two rounds -- 53, 512 -- two per CU, one round -- 49.5)
// many small planes (throughput regime): two waves per plane, ten workgroups per CU at 101 VGPRs -- 438 000 x 192 x 288: 3.95 -> 3.50 ms
// (eight words per thread in one step: 169 VGPRs, 5.5 ms)
// (small planes in long shards: room for five waves per SIMD -- 96 VGPRs, 14 of the 105 in scratch -- 3.49 -> 3.05 ms at 438 000 x 192 x 288;
// at 2707 x 181 x 360 the same costs <5, 256> ten of its 36 us: only here.  <5, 256> itself is NOT one round there: 121 VGPRs hold four
// workgroups on a CU, 1024 planes of the 2707 at a time -- 2.6 rounds of about 11 us behind a 2.5 us launch.  Six workgroups per CU
// -- 79 VGPRs, by handing the words with common pixels to the lanes of their wave -- were built and measured slower, 40.4 us: NOTES,
// "k_overlap: wave-level hand-over"; tools/kernel_resources.py prints what every instance takes)
inline int ctk_overlap_form(int64_t T, int ny, int W)
{
    const int nwords = ny * W, per = (nwords + 255) / 256;                             // words per thread if one step is to cover all
    if (T > 65536 && nwords <= 2048) return CTK_OVERLAP_CODE(4, 128, 5);
    if (T <= 1024 && nwords >= 8192) return CTK_OVERLAP_CODE(4, 512, 1);
    if (per <= 4 || per > 8) return CTK_OVERLAP_CODE(4, 256, 1);
    if (per == 5) return CTK_OVERLAP_CODE(5, 256, 1);
    if (per == 6) return CTK_OVERLAP_CODE(6, 256, 1);
    return CTK_OVERLAP_CODE(8, 256, 1);
}

// ------------------------------------------------------------------------------------------------
// extents: threads of k_extent, or CTK_EXTENT_BLK = k_extent_blk (the value is CTK_S_EXTENT_FORM)
// ------------------------------------------------------------------------------------------------
#define CTK_EXTENT_BLK 1024
// (a timestep has ~40 components: one wave per timestep puts every plane of a long slab on the chip at once -- 11.2 instead of
// 14.0 us at 2707 x 181 x 360, equal at 480 x 721 x 1440; tools/small_probe.py)
// (one wave per plane beyond 2048 planes; two on wide grids, whose complex components are folded row by row: 14 600 x 721 x 1440 0.40 -> 0.26 ms)
// round 6: sixteen timesteps per workgroup, the ids' extents reduced in LDS before they touch memory (k_extent_blk), for shards of
// more than 2048 timesteps on narrow grids (where k_extent ran one wave per plane)
// forced: ctk_debug_set_small_threads' extent (0 = the rule)
inline int ctk_extent_form(int64_t T, int nx, int forced)
{
    if (forced > 0) return forced;                 // (1024 = CTK_EXTENT_BLK)
    if (T > 2048) return nx < 1024 ? CTK_EXTENT_BLK : 128;
    return 256;
}

// ------------------------------------------------------------------------------------------------
// the write pass (k_relabel_v5 / k_relabel_v4 / k_relabel)
// ------------------------------------------------------------------------------------------------
#define CTK_RV5 512          // run values k_relabel_v5 stages in LDS
#define CTK_RVCAP 2048       // ... k_relabel_v4
enum CtkWriteKernel { CTK_WR_NONE = -1, CTK_WR_GENERIC = 0, CTK_WR_V4 = 4, CTK_WR_V5 = 5 };       // (the values of CTK_S_RELABEL_KERNEL)
// rows per chunk (workgroup) of a T-step shard.  k_relabel_v4, measured on MI355X (ms):
//   2707 x 181 x 360:    990 int4 stores per workgroup (11 rows) 0.147 | 720: 0.159 | 1440: 0.168 | 540: 0.182
//   480 x 721 x 1440:    720 (2 rows) 0.337 | 2880 (8 rows) 0.343 | 2160: 0.359 | 1440: 0.366
//   14600 x 721 x 1440:  2880 (8 rows, 1.3 M workgroups) 10.9 | 5760: 11.6 | 1440 (2.6 M): 14.0 | 720 (5.3 M): 17.1
// (k_relabel_v4, round 1; for k_relabel_v5 see the table inside)
inline int ctk_write_rows(int64_t T, int ny, int nx)
{
    const int n4r = std::max(1, nx / 4);
    int rb = std::min(ny, std::max(1, std::min(64, 1024 / n4r)));
    // Rows per chunk at 721 x 1440, ns of kernel time per ROW (round 3, `CTK_RELABEL_ROWS` sweeps):
    //   480 steps: 2 rows 0.98 | 3: 1.06 | 6: 1.10        1000 steps: 2 rows 1.53 | 3: 1.03 | 4: 1.04 | 6: 1.08
    //   2000 steps: 3 rows 1.37 | 4: 1.31 | 6: 1.02 | 8: 1.12 | 12: 1.10        14 600 steps: 6 rows 1.03 | 8: 1.07 | 9: 1.09
    // i.e. the smallest chunk that keeps the launch at or below ~250 000 workgroups, and not more than ~2300 stores (6 rows).
    // Narrow rows (192 x 288, configs[4]: 72 stores per row), 438 000 steps, ms per launch: 32 rows 21.6 | 48: 20.2 | 64: 18.9 | 96: 18.5 | 192: 22.8
    // (round 6 sweep) -- the cap of ~2300 stores was found on 1440-wide rows (360 stores each); up to ~6900 where a row is short.
    const int store_cap = n4r >= 256 ? 2304 : 6912;
    const int rb_max = std::min(ny, std::max(rb, std::min(96, store_cap / n4r)));
    // Round 6, with eight workgroups per CU really there (CTK_SGPR_8WAVES), us per launch: 480 steps 2 rows 371 | 3: 332-349 | 4: 353-367 | 5: 337-345 |
    // 6: 348-353; 1000 steps 3 rows 716-734 | 4: 702-707 | 5: 609-699 | 6: 599-707; 2000 steps 4 rows 1688-1762 | 5: 1518-1553 | 6: 1370-1373
    // -> the smallest chunk that keeps the launch at or below ~130 000 workgroups (it was 250 000).
    while (rb < rb_max && T * ((ny + rb - 1) / rb) > 130000) rb++;
    while (rb < ny && T * ((ny + rb - 1) / rb) >= (1 << 24)) rb++;
    return rb;
}
// LDS bytes of a chunk's tables in the word-sliced write kernels: mask words, word starts, row starts of rb rows
inline size_t ctk_write_tables_lds(int rb, int W)
{
    return (size_t)rb * W * 8 + (((size_t)rb * W * 2 + 7) & ~(size_t)7) + ((((size_t)rb + 1) * 4 + 7) & ~(size_t)7);
}
struct CtkWritePlan {
    int kernel;              // CtkWriteKernel
    int rb;                  // rows per chunk (of the whole shard: the chunk-ordered copy is built for it)
    int sub;                 // V5: rows per LDS image of flag values
    int kb;                  // V5: the LDS budget, KB (20, 24 or 28)
    int tab_batched;
    int64_t nchunk;          // chunks per timestep
    unsigned grid;           // V5 / V4: one workgroup per (timestep, chunk); GENERIC: grid-stride over the rows
    size_t lds;              // dynamic LDS of the launch
    int64_t shape;           // the launch's bits of CTK_S_RELABEL_SHAPE
};
// timesteps [t0, t0 + nt) of a T-step shard; aligned16: of the address these timesteps are written to
inline CtkWritePlan ctk_write_plan(int64_t T, int64_t nt, int ny, int nx, int W, bool aligned16)
{
    CtkWritePlan p = {};
    p.rb = ctk_write_rows(T, ny, nx);
    p.nchunk = (ny + p.rb - 1) / p.rb;
    const int64_t nblk4 = nt * p.nchunk;
    p.tab_batched = nblk4 < 200000 ? 1 : 0;          // (1 deg, 480 x 0.25 deg: -4 %; 14 600 x 0.25 deg: +2.7 % -- NOTES round 4)
    const size_t tables = ctk_write_tables_lds(p.rb, W), lds4 = tables + (size_t)CTK_RVCAP * 4;
    if (!((nx % 4 == 0) && aligned16 && (int64_t)ny * nx < 0x7fffffff && nblk4 < (1 << 24) && nt > 0 && lds4 <= 60 * 1024)) {
        p.kernel = nt > 0 ? CTK_WR_GENERIC : CTK_WR_NONE;
        p.grid = (unsigned)ctk_grid_for_rows(nt * ny);
        return p;
    }
    p.grid = (unsigned)nblk4;
    // word-centric form: the LDS image of `sub` rows of flag values (sub x nx x 4 bytes) leaves eight workgroups per CU; tall
    // chunks (the 8-row chunks of slabs with many timesteps) are written in several passes of `sub` rows
    const size_t tab5 = tables + (((size_t)CTK_RV5 * 4 + 15) & ~(size_t)15) + 16;
    // 20 KB = eight workgroups of 256 threads per CU.  A chunk that needs three or more images at that size gets 24 or 28 KB (six / five
    // workgroups per CU) if that brings it down to two: 14 600 x 721 x 1440 in 6-row chunks (34 KB of values) 11.46 -> 10.55 ms,
    // 2000 steps 1.55 -> 1.47; 32 KB: 14.1 ms (four per CU); 438 000 x 192 x 288 in 96-row chunks: 9 or 6 images, no difference
    auto rows_per_image = [&](int kb) { int q = p.rb; while (q > 1 && tab5 + (size_t)q * nx * 4 > (size_t)kb * 1024) q--; return q; };
    p.kb = 20;
    p.sub = rows_per_image(p.kb);
    if ((p.rb + p.sub - 1) / p.sub > 2)
        for (int kb = 24; kb <= 28; kb += 4) {
            const int s2 = rows_per_image(kb);
            if ((p.rb + s2 - 1) / s2 <= 2) { p.kb = kb; p.sub = s2; break; }
        }
    p.lds = tab5 + (size_t)p.sub * nx * 4;
    if (p.lds <= (size_t)p.kb * 1024) {
        p.kernel = CTK_WR_V5;
        p.shape = ((int64_t)p.rb << 24) | ((int64_t)p.sub << 8) | (p.tab_batched ? 1 : 2) | (4 << (p.kb / 4 - 5));
    } else {
        p.kernel = CTK_WR_V4; p.sub = 0; p.kb = 0;
        p.lds = lds4;
        p.shape = (int64_t)p.rb << 24;
    }
    return p;
}
// k_run_values builds the chunk-ordered copy of the run values when a word-sliced kernel will write the shard
inline bool ctk_write_chunk_copy(const CtkWritePlan &whole_shard) { return whole_shard.kernel >= CTK_WR_V4 && whole_shard.nchunk <= CTK_CV_MAXCHUNK; }

// ------------------------------------------------------------------------------------------------
// the one-workgroup-per-timestep kernels k_run_values and k_compact_init.  forced: ctk_debug_set_small_threads' value (0 = the
// rule); only the fused pass has a rule of its own and takes the override, the staged and the time-sharded path launch 256 threads
// ------------------------------------------------------------------------------------------------
// (one wave per plane in the throughput regime with few runs per plane: 438 000 x 192 x 288 1.19 -> 0.63 ms)
inline int ctk_runval_threads(CtkPath path, int64_t T, uint64_t total_runs, int forced)
{
    if (path != CTK_PATH_FUSED) return 256;
    if (forced > 0) return forced;
    return (T > 65536 && total_runs / (uint64_t)T < 1024) ? 64 : 256;
}
inline int64_t ctk_runval_code(int threads, bool chunk_copy) { return threads * 10 + (chunk_copy ? 1 : 0); }       // CTK_S_RUNVAL_FORM
// (one wave per plane in the throughput regime -- 438 000 x 192 x 288: 0.81 -> 0.55 ms; 256 in the latency regime, NOTES round 4)
inline int ctk_compact_init_threads(CtkPath path, int64_t T, int forced)
{
    if (path != CTK_PATH_FUSED) return 256;
    if (forced > 0) return forced;
    return T > 65536 ? 64 : 256;
}

// ------------------------------------------------------------------------------------------------
// the alive count; the values are the bits of CTK_S_COUNT_FORM
// ------------------------------------------------------------------------------------------------
enum CtkCountForm {
    CTK_COUNT_F = 1,         // fused pass: k_count_alive_f (one round of loads, one barrier: round 6)
    CTK_COUNT_1 = 2,         // fused pass: k_count_alive_1
    CTK_COUNT_FULL = 4,      // fused pass: k_count_alive
    CTK_COUNT_W1 = 8,        // ctk_shard_write: k_count_alive_1
    CTK_COUNT_WFULL = 16     // ctk_shard_write: k_count_alive
};
inline int ctk_count_form_staged(int64_t n_labels) { return n_labels <= 262144 ? CTK_COUNT_W1 : CTK_COUNT_WFULL; }
// last_nlab: the previous pass' id count (a slab of the same kind); passes: the filter passes the fused pass launched.
// k_count_alive_f reads one 'changed' word per pass with its first 32 lanes and DEPENDS on passes <= 32 being checked here and
// nowhere else: it has no clamp of its own.
inline int ctk_count_form_fused(int64_t last_nlab, int passes)
{
    if (last_nlab > 1000000) return CTK_COUNT_FULL;
    return passes <= 32 ? CTK_COUNT_F : CTK_COUNT_1;
}

// ------------------------------------------------------------------------------------------------
// the overlap filter, the 3-D unions behind it and the numbering of the ids; bits of CTK_S_FILTER_FORMS
// ------------------------------------------------------------------------------------------------
#define CTK_PB_MAX_PASSES 24 // iterations one k_rs_pass_blk launch takes
// blocks of 256 components of the rank scan (k_rs_roots / k_rs_rank) over tables of at most R components (components <= runs)
inline int64_t ctk_rank_blocks(size_t R) { return (int64_t)(((R ? R : 1) + 255) / 256); }
enum CtkFilterBits {
    CTK_FF_BLK = 1, CTK_FF_BLK_SEG = 2, CTK_FF_2PC = 4, CTK_FF_2PC_SEG = 8,            // k_rs_pass_blk / k_rs_pass_blk_2pc, fused pass
    CTK_FF_PASS = 16, CTK_FF_PASS_SEG = 32,                                            // k_rs_pass per pass, fused pass
    CTK_FF_SYNC = 64, CTK_FF_SYNC_SEG = 128,                                           // k_rs_pass per pass, synchronous resolver
    CTK_FF_UNITE_SLOTS = 256, CTK_FF_UNITE = 512, CTK_FF_RANK_MERGED = 1024, CTK_FF_RANK_SPLIT = 2048
};
// one round of `npass` passes over `steps` timesteps: all of them in one launch (k_rs_pass_blk) when every workgroup of the launch
// can wait for its predecessor (no_sys: a wait of this handle once gave up), else one launch per pass
struct CtkFilterRound {
    bool blk;
    bool two_pc;             // the build with two workgroups per CU, when the launch is larger than the chip (ctk_resolve_dev.hip)
    int nb;                  // workgroups of the block launch
};
inline CtkFilterRound ctk_filter_round(int64_t steps, int npass, bool no_sys, int n_cus)
{
    CtkFilterRound r;
    r.blk = !no_sys && npass <= CTK_PB_MAX_PASSES;
    r.nb = (int)((steps + PB_G - 1) / PB_G);
    r.two_pc = r.nb > n_cus;
    return r;
}
enum CtkUnite { CTK_UNITE_IN_PASS = 0, CTK_UNITE_SLOTS, CTK_UNITE_PAIRS };              // k_rs_pass_blk itself / k_rs_unite_slots / k_rs_unite
struct CtkFilterPlan {
    bool sys;                // the block launch is allowed (its per-timestep state words are needed)
    int passes;              // NP
    CtkFilterRound round;    // (blk: sys && passes > 0)
    int unite;               // CtkUnite
    bool merged;             // numbering and seam marks in one launch (k_fz_rank_mark), while the block sums fit LDS
    int64_t bits;            // CTK_S_FILTER_FORMS of the pass
};
// the fused pass: async_passes = the passes the handle launches (previous pass' count + 2); pslot: pair-record slots per timestep
// (0: ungrouped records); nsb: blocks of 256 components of the rank scan.  (timesteps 1 .. T-2 are filtered; T-1's wave only unites
// its pairs)
inline CtkFilterPlan ctk_filter_plan_fused(int64_t T, int async_passes, bool no_sys, int n_cus, bool seg, int pslot, int64_t nsb)
{
    CtkFilterPlan p;
    p.sys = !no_sys && async_passes <= CTK_PB_MAX_PASSES;
    p.passes = T > 2 ? std::min(std::max(async_passes, 2), p.sys ? CTK_PB_MAX_PASSES : CTK_MAX_JACOBI) : 0;
    p.round = ctk_filter_round(T - 1, p.passes, no_sys, n_cus);
    p.round.blk = p.sys && p.passes > 0;
    p.unite = p.round.blk ? CTK_UNITE_IN_PASS : (pslot ? CTK_UNITE_SLOTS : CTK_UNITE_PAIRS);
    p.merged = nsb <= CTK_RL_BLOCKS;
    p.bits = 0;
    if (p.round.blk) p.bits |= (p.round.two_pc ? CTK_FF_2PC : CTK_FF_BLK) << (seg ? 1 : 0);
    else if (p.passes > 0) p.bits |= seg ? CTK_FF_PASS_SEG : CTK_FF_PASS;
    if (p.unite == CTK_UNITE_SLOTS) p.bits |= CTK_FF_UNITE_SLOTS;
    if (p.unite == CTK_UNITE_PAIRS) p.bits |= CTK_FF_UNITE;
    p.bits |= (p.merged ? CTK_FF_RANK_MERGED : CTK_FF_RANK_SPLIT) | ((int64_t)p.passes << 16);
    return p;
}
// the synchronous resolver: one launch per pass over timesteps 1 .. T-2, k_rs_unite, split rank
inline int64_t ctk_filter_bits_sync(int64_t T, bool seg) { return (T > 2 ? (seg ? CTK_FF_SYNC_SEG : CTK_FF_SYNC) : 0) | CTK_FF_UNITE; }

// ------------------------------------------------------------------------------------------------
// percentile per group (ctk_pctl.hip): radix selection over all groups at once
// ------------------------------------------------------------------------------------------------
#define CTK_PCTL_BITS 11          // widest digit: 2048 bins, 8 KB of uint32 per histogram
#define CTK_PCTL_BINS (1 << CTK_PCTL_BITS)
#define CTK_PCTL_LDS_SLOTS 4      // histograms a sweep workgroup keeps in LDS (32 KB: 4 workgroups per CU); the distinct prefixes of a
                                  // day beyond them are deep digits, whose few matching values go to HBM one atomic each
#define CTK_PCTL_MAX_WINDOW 1024  // distinct prefixes of a day's targets held in LDS (a window below the group count is at most this)
#define CTK_PCTL_MAX_SLOTS (1ll << 19)   // histograms (groups x distinct prefixes per day) of 8 KB a call may ask for: 4 GB
#define CTK_PCTL_CHUNK 16384      // band values per sweep workgroup (256 lanes x 16 loads of 16 bytes, float32)
struct CtkPctlForm {
    int levels;                   // sweeps that build histograms: 3 for 32-bit keys (11/11/10 bits), 6 for 64-bit (11/11/11/11/10/10)
    int shift[8], bits[8];        // digit of level l: (key >> shift[l]) & ((1 << bits[l]) - 1), most significant first
    int sweeps;                   // band reads of one call: levels + the closing sweep -- independent of the groups and the window
    int stride;                   // histogram slots per day: the distinct prefixes its targets can have (1 when every group pools everything)
    int64_t chunk;
    unsigned chunks;              // workgroups per timestep
};
inline CtkPctlForm ctk_pctl_form(int keybits, int64_t nband, int G, int W)
{
    CtkPctlForm f = {};
    f.levels = (keybits + CTK_PCTL_BITS - 1) / CTK_PCTL_BITS;
    const int base = keybits / f.levels, extra = keybits % f.levels;
    int left = keybits;
    for (int l = 0; l < f.levels; l++) { f.bits[l] = base + (l < extra ? 1 : 0); left -= f.bits[l]; f.shift[l] = left; }
    f.sweeps = f.levels + 1;
    f.stride = W >= G ? 1 : W;
    f.chunk = CTK_PCTL_CHUNK;
    f.chunks = (unsigned)((nband + f.chunk - 1) / f.chunk);
    return f;
}
// per-day histogram counters are uint32: a day's timesteps x band pixels must stay below 2^32
inline bool ctk_pctl_day_fits(int64_t steps_of_day, int64_t nband) { return steps_of_day == 0 || nband <= (int64_t)0xffffffffll / steps_of_day; }
// what ctk_percentile_groups_* refuses by size (pctl_validate and ctk_debug_percentile_groups_plan ask here), first reason met:
// a window below the group count wider than the LDS list of a day's prefixes; more histograms than CTK_PCTL_MAX_SLOTS; more sweep
// workgroups per timestep than gridDim.y holds; a group whose timesteps x band values overflow its uint32 counters
enum CtkPctlRefusal { CTK_PCTL_FINE = 0, CTK_PCTL_REFUSE_WINDOW = 1, CTK_PCTL_REFUSE_SLOTS = 2, CTK_PCTL_REFUSE_BAND = 3, CTK_PCTL_REFUSE_DAY = 4 };
inline int ctk_pctl_refusal(int64_t nband, int G, int W, int64_t max_steps_of_a_group)
{
    if (W < G && W > CTK_PCTL_MAX_WINDOW) return CTK_PCTL_REFUSE_WINDOW;
    const CtkPctlForm f = ctk_pctl_form(32, nband, G, W);
    if ((uint64_t)G * (uint64_t)f.stride > (uint64_t)CTK_PCTL_MAX_SLOTS) return CTK_PCTL_REFUSE_SLOTS;
    if ((nband + CTK_PCTL_CHUNK - 1) / CTK_PCTL_CHUNK > 65535) return CTK_PCTL_REFUSE_BAND;
    if (!ctk_pctl_day_fits(max_steps_of_a_group, nband)) return CTK_PCTL_REFUSE_DAY;
    return CTK_PCTL_FINE;
}

// ------------------------------------------------------------------------------------------------
// percentile field per group and grid point (ctk_pfield.hip): a radix selection per (group, pixel)
// ------------------------------------------------------------------------------------------------
#define CTK_PFIELD_LDS_BYTES 163840   // what a workgroup may declare on gfx950
#define CTK_PFIELD_RING_THREADS 512   // ring form: lanes per pixel = 512 / pixel tile
#define CTK_PFIELD_DIRECT_THREADS 256
#define CTK_PFIELD_DIRECT_TILE 64     // direct form: pixels per workgroup (4 lanes per pixel); k_quantile runs the same tile
#define CTK_PFIELD_MIN_TILE 8         // ring form: the pixel tile is 32, 16 or 8 -- the widest whose ring holds the longest pool
#define CTK_PFIELD_MAX_TILE 32
enum CtkPfieldForm { CTK_PFIELD_DIRECT = 0, CTK_PFIELD_RING = 1 };
// LDS of a selection workgroup beside the ring: 257 uint32 bins per pixel, one partial sum per lane, 64 bytes of rank state per pixel
constexpr int64_t ctk_pfield_select_bytes(int tile, int threads) { return (int64_t)tile * 257 * 4 + (int64_t)threads * 4 + (int64_t)tile * 64; }
// timesteps the ring of a workgroup of `tile` pixels holds
constexpr int64_t ctk_pfield_ring_steps(int keybytes, int tile)
{
    return (CTK_PFIELD_LDS_BYTES - ctk_pfield_select_bytes(tile, CTK_PFIELD_RING_THREADS)) / ((int64_t)tile * keybytes);
}
// the longest pool (in timesteps) the ring form takes: 4 783 for float32, 2 391 for float64
#define CTK_PFIELD_CAP_F32 ctk_pfield_ring_steps(4, CTK_PFIELD_MIN_TILE)
#define CTK_PFIELD_CAP_F64 ctk_pfield_ring_steps(8, CTK_PFIELD_MIN_TILE)
struct CtkPfieldPlan {
    int form;                     // CtkPfieldForm
    int64_t cap;                  // longest pool of the ring form for this key width
    int tile;                     // pixels per workgroup
    int64_t ring_steps, ring_bytes;   // the ring of the chosen tile (0: direct form)
    int planes;                   // planes selected: G, or 1 when the window covers every group (the plane is replicated)
};
// max_pool_steps: the most timesteps any group's window pools
inline CtkPfieldPlan ctk_pfield_plan(int keybytes, int64_t max_pool_steps, int G, int W)
{
    CtkPfieldPlan p = {};
    p.cap = keybytes == 4 ? CTK_PFIELD_CAP_F32 : CTK_PFIELD_CAP_F64;
    p.planes = W >= G ? 1 : G;
    p.form = max_pool_steps <= p.cap ? CTK_PFIELD_RING : CTK_PFIELD_DIRECT;
    p.tile = CTK_PFIELD_DIRECT_TILE;
    if (p.form == CTK_PFIELD_RING) {
        p.tile = CTK_PFIELD_MAX_TILE;
        while (p.tile > CTK_PFIELD_MIN_TILE && ctk_pfield_ring_steps(keybytes, p.tile) < max_pool_steps) p.tile /= 2;
        p.ring_steps = ctk_pfield_ring_steps(keybytes, p.tile);
        p.ring_bytes = p.ring_steps * p.tile * keybytes;
    }
    return p;
}

// ------------------------------------------------------------------------------------------------
// standard-deviation field per group and grid point (ctk_std.hip): k_std_field keeps the accumulators of ALL planes of its pixel tile
// in LDS -- per (plane, pixel) a float64 sum that becomes the mean in place, a float64 sum of squares and, when NaNs are skipped, a
// uint32 count -- beside CTK_STD_STAGE staged timesteps of the tile (reserved at 8 bytes per value for either dtype)
// ------------------------------------------------------------------------------------------------
#define CTK_STD_LDS_BYTES 163840      // what a workgroup may declare on gfx950
#define CTK_STD_THREADS 512           // owners per pixel = 512 / pixel tile: owner s of a pixel holds the planes h with h % owners == s
#define CTK_STD_STAGE 64              // timesteps staged per round
#define CTK_STD_MIN_TILE 8            // the pixel tile is 32, 16 or 8 -- the widest whose accumulators fit
#define CTK_STD_MAX_TILE 32
constexpr int64_t ctk_std_acc_bytes(int skipna) { return 16 + (skipna ? 4 : 0); }
constexpr int64_t ctk_std_stage_bytes(int tile) { return (int64_t)CTK_STD_STAGE * tile * 8; }
// planes a workgroup of `tile` pixels holds
constexpr int64_t ctk_std_planes_max(int tile, int skipna) { return (CTK_STD_LDS_BYTES - ctk_std_stage_bytes(tile)) / ((int64_t)tile * ctk_std_acc_bytes(skipna)); }
struct CtkStdPlan {
    int tile;                     // pixels per workgroup; 0: even CTK_STD_MIN_TILE pixels do not fit
    int planes;                   // planes accumulated: G, or 1 when the window covers every group (the plane is replicated)
    int64_t lds_bytes;            // dynamic LDS of the launch (0 with tile 0)
    int64_t max_groups;           // the most groups a window below the group count may have: 998 with counts, 1 248 without
};
inline CtkStdPlan ctk_std_plan(int G, int W, int skipna)
{
    CtkStdPlan p = {};
    p.planes = W >= G ? 1 : G;
    p.max_groups = ctk_std_planes_max(CTK_STD_MIN_TILE, skipna);
    for (int tile = CTK_STD_MAX_TILE; tile >= CTK_STD_MIN_TILE; tile /= 2)
        if (p.planes <= ctk_std_planes_max(tile, skipna)) {
            p.tile = tile;
            p.lds_bytes = (int64_t)p.planes * tile * ctk_std_acc_bytes(skipna) + ctk_std_stage_bytes(tile);
            break;
        }
    return p;
}

// ------------------------------------------------------------------------------------------------
// run_lifecycle reductions (ctk_lifecycle.hip): the strip form k_life_seam / k_life_strips<VT, VEC> / k_life_finish, and k_lifecycle for
// the time steps the strip form gives up.  (CTK_LIFE_SW and CTK_LIFE_WAVES restate LB_SW and LB_THREADS / 64 of ctk_lifecycle.hip;
// ctk_api.hip asserts that they agree.)
// ------------------------------------------------------------------------------------------------
#define CTK_LIFE_SW 256           // columns per strip: one wave, four per lane
#define CTK_LIFE_WAVES 4          // waves (bands of rw rows) per workgroup
#define CTK_LIFE_KS_MAX 32        // k_lifecycle: column bit sets of seam-crossing ids, at most
#define CTK_LIFE_KS_BYTES 32768   // ... and their dynamic LDS
struct CtkLifePlan {
    int rw;                       // rows per wave of k_life_strips
    int nsx, nby;                 // strips per row, workgroups per strip: nsx * nby workgroups per time step
    int vec;                      // k_life_strips<VT, true>: one 16- / 32-byte request per lane and row
    int ks;                       // seam-crossing ids per pass of k_lifecycle
};
// Rows per wave of k_life_strips: four waves (one workgroup) cover a band of the strip, `g` bands cover the ny rows without idle
// waves at the end (181 rows: 4 x 46; 721 rows: 20 x 37).  Measured (us, 2707 x 181 x 360 | 480 x 721 x 1440): 16 rows 316 | 509,
// 23: 291 | 474, 31: 379 (a quarter of the waves idle) | 441, 37: | 436, 46: 281 | 458, 61: | 433 -- long streams per wave, as long
// as the launch keeps a few thousand workgroups.
inline int ctk_life_rows_per_wave(int64_t T, int ny, int nx)
{
    const int64_t nsx = (nx + CTK_LIFE_SW - 1) / CTK_LIFE_SW;
    int g = std::max(1, (ny + 80) / 160);
    while (T * nsx * g < 2048 && (ny + 4 * g - 1) / (4 * g) > 8) g++;
    return std::max(1, (ny + 4 * g - 1) / (4 * g));
}
// flag_ptr / field_ptr: the device addresses of the two slabs (only their alignment matters: VEC needs nx a multiple of 4, the flags
// on 16 bytes and the field on 16 (float32) or 32 (float64), so that every row of every plane starts on a whole request)
inline CtkLifePlan ctk_life_plan(int64_t T, int ny, int nx, bool f64, uintptr_t flag_ptr, uintptr_t field_ptr)
{
    CtkLifePlan p;
    p.rw = ctk_life_rows_per_wave(T, ny, nx);
    p.nsx = (nx + CTK_LIFE_SW - 1) / CTK_LIFE_SW;
    p.nby = (ny + p.rw * CTK_LIFE_WAVES - 1) / (p.rw * CTK_LIFE_WAVES);
    p.vec = ((nx & 3) == 0 && (flag_ptr & 15u) == 0 && (field_ptr & (f64 ? 31u : 15u)) == 0) ? 1 : 0;
    const int nxw = (nx + 31) / 32;
    p.ks = std::max(1, std::min(CTK_LIFE_KS_MAX, CTK_LIFE_KS_BYTES / (nxw * 4)));
    return p;
}

// ------------------------------------------------------------------------------------------------
// segmented anomalies (ctk_anom_seg.hip): k_anom_ring keeps the last `smooth` raw anomalies of a thread's pixel in LDS while it walks
// its time tile; k_anom_plain re-reads the window from memory for a smoothing whose ring does not fit
// ------------------------------------------------------------------------------------------------
#define CTK_ANOM_THREADS 256
#define CTK_ANOM_RING_BYTES 32768     // ring of a workgroup: five workgroups (20 waves) per CU; float32 smooth <= 32, float64 <= 16
#define CTK_ANOM_TILE_MIN 32          // output steps per workgroup: the ring form reads smooth - 1 halo steps per tile on top of them
#define CTK_ANOM_TILE_MAX 256
#define CTK_ANOM_WAVES 16384          // waves that fill 256 CUs several times over (as k_freq)
enum CtkAnomForm { CTK_ANOM_PLAIN = 0, CTK_ANOM_RING = 1 };
struct CtkAnomPlan {
    int form;                     // CtkAnomForm
    size_t lds;                   // dynamic LDS of the launch (ring form)
    int64_t tile;                 // output steps per workgroup
    unsigned gx, gy;
};
// nt output steps of a plane of npix pixels; waves_wanted: CTK_ANOM_WAVES, grid_y_max: 65535 -- or a test's values, which reach the
// tile edges on small slabs (ctk_debug_set_anom)
inline CtkAnomPlan ctk_anom_plan(int elem_bytes, int smooth, int64_t nt, int64_t npix, int64_t waves_wanted = CTK_ANOM_WAVES, int64_t grid_y_max = 65535)
{
    CtkAnomPlan p = {};
    p.lds = (size_t)smooth * CTK_ANOM_THREADS * (size_t)elem_bytes;
    p.form = p.lds <= CTK_ANOM_RING_BYTES ? CTK_ANOM_RING : CTK_ANOM_PLAIN;
    if (p.form == CTK_ANOM_PLAIN) p.lds = 0;
    const int64_t waves = (npix + 63) / 64;
    // the longest tile that still leaves waves_wanted waves, at least 8 x the halo so that it stays below an eighth of the reads
    int64_t tile = std::max<int64_t>(1, nt * waves / waves_wanted);
    tile = std::min<int64_t>(CTK_ANOM_TILE_MAX, std::max<int64_t>(tile, std::max<int64_t>(CTK_ANOM_TILE_MIN, 8 * (int64_t)(smooth - 1))));
    if (p.form == CTK_ANOM_PLAIN) tile = CTK_ANOM_TILE_MIN;
    tile = std::max(tile, (nt + grid_y_max - 1) / grid_y_max);                         // gridDim.y <= 65535
    p.tile = tile;
    p.gx = (unsigned)((npix + CTK_ANOM_THREADS - 1) / CTK_ANOM_THREADS);
    p.gy = (unsigned)std::max<int64_t>(1, (nt + tile - 1) / tile);
    return p;
}

// ------------------------------------------------------------------------------------------------
// weighted time filter and block means (ctk_filter.hip): k_filter_ring keeps the last K values of a lane's pixel in LDS while it walks
// the steps of its tile of outputs; k_filter_plain reads every tap from memory -- for a K whose ring does not fit, and for
// stride >= K, where no two outputs share a tap.
// The ring of a workgroup is K * threads * elem_bytes.  Its budget stays CTK_ANOM_RING_BYTES: 160 KB of LDS per CU hold five such
// workgroups, which at 256 threads are 20 waves per CU -- the occupancy k_anom_ring runs at.  A longer K takes fewer threads per
// workgroup, 128, then 64 (one wave): 128 float32 / 64 float64 taps.  Five workgroups of one wave are 5 waves per CU; a kernel that long
// is bound by its K LDS reads and float64 additions per output, not by loads in flight, so the lower occupancy costs little there,
// and the plain form it replaces reads x K times.
// ------------------------------------------------------------------------------------------------
#define CTK_FILTER_THREADS 256        // the most threads of a workgroup (the launch bound of both kernels)
#define CTK_FILTER_THREADS_MIN 64
#define CTK_FILTER_RING_BYTES CTK_ANOM_RING_BYTES
#define CTK_FILTER_TILE_MIN 32        // outputs per workgroup: the ring form reads K - stride halo steps per tile on top of tile * stride
#define CTK_FILTER_TILE_MAX 1024      // (K = 121 at stride 1: the halo stays near a tenth of the reads)
#define CTK_FILTER_MAX_TAPS (1 << 20)
enum CtkFilterForm { CTK_FILTER_PLAIN = 0, CTK_FILTER_RING = 1 };
struct CtkTimeFilterPlan {
    int form;                     // CtkFilterForm
    int threads;                  // per workgroup
    size_t lds;                   // dynamic LDS of the launch (ring form)
    int64_t tile;                 // outputs per workgroup
    unsigned gx, gy;
};
// nout outputs of a plane of npix pixels.  waves_test: 0, grid_y_max: 65535, forced: -1 the rule -- or a test's values
// (ctk_debug_set_filter): waves_test > 0 asks for that many waves and drops the rule's shortest tiles, so that a small slab reaches
// a tile of one output and one longer than the slab; forced = CTK_FILTER_PLAIN always holds, forced = CTK_FILTER_RING where a ring fits
inline CtkTimeFilterPlan ctk_filter_plan(int elem_bytes, int64_t K, int64_t stride, int64_t nout, int64_t npix, int64_t waves_test = 0, int64_t grid_y_max = 65535,
                                         int forced = -1)
{
    CtkTimeFilterPlan p = {};
    p.form = CTK_FILTER_PLAIN; p.threads = CTK_FILTER_THREADS;
    int fit = 0;                                                                         // the most threads whose ring fits (0: none)
    for (int th = CTK_FILTER_THREADS; th >= CTK_FILTER_THREADS_MIN && !fit; th /= 2)
        if ((uint64_t)K * (uint64_t)th * (uint64_t)elem_bytes <= CTK_FILTER_RING_BYTES) fit = th;
    if (fit && forced != CTK_FILTER_PLAIN && (stride < K || forced == CTK_FILTER_RING)) {
        p.form = CTK_FILTER_RING; p.threads = fit; p.lds = (size_t)K * (size_t)fit * (size_t)elem_bytes;
    }
    const int64_t waves = (npix + 63) / 64;
    // the longest tile that still leaves waves_wanted waves; the ring form: at least 8 x the halo, so that it stays below an eighth of the reads
    int64_t tile = std::min<int64_t>(CTK_FILTER_TILE_MAX, std::max<int64_t>(1, nout * waves / (waves_test > 0 ? waves_test : CTK_ANOM_WAVES)));
    if (waves_test <= 0) {
        const int64_t halo8 = K > stride ? (8 * (K - stride) + stride - 1) / stride : 0;
        tile = std::min<int64_t>(CTK_FILTER_TILE_MAX, std::max<int64_t>(tile, std::max<int64_t>(CTK_FILTER_TILE_MIN, halo8)));
        if (p.form == CTK_FILTER_PLAIN) tile = CTK_FILTER_TILE_MIN;
    }
    tile = std::max(tile, (nout + grid_y_max - 1) / grid_y_max);                          // gridDim.y <= 65535
    p.tile = tile;
    p.gx = (unsigned)((npix + p.threads - 1) / p.threads);
    p.gy = (unsigned)std::max<int64_t>(1, (nout + tile - 1) / tile);
    return p;
}

// ------------------------------------------------------------------------------------------------
// vertical mean over the selected levels (ctk_level.hip): k_level_mean, one thread per 16 bytes of adjacent pixels of one step (vector
// form: every level plane starts on a 16-byte boundary) or per pixel (scalar form); a workgroup stays inside one step, so the step of a
// workgroup is a scalar and `steps` never sits in a grid dimension that ends at 65 535
// ------------------------------------------------------------------------------------------------
#define CTK_LEVEL_THREADS 256
#define CTK_LEVEL_UNROLL 8            // level planes whose loads of a lane are in flight together (then batches of 4, 2, 1 for the rest)
#define CTK_LEVEL_MAX_SEL 4096        // selected levels of one call (weights and level indices: a device table of 12 bytes each)
#define CTK_LEVEL_GRID_MAX 0xffffffll   // workgroups of a launch: gridDim.x * blockDim.x must stay below 2^32 work-items (as ctk_threshold_form)
#define CTK_LEVEL_XCD_MIN 2048       // workgroups from which each XCD takes one contiguous eighth of the launch (xcd_chunk, ctk_kernels.hip)
struct CtkLevelPlan {
    int vec;                      // 1: 16-byte nontemporal loads and a 16-byte store, 0: the scalar form
    int vpt;                      // pixels per thread: 16 / elem_bytes, or 1
    int unroll;                   // the widest batch of level planes a lane loads before it uses the first
    int64_t bps;                  // workgroups per step
    int64_t blocks;               // bps * steps: (step, part of the plane) pairs, walked by ...
    unsigned grid;                // ... this many workgroups (all of them unless that exceeds what a launch of 256 threads may have)
    int xcd;                      // xcd_chunk mode of the launch: 1 one contiguous eighth of the workgroups per XCD, 0 launch order
};
// `aligned`: the input and output base pointers are multiples of 16; grid_max: CTK_LEVEL_GRID_MAX, or a test's lower cap
inline CtkLevelPlan ctk_level_plan(int elem_bytes, int64_t nsel, int64_t npix, int64_t steps, bool aligned, int64_t grid_max = CTK_LEVEL_GRID_MAX)
{
    CtkLevelPlan p = {};
    p.vec = aligned && (npix * elem_bytes) % 16 == 0;
    p.vpt = p.vec ? 16 / elem_bytes : 1;
    p.unroll = nsel >= CTK_LEVEL_UNROLL ? CTK_LEVEL_UNROLL : nsel >= 4 ? 4 : nsel >= 2 ? 2 : 1;
    const int64_t lanes = (npix + p.vpt - 1) / p.vpt;
    p.bps = (lanes + CTK_LEVEL_THREADS - 1) / CTK_LEVEL_THREADS;
    p.blocks = p.bps * steps;
    p.grid = (unsigned)std::min<int64_t>(p.blocks, std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX));
    p.xcd = p.grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    return p;
}
// the selected levels (weight != 0) of a call in rising order, as runs of neighbours: run r covers levels [l0, l0 + len) of the input
// and places [k0, k0 + len) of the compact chunk (nt, nsel, ny, nx) -- one strided copy each.  runs: room for (nlev + 1) / 2 of them.
struct CtkLevelRun { int64_t l0, k0, len; };
inline int64_t ctk_level_runs(const double *w, int64_t nlev, CtkLevelRun *runs, int64_t *nsel)
{
    int64_t nr = 0, k = 0;
    for (int64_t l = 0; l < nlev; l++) {
        if (w[l] == 0.0) continue;
        if (nr > 0 && runs[nr - 1].l0 + runs[nr - 1].len == l) runs[nr - 1].len++;
        else { runs[nr].l0 = l; runs[nr].k0 = k; runs[nr].len = 1; nr++; }
        k++;
    }
    *nsel = k;
    return nr;
}

// ------------------------------------------------------------------------------------------------
// reversal of the meridional gradient (ctk_reversal.hip): k_reversal, a stencil in latitude -- one thread per 16 bytes of adjacent
// longitudes of one row of one step (vector form: every ROW starts on a 16-byte boundary, so a lane never straddles two rows) or per
// pixel (scalar form: an odd row length, an offset pointer).  A workgroup stays inside one step, as k_level_mean's does.  A row is
// read by its own lanes and by those of up to three other rows of the same plane, 0.26 MB at 1 degree and 4 MB at a quarter degree:
// from CTK_LEVEL_XCD_MIN workgroups on every XCD takes one contiguous eighth of the launch (xcd_chunk), so the rows of a plane meet
// in ONE L2 instead of eight (profiles/NOTES.md, "k_reversal").
// ------------------------------------------------------------------------------------------------
#define CTK_REVERSAL_THREADS 256
struct CtkReversalPlan {
    int vec;                      // 1: 16-byte loads and a 16-byte store per lane, 0: the scalar form
    int vpt;                      // pixels per thread: 16 / elem_bytes, or 1
    int64_t bps;                  // workgroups per step
    int64_t blocks;               // bps * steps: (step, part of the plane) pairs, walked by ...
    unsigned grid;                // ... this many workgroups (CTK_LEVEL_GRID_MAX at most: a launch stays below 2^32 work-items)
    int xcd;                      // xcd_chunk mode of the launch: 1 one contiguous eighth of the workgroups per XCD, 0 launch order
};
// `aligned`: the input and output base pointers are multiples of 16; grid_max: CTK_LEVEL_GRID_MAX, or a test's lower cap
inline CtkReversalPlan ctk_reversal_plan(int elem_bytes, int64_t ny, int64_t nx, int64_t steps, bool aligned, int64_t grid_max = CTK_LEVEL_GRID_MAX)
{
    CtkReversalPlan p = {};
    p.vec = aligned && (nx * elem_bytes) % 16 == 0;
    p.vpt = p.vec ? 16 / elem_bytes : 1;
    const int64_t lanes = ny * (nx / p.vpt);                                      // (vector form: nx is a multiple of vpt)
    p.bps = (lanes + CTK_REVERSAL_THREADS - 1) / CTK_REVERSAL_THREADS;
    p.blocks = p.bps * steps;
    p.grid = (unsigned)std::min<int64_t>(p.blocks, std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX));
    p.xcd = p.grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    return p;
}
// rows [r0, r1) that some active row reads (itself and its partners) and rows [a0, a1) spanned by the active rows: what a host-array
// call uploads and downloads of every plane.  eq2 may be null.  No active row: all four are 0.
struct CtkReversalRows { int r0, r1, a0, a1; };
inline CtkReversalRows ctk_reversal_rows(const int32_t *eq, const int32_t *po, const int32_t *eq2, int ny)
{
    CtkReversalRows r = {ny, 0, ny, 0};
    for (int j = 0; j < ny; j++) {
        if (eq[j] < 0) continue;
        r.a0 = std::min(r.a0, j); r.a1 = std::max(r.a1, j + 1);
        const int rows[4] = {j, (int)eq[j], (int)po[j], eq2 ? (int)eq2[j] : j};
        for (int k = 0; k < 4; k++) { r.r0 = std::min(r.r0, rows[k]); r.r1 = std::max(r.r1, rows[k] + 1); }
    }
    if (r.a1 == 0) r = {0, 0, 0, 0};
    return r;
}

// ------------------------------------------------------------------------------------------------
// local wave activity (ctk_lwa.hip): k_lwa_contour, one workgroup per (step, domain) -- a domain is the rows of one hemisphere from
// the equator side to the pole --, and k_lwa_integral, one workgroup per (step, domain, strip of columns) with the strip's domain
// rows in LDS.  A strip is as wide as keeps rows x strip within CTK_LWA_CELLS pixels: a thread per (active row, column) then walks
// the domain, and about half the rows are active.  Vector form: 16-byte loads into LDS -- aligned base pointers, rows and strips of
// a multiple of 4 pixels; scalar form: pixel by pixel, strips of any width.  The capacity edge is the narrowest strip (4 pixels, or
// 1) of the longest domain in CTK_LWA_LDS_MAX bytes, and k_lwa_contour's four 8-byte words per row (+ 1, + one per wave): beyond that the
// plan says ok = 0 and the call ends with CTK_E_INVALID -- there is no other form.
// ------------------------------------------------------------------------------------------------
#define CTK_LWA_THREADS 256           // k_lwa_integral
#define CTK_LWA_SEL_THREADS 1024      // k_lwa_contour: one workgroup has a whole (step, domain) to itself
#define CTK_LWA_CELLS 2048            // pixels of a strip in LDS that the strip width aims at (rows x strip)
#define CTK_LWA_LDS_MAX 65536         // dynamic LDS of a workgroup of either kernel
struct CtkLwaPlan {
    int ok;                       // 0: the longest domain does not fit in LDS at the narrowest strip
    int vec;                      // 1: 16-byte loads of the strip, 0: the scalar form
    int strip;                    // columns of a strip (vector form: a multiple of 4)
    int64_t nstrips;              // strips of a row
    int64_t lds;                  // bytes of LDS of a k_lwa_integral workgroup: rows x strip pixels
    int64_t lds_sel;              // ... of a k_lwa_contour workgroup: 32 bytes per row + 1 (every row may be active), 8 per wave
    int64_t blocks;               // k_lwa_integral: steps x domains x strips, walked by ...
    unsigned grid;                // ... this many workgroups (CTK_LEVEL_GRID_MAX at most)
    int xcd;                      // xcd_chunk mode of that launch: 1 one contiguous eighth of the workgroups per XCD, 0 launch order
    int64_t sel_blocks;           // k_lwa_contour: steps x domains, walked by ...
    unsigned sel_grid;            // ... this many workgroups
    int sel_xcd;                  // xcd_chunk mode of that launch
};
// rows: the longest domain; aligned: input and output base pointers are multiples of 16; grid_max: CTK_LEVEL_GRID_MAX, or a test's lower cap
inline CtkLwaPlan ctk_lwa_plan(int elem_bytes, int64_t rows, int64_t nx, int64_t ndom, int64_t steps, bool aligned, int64_t grid_max = CTK_LEVEL_GRID_MAX)
{
    CtkLwaPlan p = {};
    p.vec = aligned && nx % 4 == 0;
    const int64_t unit = p.vec ? 4 : 1;
    const int64_t widest = (nx + unit - 1) / unit * unit;
    p.strip = (int)std::min<int64_t>(std::max<int64_t>(CTK_LWA_CELLS / std::max<int64_t>(rows, 1) / unit, 1) * unit, widest);
    p.nstrips = (nx + p.strip - 1) / p.strip;
    p.lds = rows * p.strip * elem_bytes;
    p.lds_sel = (rows + 1) * 32 + CTK_LWA_SEL_THREADS / 64 * 8;
    p.ok = rows * unit * elem_bytes <= CTK_LWA_LDS_MAX && p.lds_sel <= CTK_LWA_LDS_MAX;
    p.blocks = steps * ndom * p.nstrips;
    p.grid = (unsigned)std::min<int64_t>(p.blocks, std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX));
    p.xcd = p.grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    p.sel_blocks = steps * ndom;
    p.sel_grid = (unsigned)std::min<int64_t>(p.sel_blocks, std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX));
    p.sel_xcd = p.sel_grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
// selection of tracks or (step, track) rows of a flag slab (ctk_subset.hip): k_subset, one thread per 16 bytes of adjacent pixels of
// one step (vector form: every plane starts on a 16-byte boundary) or per pixel (scalar form).  A workgroup takes a PART of one step,
// CTK_SUBSET_TILES tiles of 256 lanes, per load of its table; the table's shape picks the form:
//     by id, no hits, largest id below CTK_SUBSET_BITMAP_BITS    a bitmap over [0, largest id] in LDS
//     by id, at most CTK_SUBSET_LDS_IDS ids                      binary search over the sorted ids in LDS (hits: counters beside them)
//     by id, more                                                binary search in global memory
//     by row, longest slice at most CTK_SUBSET_LDS_IDS           the step's slice in LDS, searched
//     by row, longer                                             the step's slice searched in global memory
// The by-id forms load the table once per workgroup, which then strides over as many parts as keep the table at CTK_SUBSET_TABLE_SHARE
// bytes per part or less (a part is 16 KB of flags) -- one part where the table is that small: a workgroup per part measured 0.92 of
// the copy kernel where 2048 striding ones reached 0.71-0.79 (profiles/NOTES.md); the row forms load a slice per part and launch one
// workgroup per part.  CTK_LEVEL_GRID_MAX workgroups at most, the rest by striding.
// ------------------------------------------------------------------------------------------------
#define CTK_SUBSET_THREADS 256
#define CTK_SUBSET_TILES 4                    // tiles of 256 lanes per part: their loads are in flight together
#define CTK_SUBSET_BITMAP_BITS (1ll << 18)    // 32 KB of LDS: five workgroups per CU
#define CTK_SUBSET_LDS_IDS 4096               // 16 KB of ids, 16 KB of uint32 counters with hits
#define CTK_SUBSET_TABLE_SHARE 1024           // bytes of table a by-id workgroup loads per part it takes, at most
#define CTK_SUBSET_BITMAP 0
#define CTK_SUBSET_SEARCH_LDS 1
#define CTK_SUBSET_SEARCH_GLB 2
#define CTK_SUBSET_ROW_LDS 3
#define CTK_SUBSET_ROW_GLB 4
struct CtkSubsetPlan {
    int form;                     // CTK_SUBSET_BITMAP .. CTK_SUBSET_ROW_GLB
    int vec;                      // 1: a 16-byte load and a 16-byte store per lane, 0: the scalar form
    int vpt;                      // pixels per thread: 4 or 1
    int64_t lds;                  // bytes of dynamic LDS of a workgroup
    int64_t bps;                  // parts per step
    int64_t blocks;               // bps * steps: (step, part) pairs, walked by ...
    unsigned grid;                // ... this many workgroups
    int xcd;                      // xcd_chunk mode of the launch: 1 one contiguous eighth of the workgroups per XCD, 0 launch order
};
// by_row: the table has a slice per step; max_id: the largest id of a by-id table (0: an empty one); longest: the ids of a by-id table,
// the longest slice of a row table; hits: the call counts per entry; aligned: the flag's and the output's base pointers are multiples
// of 16; grid_max: CTK_LEVEL_GRID_MAX, or a test's lower cap
inline CtkSubsetPlan ctk_subset_plan(bool by_row, int64_t max_id, int64_t longest, bool hits, int64_t npix, int64_t steps, bool aligned,
                                     int64_t grid_max = CTK_LEVEL_GRID_MAX)
{
    CtkSubsetPlan p = {};
    if (by_row) p.form = longest <= CTK_SUBSET_LDS_IDS ? CTK_SUBSET_ROW_LDS : CTK_SUBSET_ROW_GLB;
    else p.form = !hits && max_id < CTK_SUBSET_BITMAP_BITS ? CTK_SUBSET_BITMAP : longest <= CTK_SUBSET_LDS_IDS ? CTK_SUBSET_SEARCH_LDS : CTK_SUBSET_SEARCH_GLB;
    p.lds = p.form == CTK_SUBSET_BITMAP ? ((max_id >> 5) + 1) * 4
          : p.form == CTK_SUBSET_SEARCH_LDS || p.form == CTK_SUBSET_ROW_LDS ? longest * (hits ? 8 : 4) : 0;
    p.vec = aligned && npix % 4 == 0;
    p.vpt = p.vec ? 4 : 1;
    const int64_t lanes = (npix + p.vpt - 1) / p.vpt, per_part = (int64_t)CTK_SUBSET_THREADS * CTK_SUBSET_TILES;
    p.bps = (lanes + per_part - 1) / per_part;
    p.blocks = p.bps * steps;
    const int64_t per_load = by_row ? 1 : std::max<int64_t>((p.lds + CTK_SUBSET_TABLE_SHARE - 1) / CTK_SUBSET_TABLE_SHARE, 1);          // parts per table load
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX);
    p.grid = (unsigned)std::min<int64_t>((p.blocks + per_load - 1) / per_load, cap);
    p.xcd = p.grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
// per-block peak and extent (ctk_blockstat.hip): k_blockstat in k_subset's row geometry -- a workgroup takes a PART of one step,
// CTK_SUBSET_TILES tiles of CTK_SUBSET_THREADS lanes, a lane 16 bytes of flags (vector form: every plane starts on a 16-byte boundary)
// or one pixel (scalar form) -- and reduces the pixels of the step's wanted ids into one record per entry:
//     CTK_BLOCKSTAT_ROW_LDS    the step's slice, its records and its column bit sets in LDS; LDS atomics per pixel, one merge into the
//                              records in HBM per touched entry and part
//     CTK_BLOCKSTAT_ROW_GLB    the slice searched in global memory, the atomics straight on the records in HBM
// An entry takes CTK_BLOCKSTAT_REC bytes of LDS (its id, two 64-bit and four 32-bit accumulators) and, when the shape is wanted, a bit
// per column in whole words.  The LDS form runs while the longest slice fits CTK_BLOCKSTAT_LDS_BYTES: 32 KB, so that five workgroups
// fit a CU's 160 KB -- 390 entries of a 360-column grid, 151 of a 1440-column one, where a step of a tracked slab has a few dozen.
// float64 peaks take a second pass (key and position do not fit one 64-bit word): passes = 2.
// ------------------------------------------------------------------------------------------------
#define CTK_BLOCKSTAT_ROW_LDS 0
#define CTK_BLOCKSTAT_ROW_GLB 1
#define CTK_BLOCKSTAT_REC 36                   // bytes of LDS per entry without its bit set
#define CTK_BLOCKSTAT_LDS_BYTES (32ll << 10)
struct CtkBlockstatPlan {
    int form;                     // CTK_BLOCKSTAT_ROW_LDS or CTK_BLOCKSTAT_ROW_GLB
    int vec;                      // 1: a 16-byte load of flags per lane, 0: the scalar form
    int vpt;                      // pixels per thread: 4 or 1
    int passes;                   // launches of k_blockstat per chunk: 2 with float64 peaks, else 1
    int64_t words;                // 32-bit words of an entry's column bit set: ceil(nx / 32), 0 without the shape
    int64_t entry;                // bytes of LDS per entry: CTK_BLOCKSTAT_REC + 4 * words
    int64_t lds;                  // bytes of dynamic LDS of a workgroup: longest * entry, 0 in the global form
    int64_t bps;                  // parts per step
    int64_t blocks;               // bps * steps: (step, part) pairs, walked by ...
    unsigned grid;                // ... this many workgroups
    int xcd;                      // xcd_chunk mode of the launch, as CtkSubsetPlan's
};
// shape, peaks: what the call wants; elem_bytes: of the field (4 or 8; without peaks it does not matter); longest: the longest slice
// of the table; aligned: the flag's base pointer is a multiple of 16 (the field is read one value at a time, under the id test);
// grid_max: CTK_LEVEL_GRID_MAX, or a test's lower cap
inline CtkBlockstatPlan ctk_blockstat_plan(bool shape, bool peaks, int elem_bytes, int64_t longest, int64_t nx, int64_t npix, int64_t steps, bool aligned,
                                           int64_t grid_max = CTK_LEVEL_GRID_MAX)
{
    CtkBlockstatPlan p = {};
    p.words = shape ? (nx + 31) / 32 : 0;
    p.entry = CTK_BLOCKSTAT_REC + 4 * p.words;
    p.form = longest * p.entry <= CTK_BLOCKSTAT_LDS_BYTES ? CTK_BLOCKSTAT_ROW_LDS : CTK_BLOCKSTAT_ROW_GLB;
    p.lds = p.form == CTK_BLOCKSTAT_ROW_LDS ? longest * p.entry : 0;
    p.passes = peaks && elem_bytes == 8 ? 2 : 1;
    p.vec = aligned && npix % 4 == 0;
    p.vpt = p.vec ? 4 : 1;
    const int64_t lanes = (npix + p.vpt - 1) / p.vpt, per_part = (int64_t)CTK_SUBSET_THREADS * CTK_SUBSET_TILES;
    p.bps = (lanes + per_part - 1) / per_part;
    p.blocks = p.bps * steps;
    p.grid = (unsigned)std::min<int64_t>(p.blocks, std::min<int64_t>(std::max<int64_t>(grid_max, 1), CTK_LEVEL_GRID_MAX));
    p.xcd = p.grid >= CTK_LEVEL_XCD_MIN ? 1 : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
// rules every streamed entry shares
// ------------------------------------------------------------------------------------------------
// steps per chunk: chunk_steps, or (0) about 256 MB of input -- step_bytes is what one step brings in, a plane or the selected levels of
// one --, at least min_steps (the anomaly stream: its halo) and at most all T of them
inline int64_t ctk_stream_chunk(int64_t chunk_steps, int64_t T, size_t step_bytes, int64_t min_steps = 1)
{
    const int64_t c = chunk_steps > 0 ? chunk_steps : (int64_t)(((size_t)256 << 20) / std::max<size_t>(step_bytes, 1));
    return std::min<int64_t>(std::max<int64_t>(c, min_steps), T);
}
// timesteps per slice (blockIdx.y) of the kernels that give a thread 4 pixels and a slice of the T steps (k_freq, k_spell): `forced` (a
// debug override) or as many as fill the chip with `waves` waves, within [slice_min, slice_max]; and gridDim.y <= 65535
inline int64_t ctk_time_slice(int64_t forced, int64_t T, int64_t npix, int64_t slice_min, int64_t slice_max, int64_t waves)
{
    const int64_t per_slice = (npix + 255) / 256;                                   // waves per slice (4 pixels per lane)
    const int64_t s = forced > 0 ? forced : std::min(slice_max, std::max(slice_min, (T * per_slice + waves - 1) / waves));
    return std::max(s, (T + 65534) / 65535);
}

// ------------------------------------------------------------------------------------------------
// composite over flagged time steps (ctk_composite.hip): k_composite, one lane per pixel for ALL time steps of a launch -- T is never
// split, the float64 sums are added in time order.  What keeps the kernel busy is loads in flight: about pixels * (4 + elem_bytes) *
// unroll bytes, against CTK_COMPOSITE_FLIGHT chip-wide (256 CUs of ~32 KiB each).  A 1-degree plane needs the longest batch of steps;
// a quarter-degree plane fills the chip by itself, and there the batch only spreads the one dependent trip (flags, then the field of
// the lanes that passed) over more steps: 8 and 16 measured the same, 4 a sixth slower (profiles/NOTES.md).
// ------------------------------------------------------------------------------------------------
#define CTK_COMPOSITE_THREADS 256
#define CTK_COMPOSITE_UNROLL_MAX 16            // time steps whose loads of a lane are in flight together (then 8, 4, 2, 1 for the rest)
#define CTK_COMPOSITE_UNROLL_MIN 8
#define CTK_COMPOSITE_FLIGHT (8ll << 20)       // bytes in flight that fill the chip
#define CTK_COMPOSITE_GRID_MAX 0xffffffll      // workgroups of a launch: gridDim.x * blockDim.x stays below 2^32 work-items (as CTK_LEVEL_GRID_MAX)
struct CtkCompositePlan {
    int unroll;                   // the widest batch of time steps a lane loads before it uses the first (a power of two)
    int64_t blocks;               // parts of the plane of 256 pixels each, walked by ...
    unsigned grid;                // ... this many workgroups
};
// unroll: a test's choice (ctk_debug_set_composite), rounded down to a power of two and capped; -1 the rule
inline CtkCompositePlan ctk_composite_plan(int elem_bytes, int64_t npix, int unroll = -1)
{
    CtkCompositePlan p = {};
    const int64_t want = CTK_COMPOSITE_FLIGHT / std::max<int64_t>(npix * (4 + elem_bytes), 1);
    int u = CTK_COMPOSITE_UNROLL_MAX;
    while (u > CTK_COMPOSITE_UNROLL_MIN && u > want) u >>= 1;
    if (unroll > 0) { u = 1; while (u * 2 <= unroll && u * 2 <= CTK_COMPOSITE_UNROLL_MAX) u <<= 1; }
    p.unroll = u;
    p.blocks = (npix + CTK_COMPOSITE_THREADS - 1) / CTK_COMPOSITE_THREADS;
    p.grid = (unsigned)std::min<int64_t>(p.blocks, CTK_COMPOSITE_GRID_MAX);
    return p;
}

// ------------------------------------------------------------------------------------------------
// reductions over space per time step (ctk_band.hip): k_band, one thread per (step, 4 neighbouring columns) for ALL rows of the band
// -- the rows of a column are never split, the float64 sums are added in rising latitude.  The vector form (16-byte nontemporal
// loads) needs whole quads per row and a 16-byte aligned flag pointer; every other shape and alignment takes the general form, which
// pads the columns beyond the row.  rows: the widest batch of rows whose loads a thread has in flight before it adds the first.
// ------------------------------------------------------------------------------------------------
#define CTK_BAND_THREADS 256
#define CTK_BAND_ROWS 8                        // the rule's batch of rows (then 4, 2, 1 for the rest of the band)
#define CTK_BAND_ROWS_MAX 16
struct CtkBandPlan {
    bool vec;                     // the 16-byte form
    int rows;                     // the widest batch of rows in flight (a power of two)
    int64_t quads;                // threads per step: ceil(nx / 4)
    unsigned grid;                // workgroups: ceil(T * quads / 256) (the entries refuse a T that does not fit)
};
// T steps go into one launch of k_band (a thread per quad of columns) and of k_band_sect (a thread per sector): gridDim.x * blockDim.x
// stays below 2^32 work-items, as CTK_LEVEL_GRID_MAX keeps it for the striding kernels -- what the entries refuse otherwise
inline bool ctk_band_fits(int64_t T, int nx, int nsect)
{
    const int64_t lim = 0xffffffffll - CTK_BAND_THREADS;                           // (a partial last workgroup is launched whole)
    return T <= lim / std::max<int64_t>(nsect, 1) && T <= lim / (((int64_t)nx + 3) / 4);
}
// form: a test's choice (ctk_debug_set_band: 0 the vector form where it is legal, 1 the general form), rows: its batch, rounded down
// to a power of two and capped; -1 the rule
inline CtkBandPlan ctk_band_plan(int64_t T, int nx, bool aligned16, int form = -1, int rows = -1)
{
    CtkBandPlan p = {};
    p.vec = nx % 4 == 0 && aligned16 && form != 1;
    int r = CTK_BAND_ROWS;
    if (rows > 0) { r = 1; while (r * 2 <= rows && r * 2 <= CTK_BAND_ROWS_MAX) r <<= 1; }
    p.rows = r;
    p.quads = ((int64_t)nx + 3) / 4;
    p.grid = (unsigned)((T * p.quads + CTK_BAND_THREADS - 1) / CTK_BAND_THREADS);
    return p;
}

// ------------------------------------------------------------------------------------------------
// block-centred composite (ctk_centred.hip): one lane per cell (j, i) of the window for ALL stamps of the workgroup's bin -- a bin's
// stamps are never split, the float64 sums are added in stamp order.  There are few cells (a 41 x 81 window is 3321) and each is a
// chain of dependent adds behind gathers.  Two forms:
//   plain (k_centred): the lane gathers for itself, a batch of stamps whose loads it has in flight together -- 128 bytes of values per
//     lane, 32 float32 or 16 float64.  The workgroups are single waves while there are few of them (every CU gets one before any gets
//     two); past CTK_CENTRED_SMALL_GROUPS of them the chip is full and they are 256 cells wide.
//   fed (k_centred_fed): 64 cells per workgroup of 16 waves; 15 feeder waves gather 15 x 32 bytes per cell into LDS, the owner wave adds
//     them in order while the feeders fetch the next 120 (60) stamps: what k_life_exact does for its chains.
// Which one: the plain form's time is its longest chain -- the longest bin, one scalar and one vector memory latency per batch of 32
// stamps, 5.8 us measured, 181 ns per stamp -- unless the chip is full, and then 0.076 ns per (wave of cells x stamp).  The fed form
// walks a bin at 23 ns per stamp, and costs 0.082 ns per (wave of cells x stamp) plus 3.3 ns per workgroup: sixteen waves for 64
// cells are a poor trade when a bin has a dozen stamps.  The rule takes the smaller of the two estimates (MI355X, float32, both probe
// workloads with one bin, 16 bins and ~400 bins: the estimate picks the faster form in all six, profiles/NOTES.md); a bin shorter
// than CTK_CENTRED_FED_STAMPS -- little more than one round of the feeders -- stays with the plain form.
// ------------------------------------------------------------------------------------------------
#define CTK_CENTRED_THREADS_MIN 64
#define CTK_CENTRED_THREADS_MAX 256
#define CTK_CENTRED_UNROLL_MAX 32              // stamps whose loads of a lane are in flight together (then 16, 8, 4, 2, 1 for the rest)
#define CTK_CENTRED_BATCH_BYTES 128            // of values per lane in flight
#define CTK_CENTRED_SMALL_GROUPS 2048          // 256 CUs x 8 workgroups
#define CTK_CENTRED_GRID_MAX 0xffffffll
#define CTK_CENTRED_FED_WAVES 16               // one owner and 15 feeders
#define CTK_CENTRED_FED_BYTES 32               // of values per feeder lane and round: 8 float32 or 4 float64 stamps
#define CTK_CENTRED_FED_STAMPS 128
#define CTK_CENTRED_PLAIN_NS_STAMP 181.0       // per stamp of the longest bin
#define CTK_CENTRED_PLAIN_NS_WORK 0.076        // per (wave of cells x stamp)
#define CTK_CENTRED_FED_NS_STAMP 23.0
#define CTK_CENTRED_FED_NS_WORK 0.082
#define CTK_CENTRED_FED_NS_GROUP 3.3           // per workgroup
struct CtkCentredPlan {
    int form;                     // 0 plain, 1 fed
    int unroll;                   // plain: the widest batch of stamps a lane loads before it adds the first (a power of two); fed: stamps per feeder and round
    int threads;                  // cells of one bin per workgroup (64, 128 or 256; fed: 64)
    int64_t parts;                // workgroups per bin
    int64_t blocks;               // nbins * parts, walked by ...
    unsigned grid;                // ... this many workgroups
};
// wcells: (2 hy + 1) * (2 hx + 1); max_bin: the stamps of the longest bin; kept: the stamps of all bins.  form, unroll, threads: a
// test's choice (ctk_debug_set_centred; unroll and threads rounded down to a power of two and clamped, and without effect on the fed
// form); -1 the rule
inline CtkCentredPlan ctk_centred_plan(int elem_bytes, int64_t nbins, int64_t wcells, int64_t max_bin, int64_t kept, int form = -1, int unroll = -1,
                                       int threads = -1)
{
    CtkCentredPlan p = {};
    const int64_t per_bin = (wcells + CTK_CENTRED_THREADS_MIN - 1) / CTK_CENTRED_THREADS_MIN, waves = nbins * per_bin;
    const double work = (double)kept * (double)per_bin;
    const double plain_ns = std::max((double)max_bin * CTK_CENTRED_PLAIN_NS_STAMP, work * CTK_CENTRED_PLAIN_NS_WORK);
    const double fed_ns = std::max((double)max_bin * CTK_CENTRED_FED_NS_STAMP, work * CTK_CENTRED_FED_NS_WORK + (double)waves * CTK_CENTRED_FED_NS_GROUP);
    p.form = form >= 0 ? (form != 0) : (max_bin >= CTK_CENTRED_FED_STAMPS && fed_ns < plain_ns);
    int u = CTK_CENTRED_BATCH_BYTES / std::max(elem_bytes, 4);
    if (unroll > 0) { u = 1; while (u * 2 <= unroll && u * 2 <= CTK_CENTRED_UNROLL_MAX) u <<= 1; }
    int th = CTK_CENTRED_THREADS_MIN;
    if (waves > CTK_CENTRED_SMALL_GROUPS) th = CTK_CENTRED_THREADS_MAX;
    if (threads > 0) { th = CTK_CENTRED_THREADS_MIN; while (th * 2 <= threads && th * 2 <= CTK_CENTRED_THREADS_MAX) th <<= 1; }
    if (p.form) { u = CTK_CENTRED_FED_BYTES / std::max(elem_bytes, 4); th = CTK_CENTRED_THREADS_MIN; }
    p.unroll = std::min(u, CTK_CENTRED_UNROLL_MAX);
    p.threads = th;
    p.parts = (wcells + th - 1) / th;
    p.blocks = nbins * p.parts;
    // (gridDim.x * blockDim.x stays below 2^32 work-items: the fed form's workgroups are 1024 wide, a quarter as many fit)
    p.grid = (unsigned)std::min<int64_t>(p.blocks, p.form ? CTK_CENTRED_GRID_MAX / (64 * CTK_CENTRED_FED_WAVES / CTK_CENTRED_THREADS_MAX) : CTK_CENTRED_GRID_MAX);
    return p;
}
