/* contrack_hip_debug.h -- test hooks, staged-parity accessors, experiment knobs and measurement support of libcontrack_hip.so.
 *
 * NOT part of the drop-in boundary (include/contrack_hip.h is): nothing a caller of the reference's run_contrack / run_lifecycle /
 * calc_anom replacement needs is declared here.  The parity tests (tests/), the measurement scripts (bench.py, tools/) and the
 * probes bind these through ctypes; they are exported by the same shared object and may change between rounds.
 *   ctk_debug_*                      test hooks (forced overflows, failures, stalls), staged outputs (mask, 2-D labels), GPU-free
 *                                    pieces of the resolver, placement / launch-shape experiments
 *   ctk_set_filter_round / _fused_pass / _device_resolve     which form of the pass runs (the defaults are the product)
 *   ctk_synth_fill*, ctk_checksum_i32_dev, ctk_check_flag_dev   synthetic slabs and size-independent result checks on the device
 *   ctk_expand_runs_host             the decoder of the run-table result transfer on its own (host only)
 */
#ifndef CONTRACK_HIP_DEBUG_H
#define CONTRACK_HIP_DEBUG_H

#include "contrack_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test hook: the next ctk_track_sharded_* call on this handle fails at stage 1..6 (between two collectives), once */
int  ctk_debug_fail_at(ctk_handle *h, int stage);

int ctk_debug_mask(ctk_handle *h, uint8_t *mask /* (T,ny,nx) 0/1 */);

/* 2-D labels exactly as scipy numbers them at contrack.py:684 (before_seam=1) or after the seam merge
 * of contrack.py:691-698 (before_seam=0): ids are global over time, 1-based, raster order.        */
int ctk_debug_label2d(ctk_handle *h, int before_seam, int32_t *lab /* (T,ny,nx) */);

/* test hook: the NEXT call behaves as if the pair table held only `records` entries (exercises regrowth) */
int ctk_debug_set_pair_capacity(ctk_handle *h, uint32_t records);

/* test hook, GPU-free: numpy's float64 add.reduce order (what np.sum(weight_grid[...]) computes, contrack.py:717-719), used to
 * re-evaluate overlap decisions whose exactly accumulated area sums had to be rounded */
double ctk_debug_np_sum(const double *a, size_t n);

/* test hook, GPU-free: scipy's 3-D ids across time-shard boundaries from the per-rank boundary records of ctk_track_sharded_*
 * (contrack_amd/csrc/ctk_seam.h explains the records); flat arrays, rank after rank */
int ctk_debug_boundary_resolve(int world, const int32_t *nlast, const int32_t *nh, const int32_t *nroots, const int32_t *last_flat,
                               const int32_t *halo_flat, int64_t *off /* [world+1] */, int32_t *last_label_flat, int32_t *halo_label_flat,
                               int32_t *n_absorbed /* [world] */);
/* ... of a call with segment breaks (ctk_track_sharded_seg_*): nh[q] = 0 against a non-empty last step of rank q-1 is a cut that is
 * a break, nothing crosses it; n_crossing: the number of ids whose time extent the ranks would exchange */
int ctk_debug_boundary_resolve_breaks(int world, const int32_t *nlast, const int32_t *nh, const int32_t *nroots, const int32_t *last_flat,
                                      const int32_t *halo_flat, int64_t *off /* [world+1] */, int32_t *last_label_flat,
                                      int32_t *halo_label_flat, int32_t *n_absorbed /* [world] */, int32_t *n_crossing);

/* test hook: labels / operations of one seam cluster the device seam driver accepts (0 = its limits, 64 each): clusters beyond
 * send the pass to the synchronous path with the host driver, and the grid stays there */
int ctk_debug_set_seam_caps(ctk_handle *h, int labels, int ops);

/* test hook: facts about the handle's last ctk_track_sharded_* call, stored by the host where it takes each decision (an error if none
 * has finished).  Slots that hold two 32-bit facts: first | second << 32.
 *   out12[0]  capB, the capacity for the components of a cut step, at the end of the filter exchange (X3)
 *   out12[1]  how often that exchange was repeated because capB had to grow
 *   out12[2]  this rank's nlast | nh << 32 (components of its last step / of the halo it received)
 *   out12[3]  capC | capD << 32 at the end of the shared seam exchange (X5): group records / labels per rank
 *   out12[4]  repeats of that exchange
 *   out12[5]  the header this rank sent there: shared records | shared labels << 32
 *   out12[6]  ne, the ids of the extent exchange
 *   out12[7]  workgroups of the k_sh_pack_ext launch
 *   out12[8]  1 the seam tables initialised ahead of the boundary resolution were used, 0 k_sh_seam_init ran again, -1 the call made
 *             no device attempt
 *   out12[9]  the X5 form that finished the call: 0 device; otherwise host-driven, bits: 1 no device attempt (grid remembered as
 *             host-driven, shard length or id range), 2 more shared-cluster operations than the reserve, 4 some rank's device seam
 *             driver gave up
 *   out12[10] ng, the shared-cluster operations
 *   out12[11] 1 no rank saw a background pixel in the sample of its mask, so the zero flags of the write pass were exchanged afterwards
 *             (k_sh_count); 0 the sample settled it */
int ctk_debug_shard_exchange(ctk_handle *h, int64_t *out12);

/* test hook: the time-shard path's device form compares the number of shared-cluster operations with min(n, its reserve of 16384 op
 * slots) when n > 0 (0 = the reserve itself); beyond, the call is finished host-driven (CTK_S_HOST_REASON bit 4).  The allocation
 * stays the full reserve.  The decision is taken alike on every rank from the same gathered records, so the hook MUST be set to the
 * same value on every handle of a group: ranks that disagree would wait in different collectives. */
int ctk_debug_set_shared_ops_reserve(ctk_handle *h, int64_t n);

/* test hook: cap the device-written mailbox of the resolver hand-off (0 = no cap), so that the explicit-copy path runs; `labels`
 * also caps the list of shared ids the time-shard path's extent exchange keeps in LDS (longer lists: its one-workgroup form) */
int ctk_debug_set_mailbox(ctk_handle *h, uint32_t cand_records, uint32_t labels);

/* Test hook for the BOUNDED inter-workgroup waits of the one-launch ("systolic") filter pass: a wave that has waited longer than
 * limit_ms (0 = the default, 200 ms) for its predecessor gives up, the pass is marked invalid and the call repeats the resolution
 * with one launch per filter pass (CTK_S_HOST_REASON bit 3; the handle keeps doing so).  stall_mode 1: the first workgroup of the
 * chain arrives late (limit / 4); 2: it never publishes; 0: normal.  Also clears the handle's "no one-launch pass" state. */
int ctk_debug_set_spin(ctk_handle *h, double limit_ms, int stall_mode);

/* measurement support (bench.py, next to the roofline): best-of-`reps` time in ms of a PLAIN stream over a 16-byte-aligned device buffer --
 * mode 1: 16-byte non-temporal stores of zeros, 32 KB per workgroup in launch order; mode 2: the same with one contiguous eighth of the
 * buffer per XCD (the faster store stream on every size timed; the better of the two bounds the write kernel); mode 0: 16-byte
 * non-temporal loads (what bounds the threshold kernel).  Overwrites the buffer in modes 1 and 2. */
int ctk_debug_stream_ceiling(ctk_handle *h, void *p_dev, size_t nbytes, int mode, int reps, double *best_ms);

/* measurement support: the write kernel launched `reps` times on the finished tables of the last one-call pass into flag_dev (the same flags
 * again), every launch timed by events -> ms[reps].  variant: 0 k_relabel_v5, 1 the same without its SGPR limit; xcd: chunk -> XCD order (0 launch order, 1 one eighth of the launch per XCD, 16: tiles of 16; -1: the handle's). */
int ctk_debug_time_relabel(ctk_handle *h, int32_t *flag_dev, int persistence, int variant, int xcd, int reps, double *ms);

/* experiments: threads per workgroup (0 = default, 64 / 128 / 256) of the one-workgroup-per-timestep kernels k_extent, k_run_values,
 * k_compact_init of the one-call pass; extent = 1024: the sixteen-timesteps-per-workgroup form k_extent_blk whatever the shard's length
 * (test hook: by default it serves shards of more than 2048 timesteps on grids narrower than 1024) */
int ctk_debug_set_small_threads(ctk_handle *h, int extent, int run_values, int compact_init);

/* test hook, GPU-free, no handle: what the launch rules of contrack_amd/csrc/ctk_forms.h decide for a call of these numbers, so that
 * the tests' restatements of the rules (tests/label_forms.py, tail_forms.py, threshold_forms.py) are compared with the library on the
 * CPU.  Every field is an int64.  Query: a launch over timesteps [t0, t0 + nt) of a T-step shard of (ny, nx) planes; f64 / aligned16 /
 * field: the slab's (for the write plan: the output's) element type and 16-byte alignment, the threshold-field call; max_runs_step,
 * total_runs: what the run scan reported; n_labels, last_nlab: ids of this / the previous pass; async_passes, no_sys, n_cus, seg,
 * pslot: the filter's state (for round_*: one round of async_passes passes over T timesteps); path: 0 staged, 1 fused, 2 time-sharded;
 * forced_*: ctk_debug_set_small_threads; spec_set / launched: labelling variant sets as bits v1 1, v2 2, v3 4, glb 8, one 16, v1hi 32
 * (the previous call's speculative set / what ran speculatively on buffers that were large enough).
 * Plan: thr_kind 0 v7, 1 v6, 2 generic float32, 3 generic float64, 4 field vector, 5 field generic; *_bits as in CTK_S_LABEL_FORMS /
 * CTK_S_FILTER_FORMS; overlap_form, extent_form, write_kernel, write_shape, count_* as the statistics of the same name report them;
 * filter_unite 0 inside the pass kernel, 1 k_rs_unite_slots, 2 k_rs_unite; rowcount_groups: ctk_rowcount_groups for rowcount_threads,
 * the RCU of k_rowcount<RCU> (CTK_S_ROWCOUNT_GROUPS reports it for the kernel's first form, 0 for the other two). */
typedef struct ctk_form_query { int64_t T, nt, ny, nx, f64, aligned16, field, max_runs_step, total_runs, n_labels, last_nlab, async_passes, no_sys, n_cus, seg, pslot, path, forced_extent, forced_run_values, forced_compact_init, spec_set, launched; } ctk_form_query;
typedef struct ctk_form_plan { int64_t thr_kind, thr_u7, thr_rbt, thr_grid, rowcount_threads, v0b, v0_ok, v0_runs, need_glb, spec_launched, spec_bits, missing, missing_bits, next_spec, overlap_form, extent_form, write_kernel, write_rb, write_sub, write_kb, write_batched, write_lds, write_grid, write_shape, chunk_copy, runval_threads, compact_init_threads, count_staged, count_fused, filter_sys, filter_passes, filter_blk, filter_two_pc, filter_nb, filter_unite, filter_merged, filter_bits, filter_bits_sync, round_blk, round_two_pc, round_nb, rowcount_groups; } ctk_form_plan;
int ctk_debug_forms(const ctk_form_query *q, ctk_form_plan *p);

/* resources the library's owning types (csrc/ctk_own.h) hold in this process right now, over all handles:
 * out4 = { device buffers, pinned host buffers, events, streams }.  Memory from ctk_dev_malloc / ctk_host_alloc is the caller's and
 * is not counted.  No handle, no device. */
int ctk_debug_live(int64_t *out4);

/* test hook: the capacities in bytes of the staging buffers that the host-array and streamed entries of one handle share:
 * out4 = { io_in, io_out, one buffer of the pinned input pair, one buffer of the pinned output pair }; 0: not allocated (or released by
 * ctk_release_io).  The device buffers are grow-only with head room (a buffer that must grow to `need` bytes gets need + need / 8 + 256),
 * the pinned pairs grow to exactly the bytes asked for.  No device call. */
int ctk_debug_io_bytes(ctk_handle *h, int64_t *out4);

/* filter passes launched per round before convergence is checked on the host (default 10, 1..32)   */
int ctk_set_filter_round(ctk_handle *h, int passes);

/* 1 (default; CTK_ASYNC=0 in the environment turns it off): the one-call entries run the whole pass without a host hand-off (device
 * seam driver, one synchronisation at the end, validated from a device-written block of scalars; CTK_S_FUSED) and repeat the
 * resolution on the synchronous path below only if the validation says so; 0: always the synchronous path (host seam driver) */
int ctk_set_fused_pass(ctk_handle *h, int enable);

/* 1 (default): ctk_track_* resolve the tables on the device; 0: download + ctk_resolve on the host */
int ctk_set_device_resolve(ctk_handle *h, int enable);

/* deterministic on-device synthetic slab for throughput runs (bench only; not part of the path) */
int ctk_synth_fill(ctk_handle *h, float *anom_dev, int64_t T, int ny, int nx, uint64_t seed);

/* the window [t0, t0 + T) of the slab that ctk_synth_fill(seed) generates for any T >= t0 + T: time shards of one synthetic slab */
int ctk_synth_fill_window(ctk_handle *h, float *anom_dev, int64_t t0, int64_t T, int ny, int nx, uint64_t seed);

/* position-weighted checksum of an int32 device array (bench.py's in-run parity check of the time-shard path: the shards'
 * checksums against those of the one-call result).  out[0] = sum over i of (uint32)p[i] * (((index0 + i) * 0x9E3779B97F4A7C15) | 1)
 * mod 2^64, out[1] = number of nonzero elements.  Equal for two arrays iff (up to 2^-64 collisions) the arrays are equal. */
int ctk_checksum_i32_dev(ctk_handle *h, const int32_t *p_dev, int64_t n, int64_t index0, uint64_t *out2);

/* Size-independent properties of a result that lives in device memory (slabs no host holds: BASELINE.json configs[2], 60.6 GB each
 * way), for the parity tests: out6 = { pixels with flag != 0 where (double)anom <op> thr[t] is false (contrack.py:665 -- evaluated
 * in float64, independently of the kernels' float32 form), pixels whose id lies outside [1, max_id], nonzero pixels, distinct ids,
 * ids whose time extent stop - start is below `persistence` (contrack.py:765-772: none may survive), largest id }. */
int ctk_check_flag_dev(ctk_handle *h, const float *anom_dev, const int32_t *flag_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                       int persistence, int64_t max_id, uint64_t *out6);

/* The decoder of that transfer on its own, on tables in host memory (no device call; for tests): mask u64 [T][ny][ceil(nx/64)],
 * rowstart u32 [T][ny] (first run of the row, relative to its time step), run_base u32 [T + 1], run_val i32 [runs] -> flag
 * [T][ny][nx]; *wrote_background: a zero was written; *complex_runs: a negative run value was met (its pixels are not decoded). */
int ctk_expand_runs_host(const uint64_t *mask, const uint32_t *rowstart, const uint32_t *run_base, const int32_t *run_val, int64_t T, int ny, int nx,
                         int32_t *flag, int *wrote_background, int *complex_runs);

/* k_freq experiments (tools/freq_probe.py): timesteps per slice (0: the library's rule) and the 16-byte loads (0 plain, 1 nontemporal,
 * -1 the library's default: nontemporal) */
int ctk_debug_set_freq(ctk_handle *h, int64_t slice, int nt);
/* k_freq alone between HIP events: one launch that overwrites counts_dev, then `reps` timed launches that add to it; ms2 = {best, mean} */
int ctk_debug_time_freq(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                        uint32_t *counts_dev, int reps, double *ms2);

/* k_spell experiments and tests (tools/spell_probe.py): timesteps per slice (0: the library's rule) */
int ctk_debug_set_spell(ctk_handle *h, int64_t slice);
/* k_spell alone (one chunk of T steps, without k_spell_close) between HIP events: one launch on zeroed maps, then `reps` timed launches
 * that add to them; ms2 = {best, mean} */
int ctk_debug_time_spell(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts,
                         int64_t nseg, int32_t above, int by_id, int64_t min_duration, uint32_t *events_dev, uint32_t *steps_dev, uint32_t *longest_dev,
                         int reps, double *ms2);

/* test hook: the per-grid-point quantiles of the last ctk_percentile_* call on this handle, n = the band's pixels ((y1 - y0) * nx, row
 * major), before their mean is taken; an error if no result is held (a ctk_anom_* call or ctk_release_io in between) or n differs */
int ctk_debug_percentile_values(ctk_handle *h, double *out, int64_t n);

/* test hook: how often the last ctk_percentile_groups_* call on this handle read the band (launches of k_pctl_sweep and k_pctl_close) */
int ctk_debug_percentile_groups_sweeps(ctk_handle *h, int64_t *sweeps);
/* what ctk_pctl_form and ctk_pctl_refusal (csrc/ctk_forms.h) decide for a ctk_percentile_groups_* call on keys of `keybits` (32 / 64)
 * bits, a band of nband values, ngroups, window and a group of at most max_steps_of_a_group timesteps: out22 = { levels, sweeps
 * (levels + the closing sweep), stride (histogram slots per day), chunk (band values per sweep workgroup), chunks (workgroups per
 * timestep), shift[8], bits[8] (digit l is (key >> shift[l]) & ((1 << bits[l]) - 1); 0 beyond levels), refusal }.  refusal: what
 * the entry answers CTK_E_INVALID for -- 0 nothing, 1 a window below the group count above 1024, 2 ngroups x stride above 2^19
 * histograms, 3 more than 65 535 chunks, 4 a group whose timesteps x band values do not fit its uint32 counters -- the first of
 * these that holds; the entry asks the same function.  Host only: no handle, no GPU. */
int ctk_debug_percentile_groups_plan(int keybits, int64_t nband, int ngroups, int window, int64_t max_steps_of_a_group, int64_t *out22);
/* test hook: intermediate values of the last ctk_percentile_groups_* call on this handle, ngroups entries each, copied from the
 * handle's workspace: nu_day[d] = the distinct selected keys among the targets of day d (the groups whose window holds d), as the
 * last k_pctl_lists counted them (1 where the window covers every group); need[g] = 1 where group g takes its next larger key from
 * the closing sweep (its rank and the next one straddle the last digit's histogram); n_of[g] = the non-NaN values of its pool.
 * An error if no such call has run on the handle or ngroups differs from that call's. */
int ctk_debug_percentile_groups_state(ctk_handle *h, int ngroups, uint32_t *nu_day, uint32_t *need, uint64_t *n_of);
/* measurement (tools/pctl_probe.py) on a float32 slab in device memory: ms12 = { ctk_percentile_groups per call (best of reps, host
 * clock: upload of the ids, every kernel, download, synchronisation), one plain 16-byte read stream over the band with the sweeps'
 * grid (best of reps, HIP events), the scalar percentile's kernels (k_quantile + k_nanmean, once, HIP events), then the band sweeps
 * of one more call one by one (HIP events), 0 beyond the last }; out: the ngroups results */
int ctk_debug_time_percentile_groups(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups,
                                     int window, double q, int reps, double *out, double *ms12);

/* test hook: the kernel form of the last ctk_anom_seg_* / ctk_anom_stream_* launch on this handle: 1 the LDS ring (k_anom_ring), 0 the
 * plain form (k_anom_plain), -1 none yet (ctk_anom_plan, csrc/ctk_forms.h) */
int ctk_debug_anom_form(ctk_handle *h, int64_t *form);
/* what ctk_anom_plan (csrc/ctk_forms.h) decides for nt output steps of a plane of npix pixels (host only: no handle, no GPU);
 * waves_wanted / grid_y_max: 0 the rule's 16 384 and 65 535, or a test's values; out5 = { form, dynamic LDS in bytes, tile (output steps
 * per workgroup), gridDim.x, gridDim.y } */
int ctk_debug_anom_plan(int elem_bytes, int smooth, int64_t nt, int64_t npix, int64_t waves_wanted, int64_t grid_y_max, int64_t *out5);
/* test hook for the following anomaly launches of ctk_anom_seg_* / ctk_anom_stream_* / ctk_anom_seg_resident on this handle: the same two
 * values (0: the rule's; negative: refused; grid_y_max above 65 535 stays 65 535), so that a small slab reaches the tile edges */
int ctk_debug_set_anom(ctk_handle *h, int64_t waves_wanted, int64_t grid_y_max);
/* test hook: out8 = { form, tile, gridDim.x, gridDim.y, LDS bytes, o0, o1 } of the last anomaly launch on this handle (output steps
 * [o0, o1); form -1: none yet), then the number of such launches the last of those calls made (a streamed chunk that completes no
 * output step launches nothing) */
int ctk_debug_anom_launch(ctk_handle *h, int64_t *out8);

/* what ctk_filter_plan (csrc/ctk_forms.h) decides for nout outputs of a plane of npix pixels, K taps at `stride` (host only: no handle,
 * no GPU); waves_wanted / grid_y_max: 0 the rule's 16 384 and 65 535, or a test's values (a waves_wanted of a test's also drops the rule's
 * shortest tiles: 1 << 40 gives one output per workgroup, 1 the longest tile); forced: -1 the rule's form, 0 the plain form,
 * 1 the LDS ring where one fits; out6 = { form (1 k_filter_ring, 0 k_filter_plain), threads per workgroup, dynamic LDS in bytes, tile
 * (outputs per workgroup), gridDim.x, gridDim.y } */
int ctk_debug_filter_plan(int elem_bytes, int K, int64_t stride, int64_t nout, int64_t npix, int64_t waves_wanted, int64_t grid_y_max, int forced, int64_t *out6);
/* test hook for the following filter launches of ctk_filter_* on this handle: the same three values (negative waves_wanted / grid_y_max
 * and a form outside -1 .. 1: refused), so that a small slab reaches the tile edges and every form */
int ctk_debug_set_filter(ctk_handle *h, int64_t waves_wanted, int64_t grid_y_max, int forced);
/* test hook: out9 = { form, threads, tile, gridDim.x, gridDim.y, LDS bytes, o0, o1 } of the last filter launch on this handle (outputs
 * [o0, o1); form -1: none yet), then the number of launches the last ctk_filter_* call made (a streamed chunk that completes no output
 * launches nothing) */
int ctk_debug_filter_launch(ctk_handle *h, int64_t *out9);
/* measurement (tools/filter_probe.py) on slabs in device memory, one segment: the filter kernel alone between HIP events, one launch
 * that is not counted, then `reps` timed ones; copy_bytes > 0: the plain 16-byte copy kernel over that many bytes of the same two
 * buffers instead; ms2 = { best, mean } */
int ctk_debug_time_filter(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset,
                          int edges, int skipna, void *out_dev, int64_t T_out, int64_t copy_bytes, int reps, double *ms2);

/* what ctk_pfield_plan (csrc/ctk_forms.h) decides for keys of `keybytes` (4 / 8) bytes, a longest pool of max_pool_steps timesteps,
 * ngroups and window: out4 = { form (0 direct, 1 ring), the ring form's cap in pool timesteps, pixels per workgroup, bytes of the ring
 * (0: direct form) }.  Host only: no handle, no GPU. */
int ctk_debug_percentile_field_plan(int keybytes, int64_t max_pool_steps, int ngroups, int window, int64_t *out4);
/* test hook: out2 = { form the last ctk_percentile_field_* call on this handle took (-1: none yet), its longest pool in timesteps } */
int ctk_debug_percentile_field_form(ctk_handle *h, int64_t *out2);
/* measurement (tools/pfield_probe.py) on a slab in device memory (is_f64 != 0: float64): ms4 = { the form ctk_pfield_plan chooses,
 * the direct form forced on the same input (both per call, best of reps, host clock: upload of the lists, every kernel,
 * synchronisation; the download of the field is outside), one plain 16-byte read stream over the band (k_pctl_read, best of reps,
 * HIP events), the chosen form (0 direct, 1 ring) }; out / out_direct (either may be NULL): the two fields, ngroups * (y1 - y0) * nx */
int ctk_debug_time_percentile_field(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group,
                                    int ngroups, int window, double q, int reps, double *out, double *out_direct, double *ms4);

/* what ctk_std_plan (csrc/ctk_forms.h) decides for ngroups, window and skipna: out4 = { pixels per workgroup (0: the accumulators of
 * even 8 pixels do not fit -- ctk_std_field_* refuses the call), planes accumulated (1 when window >= ngroups), dynamic LDS of the
 * launch in bytes, the most groups a window below the group count may have }.  Host only: no handle, no GPU. */
int ctk_debug_std_field_plan(int ngroups, int window, int skipna, int64_t *out4);
/* test hook: out2 = { pixels per workgroup of the last ctk_std_field_* call on this handle (-1: none yet), its longest pool in timesteps } */
int ctk_debug_std_field_form(ctk_handle *h, int64_t *out2);
/* measurement (tools/std_probe.py) on a slab in device memory (is_f64 != 0: float64): ms2 = { ctk_std_field's device work per call
 * (best of reps, host clock: upload of the ids, every kernel, synchronisation; the download of the field is outside), pixels per
 * workgroup }; out_std (may be NULL): the field, ngroups * (y1 - y0) * nx */
int ctk_debug_time_std_field(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group,
                             int ngroups, int window, int ddof, int skipna, int reps, double *out_std, double *ms2);

/* what ctk_life_plan (csrc/ctk_forms.h) decides for a ctk_lifecycle_* call over T time steps of (ny, nx) planes, float64 field if f64,
 * whose flag / field slabs start flag_align / field_align bytes past a 32-byte boundary: out5 = { rows per wave of k_life_strips,
 * strips per row, workgroups per strip, 1 if the vector form k_life_strips<VT, true> runs, seam-crossing ids one pass of k_lifecycle
 * holds }.  Host only: no handle, no GPU. */
int ctk_debug_lifecycle_plan(int64_t T, int ny, int nx, int f64, int64_t flag_align, int64_t field_align, int64_t *out5);
/* test hook: the path of the last ctk_lifecycle_* call on this handle (an error if none finished, or if it had another T).
 * out8 = { rows per wave, strips per row, workgroups per strip, vector form (as above), time steps the strip form gave up, launches of
 * k_lifecycle, attempts (2: the row table was too small and everything ran again; the other figures describe the last attempt),
 * row order (0 two counting sorts, 1 comparison sort) }; steps[t]: the rounds of k_lifecycle time step t took part in -- 0 the strip
 * form held it, 1 one pass over all its ids, 2 its ids split into two residue classes, 3 into four, ... */
int ctk_debug_lifecycle_path(ctk_handle *h, int64_t *out8, uint8_t *steps, int64_t T);

/* what ctk_level_plan (csrc/ctk_forms.h) decides for a ctk_level_mean_* launch over `steps` steps of planes of npix pixels of
 * elem_bytes (4 / 8) with nsel selected levels, `aligned`: both base pointers are multiples of 16.  out7 = { 1 the vector form
 * (16 bytes per lane) / 0 the scalar form, pixels per thread, the widest batch of level loads in flight, workgroups per step,
 * workgroups of work (per step x steps), workgroups launched (at most 2^24 - 1; the kernel strides over the rest), 1 if every XCD takes one contiguous eighth of them (0: launch
 * order) }.  Host only: no handle, no GPU. */
int ctk_debug_level_plan(int elem_bytes, int64_t nsel, int64_t npix, int64_t steps, int aligned, int64_t *out7);
/* test hook / experiments for the following k_level_mean launches on this handle: how workgroups map to XCDs (0 launch order, 1 one
 * contiguous eighth per XCD, n > 1 tiles of n workgroups; -1: the rule above) and a lower cap on the workgroups of a launch, so that
 * a small case walks the kernel's stride loop (0: the rule's cap, 2^24 - 1: a launch stays below 2^32 work-items) */
int ctk_debug_set_level(ctk_handle *h, int xcd_mode, int64_t grid_max);
/* test hook: out2 = { the form of the last k_level_mean launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups } */
int ctk_debug_level_form(ctk_handle *h, int64_t *out2);
/* measurement (tools/level_probe.py): k_level_mean alone on slabs in device memory (the arguments of ctk_level_mean_*_dev; is_f64 != 0:
 * float64) between HIP events: one launch that is not counted, then `reps` timed ones; ms2 = { best, mean } */
int ctk_debug_time_level_mean(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna,
                              void *out_dev, int reps, double *ms2);

/* what ctk_reversal_plan (csrc/ctk_forms.h) decides for a ctk_reversal_* launch over `steps` steps of planes of ny rows of nx pixels
 * of elem_bytes (4 / 8), `aligned`: both base pointers are multiples of 16.  out6 = { 1 the vector form (16 bytes per lane; every row
 * starts on a 16-byte boundary) / 0 the scalar form, pixels per thread, workgroups per step, workgroups of work (per step x steps),
 * workgroups launched (at most 2^24 - 1; the kernel strides over the rest), 1 if every XCD takes one contiguous eighth of them (0:
 * launch order) }.  Host only: no handle, no GPU. */
int ctk_debug_reversal_plan(int elem_bytes, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t *out6);
/* test hook / experiments for the following k_reversal launches on this handle: as ctk_debug_set_level */
int ctk_debug_set_reversal(ctk_handle *h, int xcd_mode, int64_t grid_max);
/* test hook: out2 = { the form of the last k_reversal launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups } */
int ctk_debug_reversal_form(ctk_handle *h, int64_t *out2);
/* measurement (tools/reversal_probe.py): k_reversal alone on slabs in device memory (the arguments of ctk_reversal_*_dev; is_f64 != 0:
 * float64) between HIP events: one launch that is not counted, then `reps` timed ones; ms2 = { best, mean }.  eq == NULL: a plain
 * copy kernel (one 16-byte load and one 16-byte store per lane) over the same two buffers instead, the yardstick. */
int ctk_debug_time_reversal(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2,
                            const double *dE, const double *tS, const double *tN, const double *tS2, int mask, void *out_dev, int reps, double *ms2);

/* what ctk_subset_plan (csrc/ctk_forms.h) decides for a ctk_subset_* launch over `steps` steps of planes of ny rows of nx pixels from
 * the table's shape: by_row (0: by id), max_id the largest id of a by-id table (0: an empty one), longest the ids of a by-id table or
 * the longest slice of a row table, want_hits; `aligned`: both base pointers are multiples of 16; grid_max: a lower cap on the
 * workgroups of a launch (0: the rule's).  out12 = { the form: 0 bitmap in LDS (by id, no hits, max_id below the bitmap's bits), 1
 * sorted ids in LDS (by id, at most the LDS ids), 2 sorted ids in global memory, 3 the step's slice in LDS (by row, longest at most
 * the LDS ids), 4 the step's slice in global memory; 1 the vector form (16 bytes per lane; every plane starts on a 16-byte boundary:
 * ny * nx a multiple of 4) / 0 the scalar form; pixels per thread; LDS bytes of a workgroup; parts per step; parts of work (per step x
 * steps); workgroups launched (by id one per ceil(LDS bytes / out12[10]) parts, by row one per part, at most 2^24 - 1; the kernel strides over the rest); 1 if every XCD
 * takes one contiguous eighth of them (0: launch order); the capacities of the rule: bits of the bitmap, ids in LDS, bytes of table
 * per part of a by-id workgroup; lanes of a part }.  Host only: no handle, no GPU. */
int ctk_debug_subset_plan(int by_row, int64_t max_id, int64_t longest, int want_hits, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t grid_max,
                          int64_t *out12);
/* test hook / experiments for the following k_subset launches on this handle: as ctk_debug_set_level */
int ctk_debug_set_subset(ctk_handle *h, int xcd_mode, int64_t grid_max);
/* test hook: out3 = { the form of the last k_subset launch on this handle (0 .. 4 as above, -1 none yet), 1 vector / 0 scalar, its
 * workgroups } */
int ctk_debug_subset_form(ctk_handle *h, int64_t *out3);
/* measurement (tools/subset_probe.py): k_subset alone on slabs in device memory (the arguments of ctk_subset_dev; out_dev NULL: count
 * only; want_hits / want_n_selected: the counters are kept, not returned) between HIP events: one launch that is not counted, then
 * `reps` timed ones; ms2 = { best, mean }.  off == NULL: a plain copy kernel (one 16-byte load and one 16-byte store per lane) over
 * the same two buffers instead, the yardstick. */
int ctk_debug_time_subset(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids,
                          int invert, int kind, int32_t *out_dev, int want_hits, int want_n_selected, int reps, double *ms2);

/* what ctk_blockstat_plan (csrc/ctk_forms.h) decides for a ctk_blockstat_* launch over `steps` steps of planes of ny rows of nx pixels:
 * want as the entries take it, elem_bytes of the field (4 or 8), longest the longest slice of the row table; `aligned`: the flag's
 * base pointer is a multiple of 16; grid_max: a lower cap on the workgroups (0: the rule's).  out14 = { form: 0 the slice's records and
 * bit sets in LDS, 1 atomics straight on the records in HBM; 1 vector (16 bytes of flags per lane) / 0 scalar; pixels per thread; bytes
 * of dynamic LDS of a workgroup; parts per step; parts of work = parts per step * steps; workgroups launched; 1: every XCD takes one
 * contiguous eighth of them; launches per chunk (2: float64 peaks); words of an entry's column bit set; bytes of LDS per entry; the
 * LDS budget in bytes; the entries that fit it at this nx; lanes of a part }.  Host only: no handle, no GPU. */
int ctk_debug_blockstat_plan(int want, int elem_bytes, int64_t longest, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t grid_max, int64_t *out14);
/* test hook / experiments for the following k_blockstat launches on this handle: as ctk_debug_set_level */
int ctk_debug_set_blockstat(ctk_handle *h, int xcd_mode, int64_t grid_max);
/* test hook: out3 = { the form of the last k_blockstat launch on this handle (0 / 1 as above, -1 none yet), 1 vector / 0 scalar, its
 * workgroups } */
int ctk_debug_blockstat_form(ctk_handle *h, int64_t *out3);
/* measurement (tools/blockstat_probe.py): the k_blockstat launches of the whole slab alone on slabs in device memory (the arguments of
 * ctk_blockstat_*_dev; is_f64: the field's type) between HIP events: one round that is not counted, then `reps` timed ones; ms2 =
 * { best, mean }.  The records go on accumulating and are not returned.  off == NULL: a plain stream of 16-byte loads over the flag
 * slab and, where x_dev is given, the field slab instead, the yardstick. */
int ctk_debug_time_blockstat(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                             const int32_t *ids, int64_t n_ids, int want, int reps, double *ms2);

/* what ctk_lwa_plan (csrc/ctk_forms.h) decides for a ctk_lwa_* launch over `steps` steps of ndom (1 / 2) domains, the longest of
 * `rows` rows of nx pixels of elem_bytes (4 / 8), `aligned`: both base pointers are multiples of 16.  out12 = { 1 the domain fits in
 * LDS / 0 the call is refused, 1 the vector form (16-byte loads of the strip; nx a multiple of 4) / 0 the scalar form, columns of a
 * strip, strips of a row, LDS bytes of a k_lwa_integral workgroup, LDS bytes of a k_lwa_contour workgroup, workgroups of work (steps x
 * domains x strips), workgroups launched (at most 2^24 - 1; the kernel strides over the rest), 1 if every XCD takes one contiguous
 * eighth of them (0: launch order), and the same three for k_lwa_contour (steps x domains) }.  Host only: no handle, no GPU. */
int ctk_debug_lwa_plan(int elem_bytes, int64_t rows, int64_t nx, int64_t ndom, int64_t steps, int aligned, int64_t *out12);
/* test hook / experiments for the following k_lwa_contour and k_lwa_integral launches on this handle: as ctk_debug_set_level */
int ctk_debug_set_lwa(ctk_handle *h, int xcd_mode, int64_t grid_max);
/* test hook: out2 = { the form of the last k_lwa_integral launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups } */
int ctk_debug_lwa_form(ctk_handle *h, int64_t *out2);
/* measurement (tools/lwa_probe.py): one stage of ctk_lwa_*_dev alone on slabs in device memory (16-byte aligned; is_f64 != 0: float64)
 * between HIP events: one launch that is not counted, then `reps` timed ones; ms2 = { best, mean }.  stage 1: the contours, stage 2:
 * the integrals on the contours of one stage-1 run, stage 0: a plain copy kernel (one 16-byte load and one 16-byte store per lane)
 * over the same two buffers, the yardstick (the table arguments may be NULL). */
int ctk_debug_time_lwa(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows,
                       const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part, void *out_dev, int stage, int reps, double *ms2);

/* what ctk_composite_plan (csrc/ctk_forms.h) decides for a k_composite launch over planes of npix pixels and a field of elem_bytes
 * (4 / 8); unroll: what ctk_debug_set_composite would force (-1: the rule).  out3 = { the widest batch of time steps in flight,
 * workgroups of work (256 pixels each), workgroups launched (at most 2^24 - 1; the kernel strides over the rest) }.  Host only: no
 * handle, no GPU. */
int ctk_debug_composite_plan(int elem_bytes, int64_t npix, int unroll, int64_t *out3);
/* test hook for the following k_composite launches on this handle: the widest batch of time steps (rounded down to a power of two,
 * at most 16), -1 the rule */
int ctk_debug_set_composite(ctk_handle *h, int unroll);
/* test hook: out2 = { the widest batch of the last k_composite launch on this handle (0: none yet), its workgroups } */
int ctk_debug_composite_launch(ctk_handle *h, int64_t *out2);
/* measurement (tools/composite_probe.py): k_composite alone on slabs in device memory (is_f64 != 0: a float64 field) between HIP
 * events: one launch from zeroed accumulators that is not counted, then `reps` timed ones that continue from them; ms2 = { best, mean } */
int ctk_debug_time_composite(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const int32_t *group,
                             int ngroups, int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int reps, double *ms2);

/* what ctk_centred_plan (csrc/ctk_forms.h) decides for a centred launch over nbins bins of a (2 hy + 1) x (2 hx + 1) window, the
 * longest bin max_bin stamps and all bins together kept stamps, a field of elem_bytes (4 / 8); form, unroll, threads: what ctk_debug_set_centred would force (-1: the
 * rule).  out6 = { the batch: stamps a lane (plain form) or a feeder wave (fed form) has in flight, cells of a bin per workgroup (64 /
 * 128 / 256), workgroups of work per bin, workgroups of work in all, workgroups launched (at most 2^24 - 1; the kernels stride over
 * the rest), the form: 0 plain (k_centred), 1 fed (k_centred_fed) }.  Host only: no handle, no GPU. */
int ctk_debug_centred_plan(int elem_bytes, int nbins, int hy, int hx, int64_t max_bin, int64_t kept, int form, int unroll, int threads, int64_t *out6);
/* test hook for the following centred launches on this handle: the form (0 plain, 1 fed), and for the plain form the widest batch of
 * stamps (rounded down to a power of two, at most 32) and the cells per workgroup (rounded down to 64 / 128 / 256); -1 the rule */
int ctk_debug_set_centred(ctk_handle *h, int form, int unroll, int threads);
/* test hook: out4 = { the batch of the last centred launch on this handle (0: none yet), its cells per workgroup, its workgroups, its form } */
int ctk_debug_centred_launch(ctk_handle *h, int64_t *out4);
/* measurement (tools/centred_probe.py): the centred kernel alone (k_centred or k_centred_fed, as the rule or ctk_debug_set_centred decides) on a slab in device memory (is_f64 != 0: a float64 field; the stamps are host
 * arrays as in ctk_centred_*_dev) between HIP events: one launch from zeroed accumulators that is not counted, then `reps` timed ones
 * that continue from them; ms2 = { best, mean }.  floor != 0: instead of k_centred the yardstick kernel, a plain gather of the same
 * windows with one lane per (stamp, cell), in no order, that keeps nothing (sum_dev is its sink). */
int ctk_debug_time_centred(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row,
                           const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev,
                           int floor, int reps, double *ms2);

/* what ctk_band_plan (csrc/ctk_forms.h) decides for a k_band launch over T steps of rows of nx columns, aligned16: the flag pointer is
 * a multiple of 16; form, rows: what ctk_debug_set_band would force (-1: the rule).  out4 = { the form: 0 vector (16-byte loads), 1
 * general; the widest batch of rows in flight; threads per step; workgroups }.  Host only: no handle, no GPU. */
int ctk_debug_band_plan(int64_t T, int nx, int aligned16, int form, int rows, int64_t *out4);
/* test hook for the following k_band launches on this handle: the form (0 the vector form where nx % 4 == 0 and the pointer allow it,
 * 1 the general form) and the widest batch of rows in flight (rounded down to a power of two, at most 16); -1 the rule */
int ctk_debug_set_band(ctk_handle *h, int form, int rows);
/* test hook: out3 = { the form of the last k_band launch on this handle (-1: none yet), its widest batch of rows, its workgroups } */
int ctk_debug_band_launch(ctk_handle *h, int64_t *out3);
/* measurement (tools/band_probe.py): k_band -- and k_band_sect when the spec has sectors -- alone on slabs in device memory (the
 * arguments of ctk_band_dev) between HIP events: one launch that is not counted, then `reps` timed ones; ms2 = { best, mean } */
int ctk_debug_time_band(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int elem_bytes, int64_t T, int ny, int nx, const ctk_band_spec *spec,
                        const ctk_band_out *out_dev, int reps, double *ms2);

#ifdef __cplusplus
}
#endif

#endif /* CONTRACK_HIP_DEBUG_H */
