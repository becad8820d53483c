// ctk_api.hip -- host side of libcontrack_hip.so: handle, workspace, stage orchestration, C ABI
// (include/contrack_hip.h).  The kernels are in ctk_kernels.hip (same translation unit), the GPU-free
// sequential resolver in ctk_resolve.cpp.
#include "ctk_kernels.hip"
#include "ctk_resolve_dev.hip"
#include "ctk_seam_dev.hip"
#include "ctk_lifecycle.hip"
#include "ctk_seam.h"
#include "ctk_comm.h"
#include "ctk_forms.h"
#include "ctk_select.h"
#include "ctk_own.h"
#include "../../include/contrack_hip_debug.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>
#include <sys/mman.h>
#include <emmintrin.h>
#include <atomic>
#include <thread>
#include <functional>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <string>

int ctk_set_error(int code, const char *fmt, ...);            // ctk_resolve.cpp
extern "C" int ctk_weights_to_limbs(const float *wrow, int ny, int64_t npix, int64_t *wlo, int64_t *whi, int32_t *wshift, int32_t *limb_bits);
int ctk_resolve_ex(const void *const *blobs, const size_t *nbytes, int nshards, double overlap, int twosided, CtkExactAreas *exact,
                   ctk_result **out, const uint8_t *seg_edge = nullptr);       // ctk_resolve.cpp
double ctk_np_sum(const double *a, size_t n);

#define HIPCHK(expr)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess)                                                                                 \
            return ctk_set_error(e_ == hipErrorOutOfMemory ? CTK_E_NOMEM : CTK_E_NODEVICE, "%s failed: %s (%s:%d)", \
                                 #expr, hipGetErrorString(e_), __FILE__, __LINE__);                           \
    } while (0)
#define CTKCHK(expr)               \
    do {                           \
        int r_ = (expr);           \
        if (r_ != CTK_OK) return r_; \
    } while (0)

// Switches of the environment, read ONCE per process, here and nowhere else in this translation unit (getenv is a linear scan of
// environ and not safe against a concurrent setenv from another rank's host thread; the passes shave microseconds).
struct CtkEnv {
    int sd_dbg = 0, mask_tries = 0;
    bool seamstats = false, hosttrace = false, hostprof = false, shdebug = false, sh_force_split = false, rle_out = true, mask_tune = true, async = true;
    CtkEnv()
    {
        auto num = [](const char *k) { const char *e = getenv(k); return e ? atoi(e) : 0; };
        auto on = [](const char *k) { return getenv(k) != nullptr; };
        sd_dbg = num("CTK_SD_DBG"); seamstats = on("CTK_SEAMSTATS"); hosttrace = on("CTK_HOSTTRACE"); hostprof = on("CTK_HOSTPROF"); shdebug = on("CTK_SHDEBUG");
        sh_force_split = on("CTK_SH_FORCE_SPLIT");
        rle_out = !(on("CTK_RLE_OUT") && num("CTK_RLE_OUT") == 0);
        mask_tune = !(on("CTK_MASK_TUNE") && num("CTK_MASK_TUNE") == 0);
        mask_tries = std::min(std::max(num("CTK_MASK_TRIES"), 0), 1);
        async = !(on("CTK_ASYNC") && num("CTK_ASYNC") == 0);
    }
};
static const CtkEnv &ctk_env() { static const CtkEnv e; return e; }

static double g_ht0 = 0;
static double now_ms_fwd() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define HT(name) do { if (ctk_env().hosttrace) { double t_ = now_ms_fwd(); fprintf(stderr, "HT %-28s %9.1f us\n", name, (t_ - g_ht0) * 1e3); } } while (0)
#define HT0() do { if (ctk_env().hosttrace) g_ht0 = now_ms_fwd(); } while (0)

struct ShardScratch;
static void shard_scratch_free(ShardScratch *s);            // ctk_sharded.hip
struct ShardScratchFree { void operator()(ShardScratch *s) const { shard_scratch_free(s); } };

namespace {

enum State { ST_IDLE = 0, ST_LABELLED, ST_OVERLAPPED, ST_TABLES, ST_EXTENTS };

}  // namespace

#define CTK_KI_ROWCOUNT (CTK_K_COUNT + 1)
#define CTK_PSLOT 128            // fused path: pair-record slots per timestep (k_overlap); a timestep with more spills to the ungrouped records

// pinned (CPU-cacheable) bounce buffers of the host-array entries' device -> host copy (bounce_copy)
struct BounceLane {
    Stream st;                                     // (first: it goes last, after what was queued on it)
    PinBuf pin[2];
    Event ev[2];
    bool create(size_t bytes)
    {
        bool ok = true;
        for (int b = 0; b < 2 && ok; b++)
            ok = pin[b].alloc(bytes, hipHostMallocNonCoherent) == hipSuccess && ev[b].create(hipEventDisableTiming) == hipSuccess;
        return ok && st.create(hipStreamNonBlocking) == hipSuccess;
    }
    void release() { for (int b = 0; b < 2; b++) { pin[b].release(); ev[b].release(); } st.release(); }
};
constexpr int kLanes = 8;
constexpr size_t kBounce = (size_t)8 << 20;

struct BouncePool {
    BounceLane lane[kLanes];
    bool ready = false;
    ~BouncePool() { for (BounceLane &l : lane) l.release(); }      // (lane by lane, in order)
    bool init()
    {
        if (ready) return true;
        for (BounceLane &l : lane)
            if (!l.create(kBounce)) { for (BounceLane &x : lane) x.release(); return false; }      // nothing half-built is left behind
        ready = true;
        return true;
    }
};

// Run-length transfer of the result (host-array entries, deliver_runs): lanes that fetch the tables of a block of timesteps
// into their pinned buffers and expand them into the caller's array
constexpr int kRleLanes = 16;
constexpr size_t kRleBuf = (size_t)2 << 20;
struct RleBlock { int64_t t0, nt; uint32_t r0, nr; };          // timesteps [t0, t0 + nt), runs [r0, r0 + nr) of run_val
// The lanes' host threads, kept between calls (until round 5 every call started sixteen threads: ~0.45 ms of an 18.5 ms call, and 0.35 ms
// until the first tables arrived).  run(n, f) lets threads 0 .. n-1 execute f(i) and returns when all are done.
struct LaneCrew {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_go, cv_done;
    std::function<void(int)> job;
    uint64_t gen = 0;
    int want = 0, active = 0;
    bool stop = false;
    void loop(int i)
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv_go.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            if (i >= want) continue;
            std::function<void(int)> f = job;
            lk.unlock();
            f(i);
            lk.lock();
            if (--active == 0) cv_done.notify_one();
        }
    }
    bool run(int n, const std::function<void(int)> &f)
    {
        // (all n lanes or none: the job strides its blocks by the lane count it asked for -- with fewer threads the blocks of the
        // missing lanes would never be written; the caller falls back to the dense copy.  Round-5 advisor finding.)
        try { while ((int)th.size() < n) { const int i = (int)th.size(); th.emplace_back([this, i] { loop(i); }); } }
        catch (...) { return false; }
        {
            std::lock_guard<std::mutex> g(m);
            job = f; want = n; active = n; gen++;
        }
        cv_go.notify_all();
        std::unique_lock<std::mutex> lk(m);
        cv_done.wait(lk, [&] { return active == 0; });
        return true;
    }
    void shutdown()
    {
        { std::lock_guard<std::mutex> g(m); stop = true; }
        cv_go.notify_all();
        for (auto &t : th) if (t.joinable()) t.join();
        th.clear();
        stop = false;
    }
};
struct RlePool {
    BounceLane lane[kRleLanes];
    LaneCrew crew;
    bool ready = false;
    size_t cap = 0;                                 // bytes per buffer: kRleBuf, or one timestep's tables if those are larger
    ~RlePool() { crew.shutdown(); drop(); }         // (the lanes' threads stop before the lanes go, lane by lane in order)
    void drop() { for (BounceLane &l : lane) l.release(); ready = false; }
    bool init(size_t need)
    {
        if (ready && need <= cap) return true;
        drop();
        cap = std::max(kRleBuf, (need + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1));
        for (BounceLane &l : lane)
            if (!l.create(cap)) { drop(); return false; }
        ready = true;
        return true;
    }
};

// Source and sink of a streaming call.  Arrays (host_in / host_out) or callbacks that fill / drain pinned chunk buffers.
struct StreamIO {
    const void *host_in = nullptr;                 // (T, ny, nx) slab in host memory, or
    ctk_read_chunk_fn read = nullptr;              // reader of [t0, t0 + nt) into a pinned buffer
    void *read_user = nullptr;
    int32_t *host_out = nullptr;
    ctk_write_chunk_fn write = nullptr;
    void *write_user = nullptr;
    void *host_out_v = nullptr;                    // ctk_anom_stream_*: the sink holds values of the slab's type, as an array or
    ctk_write_values_fn write_v = nullptr;         // through a writer of values
    // a second slab that travels with the first, chunk by chunk (ctk_lifecycle_stream_*: the int32 flags beside the field): read before
    // the first, through the output side's buffers (io_out, pin_out), which such a call does not need otherwise; esz2 = 0: none
    const void *host_in2 = nullptr;
    ctk_read_chunk_fn read2 = nullptr;
    void *read2_user = nullptr;
    size_t esz2 = 0;
    const void *dev2 = nullptr;                    // where the second slab's chunk lies while `consume` runs
    bool ahead = false;                            // `consume` waits for its results on the host: chunk k+1 is sent off BEFORE chunk k is consumed
    int64_t chunk = 0;                             // timesteps per chunk
    size_t esz = 4;
    double ms_read = 0, ms_write = 0, ms_in = 0, ms_out = 0;
    int64_t passes_in = 0;                         // how often the input was streamed (2: the call had to re-read it)
};

// What a map family (level mean, reversal, local wave activity, subset, blockstat) remembers of its launches and what its ctk_debug_set_* hook
// overrides in the following ones
struct LaunchKnobs {
    int form = -1;                                 // kernel form of the last launch (-1: none yet)
    int64_t grid = 0;                              // ... and its workgroups
    int xcd_dbg = -1;                              // ctk_debug_set_*: xcd_chunk mode of the launches (-1: the plan's)
    int64_t grid_dbg = 0;                          // ... a lower cap on the workgroups of a launch (0: none)
    int64_t cap() const { return grid_dbg > 0 ? grid_dbg : CTK_LEVEL_GRID_MAX; }      // the cap to pass to the plan
    int xcd(int planned) const { return xcd_dbg >= 0 ? xcd_dbg : planned; }           // the xcd_chunk mode of a launch, given the plan's
    void launched(int f, int64_t g) { form = f; grid = g; }
};

// A slab that stays in HBM between calls (the field to track, the vertical mean): its buffer, the shape and type of what the buffer
// holds (T = -1: nothing) and a generation that says WHICH slab that is -- a caller that left one remembers the number and reads the
// slot only while it is unchanged.  The rule stands here and nowhere else: drop() BEFORE the buffer is overwritten, keep() AFTER the
// kernels that filled it have been synchronised, find() / held() before it is read.
struct ResidentSlab {
    DevBuf buf;
    int64_t T = -1; int ny = 0, nx = 0; bool f64 = false;
    uint64_t gen = 0;
    void drop() { T = -1; gen++; }                 // the slab, if any, is gone or about to be overwritten
    void keep(int64_t T_, int ny_, int nx_, bool f64_) { T = T_; ny = ny_; nx = nx_; f64 = f64_; }       // (the generation is the preceding drop()'s)
    bool held() const { return T >= 1 && buf.p; }
    void *find(int64_t T_, int ny_, int nx_, bool f64_) const                     // null: nothing of exactly this shape and type is held
    {
        return held() && T == T_ && ny == ny_ && nx == nx_ && f64 == f64_ ? buf.p : nullptr;
    }
    void report(int64_t *T_, int *ny_, int *nx_, int *is_f64) const               // the ctk_resident_* getters (T = -1: none)
    {
        if (T_) *T_ = T;
        if (ny_) *ny_ = ny;
        if (nx_) *nx_ = nx;
        if (is_f64) *is_f64 = f64 ? 1 : 0;
    }
    // the finished result in `other` becomes the slab (T_ < 1: none), `other` gets the old buffer as scratch
    void adopt(DevBuf &other, int64_t T_, int ny_, int nx_, bool f64_) { buf.swap(other); gen++; keep(T_ >= 1 ? T_ : -1, ny_, nx_, f64_); }
    void release() { buf.release(); drop(); }
};

// Every GPU resource below is an owner of ctk_own.h and goes with the handle: ctk_destroy names none of them.  Members are destroyed
// in reverse order of declaration, so the streams stay declared ahead of everything that is enqueued on them.
struct ctk_handle {
    int device = 0;
    int n_cus = 256;                              // compute units of the device (grids of the persistent kernels)
    Stream stream;
    Stream side[2];                                // the labelling variants of one shard run concurrently
    Stream copy_stream;                            // the streaming entries' copies (stream_setup)
    Event ev_fork, ev_join[2];
    Event ev_scan;                                // after the run scan of stage 1 (the host waits for it, not for the stream)
    State state = ST_IDLE;
    // geometry of the current shard
    int64_t T = 0;
    int ny = 0, nx = 0, W = 0, has_prev = 0, cmp_op = 0;
    int32_t wshift = 0, limb_bits = CTK_LIMB_BITS_MIN;
    uint32_t total_runs = 0, max_runs_step = 0, total_comps = 0;
    uint32_t pair_cap = 0, seam_cap = 0;
    bool need_glb = false;
    // device buffers
    DevBuf mask, wstart, rowstart, tcount, run_base, ncomp, cprefix, thr32, wlo, whi, counters;
    DevBuf run_comp, run_val, cs_mrep, cs_box, cs_area, d_mrep, d_box, d_area, comp_label;
    DevBuf g_x0, g_x1, g_y, g_parent, g_root, g_idmap, g_rs;
    DevBuf pairs, seams, ext, ops, op_first, op_next, op_stage, halo_in, halo_out, dbg;
    DevBuf seam_cnt, seam_off, d_seams, d_comp_t, pair_base, pair_cnt, rv_tdirty, d_blob, seam_rowoff;
    // device resolver work space
    DevBuf rv_prc, rv_prd, rv_pgc, rv_pgd, rv_F, rv_B, rv_keep0, rv_keep1, rv_changed, rv_parent, rv_isroot, rv_rank, rv_lab, rv_lab_root, rv_lbox,
        rv_bsum, rv_boff, rv_cand_cnt, rv_cand_off, rv_cand, rv_cand_scratch, rv_seam_res, rv_scalars, rv_mark, rv_inv, rv_ff, rv_dmap, rv_dorig, rv_dbox, rv_inex, rv_touch;
    // run_lifecycle reductions
    DevBuf lc_rows, lc_cnt, lc_wlo, lc_whi, lc_w, lc_work, lc_ovf, lc_ekeys, lc_offs, lc_sw, lc_sp, lc_out, lc_cross, lc_gtab, lc_occ, lc_cp;
    const int32_t *lc_flag = nullptr; const void *lc_field = nullptr;       // slabs of the last ctk_lifecycle_* call (for the exact rows)
    // ... which live in io_out / io_in (or an_slab) after a host-array call: lc_own 1, lc_own 2 with the resident anomaly slab as the field;
    // then ctk_lifecycle_exact reads them only while io_gen (and an_slab.gen) are what the call left.  0: the caller's own device pointers
    int lc_own = 0; uint64_t lc_io_gen = 0, lc_an_gen = 0;
    bool lc_f64 = false; int64_t lc_T = 0; int lc_ny = 0, lc_nx = 0;
    // which path the time steps of the last ctk_lifecycle_* call took (ctk_debug_lifecycle_path); lc_path_T < 0: no finished call
    int64_t lc_path_T = -1; CtkLifePlan lc_plan = {0, 0, 0, 0, 0};
    int64_t lc_given_up = 0, lc_fb_launches = 0; int lc_attempts = 0, lc_sort = 0;
    std::vector<uint8_t> lc_rounds;                // per time step: rounds of k_lifecycle it took part in
    bool lc_streamed = false;                      // the last call was ctk_lifecycle_stream_*: no slab is left for ctk_lifecycle_exact
    std::vector<int64_t> lx_idx;                   // ... the rows its pick chose (indices into lc_host) and their exact records
    std::vector<ctk_life_exact> lx_rec;
    DevBuf chunk_vals;                            // run values in the chunk order of k_relabel_v4
    // fused one-call path (ctk_seam_dev.hip): clusters of candidate labels, cluster root per group record; the pass runs without a
    // host hand-off and is validated from a device-written block of scalars after its only synchronisation
    DevBuf sd_parent, sd_tmin, sd_tmax, sd_root, sd_nops, sd_lbox, rv_pstate, ci_bsum, scan_bsum;
    uint32_t *h_amail = nullptr;                   // pinned: AsyncMail scalars (the typed view of amail_pin)
    PinBuf amail_pin;
    uint32_t op_cap_hint = 4096;                   // operation slots of the next fused pass (grows with what the passes needed)
    uint32_t nd_hint = 4096;                       // dense candidate labels of the last pass: grid of k_seam_driver
    int async_passes = 24;                         // filter passes the next fused pass launches.  Before any pass has said how long this kind of slab's
                                                   // removal cascades are: all that the one-launch form carries (an unneeded pass is one hop of its chain, ~0.3 us;
                                                   // the longest cascade grows with T -- 9 passes at 2707 steps, 11 at 438 000); then what the last pass needed + 2
    int use_async = -1;                            // -1: not decided (env CTK_ASYNC), 0 / 1
    int async_off_ny = -1, async_off_nx = -1;      // grid whose clusters did not fit the device seam driver: synchronous path from then on
    uint32_t fz_pslot = 0;                         // k_overlap wrote the pair records into fixed per-timestep slots of this size
    bool fz_init = false;                          // k_compact_init ran (the resolver arrays are initialised), k_overlap prepared the pair arrays
    bool in_one_call = false;                      // inside ctk_track_*_dev (the staged entries never take the fused path)
    bool guard_on = false;                         // kernels behind the resolver check the device counters before touching the tables
    // calc_anom / percentile (ctk_anom.hip): the resident field to track (anomalies, reversal index, wave activity), climatology, scratch
    ResidentSlab an_slab;
    DevBuf an_clim, an_raw, an_idx;
    DevBuf an_acc, an_valid;                       // ctk_anom_stream_*: float64 sums + int32 counts per (group, pixel); ctk_anom_seg_*: window-inside-segment per step
    int an_form = -1;                              // kernel form the last ctk_anom_seg_* / ctk_anom_stream_* call took (CtkAnomForm; -1: none yet)
    int64_t an_waves_dbg = 0, an_gy_dbg = 0;       // ctk_debug_set_anom: waves_wanted / grid_y_max of ctk_anom_plan for the launches (0: the rule's)
    int64_t an_last[6] = {0, 0, 0, 0, 0, 0};       // the last launch_anom_seg: tile, gx, gy, lds, o0, o1 ...
    int64_t an_launches = 0;                       // ... and how many of them the last ctk_anom_seg_* / ctk_anom_stream_* call made
    int64_t an_pct_n = -1;                         // an_raw holds the per-pixel quantiles of the last ctk_percentile_* call (-1: it does not)
    // vertical mean (ctk_level.hip): the resident mean slab in a buffer of its own (io_in is reused by every tracking call; its
    // generation changes with every ctk_level_mean_* call, every kept filter result and ctk_release_io), the table of weights and
    // level indices of the running call
    ResidentSlab lv_slab;
    DevBuf lv_tab;
    LaunchKnobs lv_knobs;                          // the k_level_mean launches (form: 1 vector, 0 scalar); ctk_debug_set_level
    // time filter (ctk_filter.hip): the table of the running call (K float64 weights, then one CtkFilterTap per output); the result of
    // a call that keeps it or reads the resident mean, which the slot then adopts (never filtered in place)
    DevBuf fl_tab, fl_out;
    int64_t fl_waves_dbg = 0, fl_gy_dbg = 0; int fl_form_dbg = -1;       // ctk_debug_set_filter: ctk_filter_plan's waves_wanted / grid_y_max / forced
    int64_t fl_last[8] = {-1, 0, 0, 0, 0, 0, 0, 0};                      // the last launch_filter: form, threads, tile, gx, gy, lds, o0, o1 ...
    int64_t fl_launches = 0;                                             // ... and how many of them the last ctk_filter_* call made
    // reversal of the meridional gradient (ctk_reversal.hip): the row table of the running call (four float64 and three int32 per row);
    // the k_reversal launches (form: 1 vector, 0 scalar) and ctk_debug_set_reversal
    DevBuf gr_tab;
    LaunchKnobs gr_knobs;
    // local wave activity (ctk_lwa.hip): the row table of the running call and the contours (steps, ny) of the last one; the
    // k_lwa_integral launches (form: 1 vector, 0 scalar) and ctk_debug_set_lwa, whose two numbers hold for k_lwa_contour too
    DevBuf lw_tab, lw_ref;
    LaunchKnobs lw_knobs;
    // selection of tracks or rows of a flag slab (ctk_subset.hip): the table of the running call (offsets, ids, bitmap words) and
    // its counters (the words n_selected is summed from, then one per entry); the k_subset launches (form: CTK_SUBSET_BITMAP ..
    // CTK_SUBSET_ROW_GLB of ctk_forms.h), whether the last one was vector or scalar, and ctk_debug_set_subset
    DevBuf sb_tab, sb_hits;
    LaunchKnobs sb_knobs;
    int sb_vec = 0;
    // per-block peak and extent (ctk_blockstat.hip): the accumulators of the running call (two 64-bit and six 32-bit words per entry
    // of the table, then the column bit sets) and its rows; the k_blockstat launches (form: CTK_BLOCKSTAT_ROW_LDS / _ROW_GLB of
    // ctk_forms.h), whether the last one was vector or scalar, and ctk_debug_set_blockstat.  The table itself is sb_tab: a call of
    // either family uploads its own.
    DevBuf bs_acc, bs_rows;
    LaunchKnobs bs_knobs;
    int bs_vec = 0;
    DevBuf io_in, io_out;                          // device copies of host-array calls (ctk_track_f32 / _f64)
    uint64_t io_gen = 0;                           // bumped by claim_io and ctk_release_io: WHOSE data io_in / io_out hold
    // streaming entries (ctk_track_stream_*): the slab passes through two chunk-sized device buffers per direction
    struct StreamIO *sio = nullptr;                // set for the duration of a streaming call: where the slab comes from
    Event ev_h2d[2], ev_thr[2], ev_rel[2], ev_d2h[2];
    PinPair pin_in, pin_out;
    double stream_ms[4] = {0, 0, 0, 0};
    std::unique_ptr<BouncePool> bounce;            // created on first use
    std::unique_ptr<RlePool> rle;                  // created on first use (deliver_runs)
    std::vector<uint32_t> rle_run_base;            // host copy of run_base (deliver_runs)
    std::vector<RleBlock> rle_blocks;
    bool rle_out = false;                          // this call's result leaves the device as run tables: launch_relabel is a no-op
    int rle_mode = -1;                             // ctk_set_result_transfer: -1 environment (CTK_RLE_OUT, default on), 0 dense copy, 1 runs, 2 runs wanted but made unavailable (test hook)
    // time-sharded path (ctk_sharded.hip)
    DevBuf sh_mask_next, sh_send, sh_recv, sh_prev, sh_elist, sh_ovr_slot, sh_ovr_val, sh_amb_list, sh_counts, sh_cl_shared, sh_cl_sent;
    uint32_t sh_stamp_seq = 0;
    int sh_dev_off_ny = -1, sh_dev_off_nx = -1;   // grid whose clusters did not fit the device seam driver on the time-shard path: host-driven from then on
    std::unique_ptr<ShardScratch, ShardScratchFree> shard;
    uint32_t *h_mail2 = nullptr;                   // pinned, device-written scalars (the typed view of mail2_pin)
    PinBuf mail2_pin;
    PinBuf h_shard, h_lab, h_seam;                 // pinned: gathered boundary records / label tables / shared seam groups
    bool halo_in_zero = false; void *halo_in_zero_p = nullptr; size_t halo_in_zero_cap = 0;     // the halo header of a first shard is already zero
    uint32_t sh_capB = 0, sh_capC = 0, sh_capD = 0;     // agreed capacities of the exchanged records (grow-only)
    int64_t sh_dbg[12] = {0};                     // ctk_debug_shard_exchange: what the last ctk_track_sharded_* call decided (CTK_SHX_*)
    bool sh_dbg_valid = false;
    std::vector<std::pair<int32_t, int32_t>> sh_pairs;
    bool halo_valid = false, halo_v2 = false;
    std::vector<ctk_life_row> lc_host, lc_tmp;
    std::vector<std::pair<uint64_t, uint32_t>> lc_keys;
    std::vector<uint32_t> lc_cnt_host;
    PinBuf h_cand;                   // pinned: candidates + boxes download
    PinBuf h_ops;                    // pinned: op upload staging
    PinBuf h_mail;                   // pinned: device-written mailbox of the resolver (scalars, candidates, dense tables)
    uint32_t *h_mail1 = nullptr;     // pinned, device-written: [0..3] run scan of stage 1, [8..9] alive ids / background written (the typed view of mail1_pin)
    PinBuf mail1_pin;
    PinBuf h_stage;                  // pinned: thresholds + weight limbs on their way to the device
    uint32_t rb_last = 0, rb_total = 0;   // run_base[T-1], run_base[T]
    // what the device copies of thresholds / weight limbs were made from
    std::vector<double> c_thr; std::vector<float> c_w;
    int64_t c_T = -1; bool c_f64 = false, c_thr_valid = false, c_w_valid = false; int c_cmp = -1, c_w_nx = -1;
    // threshold field (ctk_set_threshold_field): the caller's field as given (f32 / f64 [np][ny][nx]), plane of every step, the float32
    // field the float32 compare reads (the caller's own when it is float32, else prepared for fld_prep_op), the plane-major step order
    DevBuf fld_raw, fld_f32, fld_pos, fld_order;
    int64_t fld_T = -1, fld_np = 0; int fld_ny = 0, fld_nx = 0, fld_esz = 0;
    int fld_prep_op = -1;                        // op fld_f32 was prepared for (-1: not prepared)
    int64_t fld_order_chunk = -1;                // chunk length the order in fld_order was built for (steps sorted by plane inside each chunk)
    std::vector<int32_t> fld_pos_host, fld_order_host;
    // segment breaks (ctk_set_segments): the starts as given (empty: none), the per-step edge table of the last T it was built for
    // (bit 0 first step of a segment, bit 1 last step; host copy for the host resolver) and, during a one-call track, the device
    // table the filter and overlap launches take (nullptr: no segments -- the unsegmented kernels)
    std::vector<int64_t> seg_starts;
    DevBuf seg_edge;
    std::vector<uint8_t> seg_edge_host;
    int64_t seg_edge_T = -1;
    const uint8_t *seg_cur = nullptr;
    // ... and its host twin, indexed like seg_cur (the host resolver; a time shard reads the bits of its first and last step from it)
    const uint8_t *seg_cur_host = nullptr;
    // segment starts given to the running call as an argument (ctk_track_stream_seg_*; empty: none): every pass of that call
    // -- the dense re-run too -- builds its table from them
    std::vector<int64_t> seg_call;
    bool seg_shard_breaks = false;                       // a time-shard call with more than one segment (every rank alike) is running
    // blocking frequency (ctk_freq.hip): counts of the host entries, group ids; experiments (ctk_debug_set_freq)
    DevBuf fq_counts, fq_group;
    // blocked spells (ctk_spell.hip): the three maps of the host entries, the per-step words (group id, bit 31: segment start) and
    // their host copy, the two per-pixel carries; the test hook's slice (ctk_debug_set_spell; 0: the rule of ctk_time_slice)
    DevBuf sp_out, sp_words, sp_carry;
    std::vector<uint32_t> sp_words_host;
    int64_t sp_slice_dbg = 0;
    // composite over flagged steps (ctk_composite.hip): float64 sums and uint32 counts of the host entries; the test hook's batch
    // (ctk_debug_set_composite; -1: the rule of ctk_composite_plan), the batch and the workgroups of the last launch
    DevBuf cp_sum, cp_n;
    int cp_unroll_dbg = -1, cp_unroll = 0; int64_t cp_grid = 0;
    // block-centred composite (ctk_centred.hip): sums and counts of the host entries; the stamps in bin order with the bin offsets of
    // every chunk; the test hook's form, batch and workgroup width (ctk_debug_set_centred; -1: the rule of ctk_centred_plan), those of
    // the last launch and its workgroups
    DevBuf ce_sum, ce_n, ce_idx;
    int ce_form_dbg = -1, ce_unroll_dbg = -1, ce_threads_dbg = -1, ce_form = 0, ce_unroll = 0, ce_threads = 0; int64_t ce_grid = 0;
    // reductions over space per step (ctk_band.hip): the column tables and the sector tables of one chunk, the weights and sectors of
    // the running call; the test hook's form and batch of rows (ctk_debug_set_band; -1: the rule of ctk_band_plan), those of the last
    // launch (form -1: none yet) and its workgroups
    DevBuf bd_cols, bd_sec, bd_tab;
    int bd_form_dbg = -1, bd_rows_dbg = -1, bd_form = -1, bd_rows = 0; int64_t bd_grid = 0;
    PinPair bd_pin;                               // pinned twins of the two table sets of a streamed call
    // percentile per group (ctk_pctl.hip): histograms per (day, distinct prefix); ranks, prefixes, lists, ids; band sweeps of the last call
    DevBuf pc_hist, pc_buf;
    int64_t pc_sweeps = 0;
    int pc_groups = 0; size_t pc_slots = 0;        // the last ctk_percentile_groups_* launch: G and the histogram slots, which fix pc_buf's layout (0: none yet)
    // percentile field (ctk_pfield.hip): the G planes of the last call; pool starts, pool lengths, the step list; its form and longest pool
    DevBuf pf_out, pf_idx;
    int pf_form = -1; int64_t pf_max_pool = 0;
    // standard-deviation field (ctk_std.hip): the planes of the last call (std, mean, counts); group ids and pool lengths; its tile and longest pool
    DevBuf sf_out, sf_idx;
    int sf_tile = -1; int64_t sf_max_pool = 0;
    int64_t fq_slice_dbg = 0; int fq_nt = -1;
    int w_minlsb = 0;                            // lowest set bit over the integer row weights
    int64_t last_alive = 0, last_nlab = 0;
    int64_t rowoff_T = -1; int rowoff_ny = -1; void *rowoff_p = nullptr;     // what seam_rowoff currently holds
    // speculative launch of the 2-D labelling: capacity (in runs) of the run-indexed buffers, the previous call's variants
    uint32_t runs_cap = 0;
    CtkVariantSet spec_set = {false, false, false, false, false, false};
    int spec_ny = -1, spec_nx = -1; int64_t spec_T = -1;
    size_t mail_cap_c = 0, mail_cap_d = 0, mail_want_c = 0, mail_want_d = 0;
    const int32_t *d_op_next = nullptr;
    int use_device_resolve = 1;
    int filter_round = CTK_JACOBI_ROUND;          // filter passes launched before convergence is checked
    uint32_t debug_pair_cap = 0;                  // test hook: pretend the pair table holds only this many records
    uint32_t debug_mail_c = 0, debug_mail_d = 0;  // test hook: pretend the resolver mailbox holds only this many records / labels
    int debug_sd_lab = 0, debug_sd_ops = 0;       // test hook: labels / operations per cluster the device seam driver accepts
    int debug_fail_stage = 0;                     // test hook (ctk_debug_fail_at): the time-shard path fails at this stage, once
    int64_t debug_sh_gops = 0;                    // test hook (ctk_debug_set_shared_ops_reserve): shared-cluster operations the device form takes
    // bounded inter-workgroup waits of the systolic filter kernels (ResolveDev::spin_limit): ticks of the 100 MHz wall clock after
    // which a wait gives up; no_sys: a wait did give up on this handle -- one launch per filter pass (no waits) from then on
    uint64_t spin_limit = CTK_SPIN_LIMIT_TICKS;
    int debug_stall = 0;                          // test hook (ctk_debug_set_spin): the first workgroup of the chain is late (1) / never publishes (2)
    bool no_sys = false, sh_retrying = false;
    int small_threads[3] = {0, 0, 0};              // experiments (ctk_debug_set_small_threads): threads of k_extent / k_run_values / k_compact_init, 0 = default
    bool thr_nostore = false;                     // the threshold kernel without its mask stores: the yardstick of the mask placement check
    bool thr_probe = false;                       // the launches of that check run under their own kernel name (k_threshold_probe)
    bool rel_probe = false;                       // ... and those of the write kernel's chunk -> XCD timing (k_relabel_probe)
    int rel_variant = -1;                         // ctk_debug_time_relabel: 0 k_relabel_v5, 1 the same without the SGPR limit (-1: the default's rules)
    bool mask_check_pending = false;              // the mask was (re)allocated and has not been checked against a slab yet
    int mask_check_retries = 0;                   // checks that found the device busy with other work (their times meant nothing)
    int mask_tries = 0; double mask_ratio = 0.0;  // allocations of the mask that were checked when it was last (re)allocated; kernel time / its time without stores
    double mask_check_ms = 0; double mask_spacer_gb = 0;        // host time / spacer memory held by the last mask placement check
    int xcd_rel_tuned = -1;                       // chunk -> XCD mapping of the write kernel (xcd_chunk, tune_relabel) for the shape below; -1: launch order
    int64_t rel_tuned_T = -1; int rel_tuned_ny = 0, rel_tuned_nx = 0; const void *rel_tuned_flag = nullptr;
    int64_t rel_seen_T = -1; int rel_seen_ny = 0, rel_seen_nx = 0;      // the shape of the previous pass (tuning waits for the second pass on a shape)
    bool sh_collective_err = false;               // the time-shard path's error was decided identically on every rank
    ctk_comm *active_comm = nullptr;              // set while the time-shard path runs with more than one rank
    // host scratch of the seam driver, kept between calls (fresh 100+ KB vectors would page-fault every call)
    SeamDriver sd, sd_glob;                       // sd_glob: candidate groups shared between time shards (ctk_sharded.hip)
    std::vector<int32_t> sd_last;
    std::vector<CtkOp> sd_ops;
    std::vector<unsigned char> sd_cand;
    int64_t stats[CTK_NSTATS_ALL] = {0};
    double ms_sum[CTK_NTIMERS] = {0};                  // HIP-event times of the kernel groups summed over the calls since the last reset
    int64_t ms_cnt[CTK_NTIMERS] = {0};                 // ... and how many calls measured each group (ctk_get_timing_sums)
    // host (pinned) buffers
    PinBuf h_blob;
    size_t h_blob_bytes = 0;
    PinBuf h_small;                  // pinned scratch: counters, run_base download
    // results kept between extents and write
    int64_t n_labels = 0, t_begin = 0;
    int32_t nops = 0;
    // timing
    int timing = 0;
    uint64_t pass_no = 0;                        // stage-1 launches so far (level-1 timing alternates between the two streaming kernels)
    Event ev[CTK_K_COUNT + 2][2];                // + one internal pair: stage-1 row count / run scan, reported inside CTK_K_SCAN
    bool ev_used[CTK_K_COUNT + 2];
    double ms[CTK_NTIMERS];
    bool ev_ready = false;
};

namespace {

int ensure(ctk_handle *h, DevBuf &b, size_t need)
{
    if (need == 0) need = 8;
    if (b.cap >= need) return CTK_OK;
    // hipFree waits for the device: with a collective in flight that wait must be the communicator's guarded one
    if (b.p && h && h->active_comm) { if (int rc = ctk_comm_wait(h->active_comm)) return rc; }
    b.release();
    hipError_t e = b.alloc(need + need / 8 + 256);        // a little head room: sizes vary between calls
    if (e != hipSuccess) e = b.alloc(need);
    if (e != hipSuccess) return ctk_set_error(CTK_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", need, hipGetErrorString(e));
    return CTK_OK;
}

// non_coherent: coarse-grained pinned memory -- cached on the CPU (the default, fine-grained mapping makes CPU
// reads several times slower); its contents are valid for the host after a stream synchronisation.
int ensure_host(ctk_handle *h, PinBuf &b, size_t need, bool non_coherent = false)
{
    if (b.cap >= need && b.p) return CTK_OK;
    if (b.p && h && h->active_comm) { if (int rc = ctk_comm_wait(h->active_comm)) return rc; }      // (hipHostFree waits for the device, as hipFree does)
    b.release();
    const size_t c = need + need / 4 + 4096;
    const hipError_t e = b.alloc(c, non_coherent ? hipHostMallocNonCoherent : hipHostMallocDefault);
    if (e != hipSuccess) return ctk_set_error(CTK_E_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", c, hipGetErrorString(e));
    return CTK_OK;
}

struct ActiveComm {                        // scope of ctk_handle::active_comm
    ctk_handle *h;
    ActiveComm(ctk_handle *h_, ctk_comm *c) : h(h_) { h->active_comm = (c && c->world > 1) ? c : nullptr; }
    ~ActiveComm() { h->active_comm = nullptr; }
};

// every entry that writes io_in / io_out takes them through here: what an earlier call left in them is no longer that call's
static int claim_io(ctk_handle *h, DevBuf &b, size_t need)
{
    h->io_gen++;
    return ensure(h, b, need);
}

template <typename T>
T *P(const DevBuf &b) { return (T *)b.p; }
// component prefix of the shard's timesteps; CPX(h)[-1] = 0 is where the components of the previous shard's last timestep
// (the halo of the time-sharded path) start, CPX(h)[0] their number
inline uint32_t *CPX(const ctk_handle *h) { return (uint32_t *)h->cprefix.p + 1; }

struct Timer {
    ctk_handle *h;
    int k;
    // level 1: only the two pixel-streaming kernels carry events (an event record is a command of its own, ~5 us on
    // the stream: twenty of them would stretch the pass they are supposed to measure); level 2: every group
    // (level 1 times ONE of the two in every second pass -- k_threshold in passes 0, 4, 8 ... of the handle, k_relabel in passes
    // 2, 6, 10 ...: one event pair per two passes; a pair around k_relabel showed as two 6 us bubbles in the kernel timeline)
    bool on() const
    {
        return h->ev_ready && (h->timing >= 2 || (h->timing == 1 && ((k == CTK_K_THRESHOLD && (h->pass_no & 3) == 0) || (k == CTK_K_RELABEL && (h->pass_no & 3) == 2))));
    }
    Timer(ctk_handle *h_, int k_) : h(h_), k(k_)
    {
        if (on()) { (void)hipEventRecord(h->ev[k][0], h->stream); }
    }
    ~Timer()
    {
        if (on()) { (void)hipEventRecord(h->ev[k][1], h->stream); h->ev_used[k] = true; }
    }
};

// float32 threshold such that the float32 compare `x <op> thr32` equals `(double)x <op> thr`
float adjust_threshold(double thr, int op)
{
    if (thr != thr) return __builtin_nanf("");
    float f = (float)thr;
    if (op == 0 || op == 3) {                // x >= thr  <=>  x >= ceil32(thr);  x < thr <=> x < ceil32(thr)
        if ((double)f < thr) f = std::nextafterf(f, INFINITY);
    } else {                                 // x <= thr  <=>  x <= floor32(thr); x > thr <=> x > floor32(thr)
        if ((double)f > thr) f = std::nextafterf(f, -INFINITY);
    }
    return f;
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
static void stream_teardown(ctk_handle *h)
{
    for (int b = 0; b < 2; b++) {
        h->pin_in.b[b].release(); h->pin_out.b[b].release();
        for (Event *e : {&h->ev_h2d[b], &h->ev_thr[b], &h->ev_rel[b], &h->ev_d2h[b]}) e->release();
    }
    h->copy_stream.release();
}

extern "C" int ctk_version(void) { return 100; }

extern "C" int ctk_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { ctk_set_error(CTK_E_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); return 0; }
    return n;
}

extern "C" int ctk_create(ctk_handle **out, int device)
{
    if (!out) return ctk_set_error(CTK_E_INVALID, "ctk_create: null handle pointer");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return ctk_set_error(CTK_E_NODEVICE, "ctk_create: no HIP device available (%s) -- the HIP path has no CPU fallback",
                             e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return ctk_set_error(CTK_E_INVALID, "ctk_create: device %d out of range (0..%d)", device, n - 1);
    HIPCHK(hipSetDevice(device));
    ctk_handle *h = new (std::nothrow) ctk_handle();
    if (!h) return ctk_set_error(CTK_E_NOMEM, "ctk_create: out of memory");
    h->device = device;
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) h->n_cus = cu; }
    if (h->stream.create(hipStreamNonBlocking) != hipSuccess) { delete h; return ctk_set_error(CTK_E_NODEVICE, "hipStreamCreate failed"); }
    for (int k = 0; k < 2; k++) {
        if (h->side[k].create(hipStreamNonBlocking) != hipSuccess || h->ev_join[k].create(hipEventDisableTiming) != hipSuccess) { ctk_destroy(h); return ctk_set_error(CTK_E_NODEVICE, "hipStreamCreate failed"); }
    }
    if (h->ev_fork.create(hipEventDisableTiming) != hipSuccess || h->ev_scan.create(hipEventDisableTiming) != hipSuccess) { ctk_destroy(h); return ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed"); }
    if (h->mail1_pin.alloc(256, hipHostMallocDefault) != hipSuccess) { ctk_destroy(h); return ctk_set_error(CTK_E_NOMEM, "hipHostMalloc failed"); }
    h->h_mail1 = (uint32_t *)h->mail1_pin.p;
    memset(h->h_mail1, 0, 256);
    memset(h->ms, 0, sizeof(h->ms));
    memset(h->ev_used, 0, sizeof(h->ev_used));
    *out = h;
    return CTK_OK;
}

extern "C" void ctk_destroy(ctk_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    h->rle.reset();                                // the lanes' host threads stop before any buffer goes
    h->bounce.reset();
    delete h;
}

extern "C" int ctk_set_timing(ctk_handle *h, int enable)
{
    if (!h || enable < 0 || enable > 2) return ctk_set_error(CTK_E_INVALID, "ctk_set_timing: null handle or level not in 0..2");
    HIPCHK(hipSetDevice(h->device));
    if (enable && !h->ev_ready) {
        for (int k = 0; k <= CTK_KI_ROWCOUNT; k++) { HIPCHK(h->ev[k][0].create()); HIPCHK(h->ev[k][1].create()); }
        h->ev_ready = true;
    }
    h->timing = enable;
    return CTK_OK;
}

#ifdef CTK_PHASE_TIMING
extern "C" int ctk_debug_phase_times(unsigned long long *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_t), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -1;
}
extern "C" int ctk_debug_rel_times(unsigned long long *out)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rel_t), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -1;
}
extern "C" int ctk_debug_rel_acc(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rel_acc), sizeof(unsigned long long) * 4096) != hipSuccess) return -1;
    if (reset) { std::vector<unsigned long long> z(4096, 0ull); if (hipMemcpyToSymbol(HIP_SYMBOL(g_rel_acc), z.data(), 4096 * 8) != hipSuccess) return -1; }
    return 0;
}
// k_rs_pass_blk's per-workgroup stamps; reset != 0 re-arms them (entry = ~0 for the atomicMin, the rest 0)
extern "C" int ctk_debug_pb_times(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pb_t), sizeof(unsigned long long) * 4096) != hipSuccess) return -1;
    if (reset) {
        std::vector<unsigned long long> z(4096, 0ull);
        for (int i = 0; i < 1024; i++) z[4 * i] = ~0ull;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_pb_t), z.data(), sizeof(unsigned long long) * 4096) != hipSuccess) return -1;
    }
    return 0;
}
#endif

extern "C" int ctk_get_stats(ctk_handle *h, int64_t *out)
{
    if (!h || !out) return ctk_set_error(CTK_E_INVALID, "null argument");
    memcpy(out, h->stats, (size_t)CTK_NSTATS * sizeof(int64_t));      // (frozen length; newer entries: ctk_get_stats_n)
    return CTK_OK;
}
extern "C" int ctk_get_stats_n(ctk_handle *h, int64_t *out, int n)
{
    if (!h || !out || n < 0) return ctk_set_error(CTK_E_INVALID, "null argument");
    memcpy(out, h->stats, (size_t)std::min(n, CTK_NSTATS_ALL) * sizeof(int64_t));
    return CTK_OK;
}

extern "C" int ctk_debug_set_pair_capacity(ctk_handle *h, uint32_t records)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->debug_pair_cap = records;
    return CTK_OK;
}

extern "C" int ctk_debug_set_mailbox(ctk_handle *h, uint32_t cand_records, uint32_t labels)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->debug_mail_c = cand_records; h->debug_mail_d = labels;
    return CTK_OK;
}

extern "C" int ctk_debug_set_seam_caps(ctk_handle *h, int labels, int ops)
{
    if (!h || labels < 0 || ops < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_seam_caps: null handle or negative capacity");
    h->debug_sd_lab = labels; h->debug_sd_ops = ops;
    h->async_off_ny = -1; h->async_off_nx = -1;          // (a grid that was sent to the host driver gets another try)
    h->sh_dev_off_ny = -1; h->sh_dev_off_nx = -1;
    return CTK_OK;
}

extern "C" int ctk_debug_set_small_threads(ctk_handle *h, int extent, int run_values, int compact_init)
{
    for (int v : {run_values, compact_init}) if (v != 0 && v != 64 && v != 128 && v != 256) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_small_threads: 0 / 64 / 128 / 256");
    if (extent != 0 && extent != 64 && extent != 128 && extent != 256 && extent != 1024) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_small_threads: extent 0 / 64 / 128 / 256, or 1024 = k_extent_blk");
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->small_threads[0] = extent; h->small_threads[1] = run_values; h->small_threads[2] = compact_init;
    return CTK_OK;
}

/* measurement support: the write kernel launched `reps` times on the finished tables of the last one-call pass (it writes the same flags again),
 * every launch timed by events -> ms[reps].  variant: 0 k_relabel_v5, 1 the same without its SGPR limit; xcd: chunk -> XCD order
 * (0 launch order, 1 one eighth of the launch per XCD, 16 tiles of 16; -1: what the handle uses) */
static int launch_relabel(ctk_handle *h, int persistence, int32_t *flag_dev, bool with_fold, const int32_t *chunk_vals = nullptr, int64_t t0 = 0, int64_t nt = -1);
static int32_t *chunk_vals_for(ctk_handle *h, const int32_t *flag_dev, int *rows);
extern "C" int ctk_debug_time_relabel(ctk_handle *h, int32_t *flag_dev, int persistence, int variant, int xcd, int reps, double *ms)
{
    if (!h || !flag_dev || !ms || reps < 1 || variant < 0 || variant > 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_relabel: bad argument");
    if (h->state != ST_TABLES) return ctk_set_error(CTK_E_STATE, "ctk_debug_time_relabel needs a finished pass");
    HIPCHK(hipSetDevice(h->device));
    Event e0, e1;
    HIPCHK(e0.create());
    if (e1.create() != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed");
    int rows = 0;
    const int32_t *cv = chunk_vals_for(h, flag_dev, &rows);
    const int keep_variant = h->rel_variant, keep_xcd = h->xcd_rel_tuned;
    h->rel_variant = variant;
    if (xcd >= 0) h->xcd_rel_tuned = xcd;
    int rc = CTK_OK;
    hipError_t err = hipSuccess;
    for (int r = 0; r < reps && rc == CTK_OK && err == hipSuccess; r++) {
        err = hipEventRecord(e0, h->stream);
        rc = launch_relabel(h, persistence, flag_dev, true, cv, 0, -1);
        if (err == hipSuccess) err = hipEventRecord(e1, h->stream);
        if (err == hipSuccess) err = hipEventSynchronize(e1);
        float f = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&f, e0, e1);
        ms[r] = f;
    }
    h->rel_variant = keep_variant; h->xcd_rel_tuned = keep_xcd;
    if (rc != CTK_OK) return rc;
    if (err != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "ctk_debug_time_relabel: %s", hipGetErrorString(err));
    return CTK_OK;
}

// what ctk_forms.h decides, for the tests (include/contrack_hip_debug.h); no handle, no device
extern "C" int ctk_debug_forms(const ctk_form_query *q, ctk_form_plan *p)
{
    if (!q || !p) return ctk_set_error(CTK_E_INVALID, "ctk_debug_forms: null argument");
    if (q->T < 0 || q->nt < 0 || q->ny < 1 || q->nx < 1 || q->ny > 65535 || q->nx > 65535 || q->path < 0 || q->path > 2)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_forms: bad query (T=%lld nt=%lld ny=%lld nx=%lld path=%lld)", (long long)q->T, (long long)q->nt, (long long)q->ny,
                             (long long)q->nx, (long long)q->path);
    const int64_t T = q->T;
    const int ny = (int)q->ny, nx = (int)q->nx, W = (nx + 63) / 64;
    const CtkPath path = (CtkPath)q->path;
    auto set_of = [](int64_t b) { return CtkVariantSet{(b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, (b & 32) != 0}; };
    auto bits_of = [](const CtkVariantSet &v) { return (int64_t)((v.v1 ? 1 : 0) | (v.v2 ? 2 : 0) | (v.v3 ? 4 : 0) | (v.glb ? 8 : 0) | (v.one ? 16 : 0) | (v.v1hi ? 32 : 0)); };
    memset(p, 0, sizeof(*p));
    const CtkThrForm tf = ctk_threshold_form(q->nt, ny, nx, W, q->f64 != 0, q->aligned16 != 0, q->field != 0);
    p->thr_kind = tf.kind; p->thr_u7 = tf.u7; p->thr_rbt = tf.rbt; p->thr_grid = tf.grid;
    p->rowcount_threads = ctk_rowcount_threads(T, ny, W);
    const CtkLabelShape sh = ctk_label_shape(T, ny, W);
    p->v0b = sh.v0b; p->v0_ok = sh.v0_ok; p->v0_runs = sh.v0_runs;
    p->need_glb = ctk_label_need_glb((uint32_t)q->max_runs_step, ny);
    const CtkVariantSet sl = ctk_label_speculative(set_of(q->spec_set), sh);
    p->spec_launched = bits_of(sl); p->spec_bits = ctk_label_form_bits(sl, sh);
    const CtkLabelPlan lp = ctk_label_plan(T, ny, sh, (uint32_t)q->max_runs_step, set_of(q->launched));
    p->missing = bits_of(lp.missing); p->missing_bits = ctk_label_form_bits(lp.missing, sh); p->next_spec = bits_of(lp.next);
    p->overlap_form = ctk_overlap_form(T, ny, W) + (q->seg ? CTK_OVERLAP_SEG : 0);
    p->extent_form = ctk_extent_form(T, nx, (int)q->forced_extent);
    const CtkWritePlan wp = ctk_write_plan(T, q->nt, ny, nx, W, q->aligned16 != 0);
    p->write_kernel = wp.kernel; p->write_rb = wp.rb; p->write_sub = wp.sub; p->write_kb = wp.kb; p->write_batched = wp.tab_batched;
    p->write_lds = (int64_t)wp.lds; p->write_grid = wp.grid; p->write_shape = wp.shape;
    p->chunk_copy = ctk_write_chunk_copy(ctk_write_plan(T, T, ny, nx, W, q->aligned16 != 0));
    p->runval_threads = ctk_runval_threads(path, T, (uint64_t)q->total_runs, (int)q->forced_run_values);
    p->compact_init_threads = ctk_compact_init_threads(path, T, (int)q->forced_compact_init);
    p->count_staged = ctk_count_form_staged(q->n_labels);
    const CtkFilterPlan fp = ctk_filter_plan_fused(T, (int)q->async_passes, q->no_sys != 0, (int)q->n_cus, q->seg != 0, (int)q->pslot,
                                                   ctk_rank_blocks((size_t)q->total_runs));
    p->count_fused = ctk_count_form_fused(q->last_nlab, fp.passes);
    p->filter_sys = fp.sys; p->filter_passes = fp.passes; p->filter_blk = fp.round.blk; p->filter_two_pc = fp.round.two_pc; p->filter_nb = fp.round.nb;
    p->filter_unite = fp.unite; p->filter_merged = fp.merged; p->filter_bits = fp.bits; p->filter_bits_sync = ctk_filter_bits_sync(T, q->seg != 0);
    const CtkFilterRound fr = ctk_filter_round(T, (int)q->async_passes, q->no_sys != 0, (int)q->n_cus);
    p->round_blk = fr.blk; p->round_two_pc = fr.two_pc; p->round_nb = fr.nb;
    p->rowcount_groups = ctk_rowcount_groups((int)p->rowcount_threads, ny, W);
    return CTK_OK;
}

// device buffers, pinned buffers, events and streams the owners of ctk_own.h hold in this process; no handle, no device
extern "C" int ctk_debug_live(int64_t *out4)
{
    if (!out4) return ctk_set_error(CTK_E_INVALID, "ctk_debug_live: null argument");
    for (int i = 0; i < CTK_LIVE_KINDS; i++) out4[i] = g_ctk_live[i].load();
    return CTK_OK;
}

// capacities in bytes of the staging buffers every host-array and streamed entry shares: io_in, io_out, one buffer of the pin_in pair, one
// of the pin_out pair (0: not allocated, or released by ctk_release_io).  No device call.
extern "C" int ctk_debug_io_bytes(ctk_handle *h, int64_t *out4)
{
    if (!h || !out4) return ctk_set_error(CTK_E_INVALID, "ctk_debug_io_bytes: null argument");
    out4[0] = (int64_t)h->io_in.cap; out4[1] = (int64_t)h->io_out.cap; out4[2] = (int64_t)h->pin_in.cap(); out4[3] = (int64_t)h->pin_out.cap();
    return CTK_OK;
}

extern "C" int ctk_debug_set_spin(ctk_handle *h, double limit_ms, int stall_mode)
{
    if (!h || stall_mode < 0 || stall_mode > 2 || limit_ms < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_spin: null handle, negative limit or stall mode not in 0..2");
    h->spin_limit = limit_ms > 0 ? (uint64_t)(limit_ms * 1e5) : CTK_SPIN_LIMIT_TICKS;      // 100 MHz wall clock
    h->debug_stall = stall_mode;
    h->no_sys = false;                                   // (a handle that gave up gets another try)
    return CTK_OK;
}

extern "C" int ctk_set_filter_round(ctk_handle *h, int passes)
{
    if (!h || passes < 1 || passes > 32) return ctk_set_error(CTK_E_INVALID, "ctk_set_filter_round: 1..32 passes per round");
    h->filter_round = passes;
    h->async_passes = passes;                            // (the fused pass launches this many; it adapts from there)
    return CTK_OK;
}

extern "C" int ctk_set_result_transfer(ctk_handle *h, int mode)
{
    if (!h || mode < -1 || mode > 2) return ctk_set_error(CTK_E_INVALID, "ctk_set_result_transfer: mode -1 (environment), 0 (dense copy), 1 (run tables) or 2 (test hook: run tables made unavailable)");
    h->rle_mode = mode;
    return CTK_OK;
}

extern "C" int ctk_set_fused_pass(ctk_handle *h, int enable)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->use_async = enable ? 1 : 0;
    return CTK_OK;
}

extern "C" int ctk_set_device_resolve(ctk_handle *h, int enable)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->use_device_resolve = enable ? 1 : 0;
    return CTK_OK;
}

static int collect_event_times(ctk_handle *h)
{
    if (!h->timing || !h->ev_ready) return CTK_OK;
    for (int k = 0; k <= CTK_KI_ROWCOUNT; k++) {
        if (!h->ev_used[k]) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev[k][0], h->ev[k][1]) == hipSuccess) {
            const int kk = k == CTK_KI_ROWCOUNT ? CTK_K_SCAN : k;
            h->ms[kk] += ms;
            h->ms_sum[kk] += ms; h->ms_cnt[kk]++;              // (running sums: a caller that times many passes reads them once)
        }
        h->ev_used[k] = false;
    }
    return CTK_OK;
}

extern "C" int ctk_get_timing_sums(ctk_handle *h, double *sums, int64_t *counts, int reset)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (sums) memcpy(sums, h->ms_sum, sizeof(h->ms_sum));
    if (counts) memcpy(counts, h->ms_cnt, sizeof(h->ms_cnt));
    if (reset) { memset(h->ms_sum, 0, sizeof(h->ms_sum)); memset(h->ms_cnt, 0, sizeof(h->ms_cnt)); }
    return CTK_OK;
}

extern "C" int ctk_get_timings(ctk_handle *h, double *ms)
{
    if (!h || !ms) return ctk_set_error(CTK_E_INVALID, "null argument");
    memcpy(ms, h->ms, sizeof(h->ms));
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// stage 1
// ------------------------------------------------------------------------------------------------
static int stream_in(ctk_handle *h, bool f64, int64_t T, int ny, int nx, const std::function<int(const void *, int64_t, int64_t)> &consume);
static int stream_out(ctk_handle *h, int persistence, const int32_t *chunk_vals);

// what ctk_stream_timings reports: the reader, the writer, the input side and the output side of the streamed call `io`
static void stream_ms_set(ctk_handle *h, const StreamIO &io)
{
    h->stream_ms[0] = io.ms_read; h->stream_ms[1] = io.ms_write; h->stream_ms[2] = io.ms_in; h->stream_ms[3] = io.ms_out;
}

// A read-only pass over a streamed slab (the map consumers, the climatology pass, the life cycle): `io` is the handle's source while
// stream_in runs and on no path longer, the handle gets the pass's stream timings, and a failed chunk -- a reader that gave up -- leaves
// nothing of the call in flight: a chunk may still be on its way into a buffer.  A pass that succeeds is not waited for here.
static int stream_consume(ctk_handle *h, StreamIO &io, bool f64, int64_t T, int ny, int nx, const std::function<int(const void *, int64_t, int64_t)> &consume)
{
    struct Sio { ctk_handle *h; ~Sio() { h->sio = nullptr; } } sio{h};
    h->sio = &io;
    const int rc = stream_in(h, f64, T, ny, nx, consume);
    stream_ms_set(h, io);
    if (rc != CTK_OK) {
        if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamSynchronize(h->stream);
    }
    return rc;
}

// A kernel alone between HIP events on the handle's stream (the ctk_debug_time_* hooks of the probes in tools/): one untimed launch,
// then `reps` launches between reps + 1 events; ms2 = {best, mean} per launch.  The stream is idle and the events are gone when it
// returns, also after an error; `who` names the hook in the error text.
static int time_launches(ctk_handle *h, const char *who, int reps, double *ms2, const std::function<int()> &launch)
{
    std::vector<Event> ev((size_t)reps + 1);
    struct Idle { hipStream_t s; ~Idle() { (void)hipStreamSynchronize(s); } } idle{h->stream};       // (declared after the events: it runs before they go)
    for (Event &e : ev)
        if (e.create() != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed");
    CTKCHK(launch());                                                               // (warm-up)
    for (int r = 0; r < reps; r++) {
        if (hipEventRecord(ev[r], h->stream) != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        CTKCHK(launch());
    }
    if (hipEventRecord(ev[reps], h->stream) != hipSuccess || hipEventSynchronize(ev[reps]) != hipSuccess)
        return ctk_set_error(CTK_E_NODEVICE, "%s: event wait failed", who);
    double best = 1e30, sum = 0;
    for (int r = 0; r < reps; r++) {
        float m = 0;
        (void)hipEventElapsedTime(&m, ev[r], ev[r + 1]);
        best = std::min(best, (double)m); sum += m;
    }
    ms2[0] = best; ms2[1] = sum / reps;
    return CTK_OK;
}

// The yardstick of the map families' ctk_debug_time_* hooks: k_copy16 over the whole 16-byte words of two 16-byte aligned buffers of
// `bytes` bytes, timed as above, in the workgroup order a family's launch of this size takes (its ctk_debug_set_* mode included)
static int time_copy16(ctk_handle *h, const char *who, const LaunchKnobs &k, const void *src, void *dst, int64_t bytes, int reps, double *ms2)
{
    const int64_t n16 = bytes / 16;
    const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((n16 + 255) / 256, 1), CTK_LEVEL_GRID_MAX);
    const int xcd = k.xcd(grid >= CTK_LEVEL_XCD_MIN ? 1 : 0);
    return time_launches(h, who, reps, ms2, [&]() -> int {
        k_copy16<<<grid, 256, 0, h->stream>>>((const i32x4 *)src, (i32x4 *)dst, n16, xcd);
        HIPCHK(hipGetLastError());
        return CTK_OK;
    });
}

// the bodies of the map families' ctk_debug_set_* and two-word ctk_debug_*_form hooks; k: the family's record in the handle
static int knobs_set(const char *who, ctk_handle *h, LaunchKnobs ctk_handle::*k, int xcd_mode, int64_t grid_max)
{
    if (!h || xcd_mode < -1 || grid_max < 0) return ctk_set_error(CTK_E_INVALID, "%s: bad argument", who);
    (h->*k).xcd_dbg = xcd_mode;
    (h->*k).grid_dbg = grid_max;
    return CTK_OK;
}
static int knobs_form(ctk_handle *h, LaunchKnobs ctk_handle::*k, int64_t *out2)
{
    if (!h || !out2) return ctk_set_error(CTK_E_INVALID, "null argument");
    out2[0] = (h->*k).form; out2[1] = (h->*k).grid;
    return CTK_OK;
}

static bool async_wanted(ctk_handle *h);
// exclusive scan of n uint32 items into out[0 .. n] (out[n] = the total): one workgroup for short shards, block sums + one workgroup
// per 1024 items for long ones (k_scan_blocks)
static int launch_scan_u32(ctk_handle *h, const uint32_t *in, int64_t n, uint32_t *out, uint32_t *mail = nullptr, uint32_t stamp = 0)
{
    hipStream_t s = h->stream;
    uint32_t *ovf = (uint32_t *)h->counters.p + CTK_CNT_OVERFLOW;
    if (n <= 16 * CTK_SCAN_BLOCK) { k_scan_u32<<<1, 1024, 0, s>>>(in, n, out, ovf, mail, nullptr, stamp); return CTK_OK; }
    const int nb = (int)((n + CTK_SCAN_BLOCK - 1) / CTK_SCAN_BLOCK);
    CTKCHK(ensure(h, h->scan_bsum, (size_t)nb * 12));
    uint64_t *bsum = (uint64_t *)h->scan_bsum.p;
    uint32_t *bmax = (uint32_t *)(bsum + nb);
    k_scan_blocks_sum<<<nb, CTK_SCAN_BLOCK, 0, s>>>(in, n, bsum, bmax);
    k_scan_blocks<<<nb, CTK_SCAN_BLOCK, 0, s>>>(in, n, out, ovf, bsum, bmax, mail, stamp);
    return CTK_OK;
}

// Threshold field for the following track calls (include/contrack_hip.h).  The field stays on the device until it is cleared or
// replaced: repeated calls with the same climatology upload nothing.
extern "C" int ctk_set_threshold_field(ctk_handle *h, const void *field, int elem_bytes, int64_t nplanes, int ny, int nx,
                                       const int32_t *plane_of_step, int64_t T)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));                  // nothing in flight reads the old field
    h->fld_T = -1; h->fld_prep_op = -1; h->fld_order_chunk = -1;
    h->c_thr_valid = false;
    if (!field) {
        for (DevBuf *b : {&h->fld_raw, &h->fld_f32, &h->fld_pos, &h->fld_order}) b->release();
        h->fld_pos_host.clear();
        return CTK_OK;
    }
    if ((elem_bytes != 4 && elem_bytes != 8) || nplanes < 1 || ny < 1 || nx < 1 || T < 0 || (T > 0 && !plane_of_step))
        return ctk_set_error(CTK_E_INVALID, "ctk_set_threshold_field: bad arguments (elem_bytes=%d nplanes=%lld ny=%d nx=%d T=%lld)", elem_bytes,
                             (long long)nplanes, ny, nx, (long long)T);
    if (nplanes > 0x7fffffffll) return ctk_set_error(CTK_E_RANGE, "ctk_set_threshold_field: more than 2^31-1 planes");
    for (int64_t t = 0; t < T; t++)
        if (plane_of_step[t] < 0 || plane_of_step[t] >= nplanes)
            return ctk_set_error(CTK_E_INVALID, "ctk_set_threshold_field: plane_of_step[%lld] = %d is not in [0, %lld)", (long long)t, plane_of_step[t], (long long)nplanes);
    const size_t bytes = (size_t)nplanes * ny * nx * elem_bytes;
    CTKCHK(ensure(h, h->fld_raw, bytes));
    CTKCHK(ensure(h, h->fld_pos, (size_t)std::max<int64_t>(T, 1) * 4));
    HIPCHK(hipMemcpy(h->fld_raw.p, field, bytes, hipMemcpyHostToDevice));
    if (T > 0) HIPCHK(hipMemcpy(h->fld_pos.p, plane_of_step, (size_t)T * 4, hipMemcpyHostToDevice));
    h->fld_pos_host.assign(plane_of_step, plane_of_step + T);
    h->fld_T = T; h->fld_np = nplanes; h->fld_ny = ny; h->fld_nx = nx; h->fld_esz = elem_bytes;
    return CTK_OK;
}

// Segment breaks for the following track calls (include/contrack_hip.h).  The starts are kept; the per-step edge table is built on
// the device by the first call of a given T (segment_table) and reused while T stays the same.
extern "C" int ctk_set_segments(ctk_handle *h, const int64_t *starts, int64_t nseg)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (nseg < 0 || (nseg > 0 && !starts)) return ctk_set_error(CTK_E_INVALID, "ctk_set_segments: bad arguments (nseg=%lld)", (long long)nseg);
    if (nseg > 0) {
        if (starts[0] != 0) return ctk_set_error(CTK_E_INVALID, "ctk_set_segments: starts[0] = %lld, must be 0", (long long)starts[0]);
        for (int64_t k = 1; k < nseg; k++)
            if (starts[k] <= starts[k - 1])
                return ctk_set_error(CTK_E_INVALID, "ctk_set_segments: starts must be strictly increasing (starts[%lld] = %lld after %lld)", (long long)k,
                                     (long long)starts[k], (long long)starts[k - 1]);
        if (starts[nseg - 1] > 0x7ffffffell) return ctk_set_error(CTK_E_RANGE, "ctk_set_segments: start %lld beyond int32 timesteps", (long long)starts[nseg - 1]);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));                  // nothing in flight reads the old table
    h->seg_starts.assign(starts, starts + nseg);
    h->seg_edge_T = -1;
    h->seg_edge_host.clear();
    return CTK_OK;
}

// The edge table of the segments for a slab of T steps (T > the last start): bit 0 = first step of a segment, bit 1 = last step.
static int segment_table(ctk_handle *h, int64_t T)
{
    const std::vector<int64_t> &st = h->seg_starts;
    if (T <= st.back())
        return ctk_set_error(CTK_E_INVALID, "ctk_track: the last segment starts at step %lld, the slab has %lld steps", (long long)st.back(), (long long)T);
    if (h->seg_edge_T != T) {
        std::vector<uint8_t> &e = h->seg_edge_host;
        e.assign((size_t)T, 0);
        for (size_t k = 0; k < st.size(); k++) {
            e[(size_t)st[k]] |= 1u;
            if (st[k] > 0) e[(size_t)st[k] - 1] |= 2u;
        }
        e[(size_t)T - 1] |= 2u;
        CTKCHK(ensure(h, h->seg_edge, (size_t)T));
        HIPCHK(hipMemcpy(h->seg_edge.p, e.data(), (size_t)T, hipMemcpyHostToDevice));
        h->seg_edge_T = T;
    }
    h->seg_cur = P<uint8_t>(h->seg_edge);
    h->seg_cur_host = h->seg_edge_host.data();
    return CTK_OK;
}

// Segment starts given as an ARGUMENT of a call (the streaming and time-shard entries, ctk_track_*_seg_*): the rules of
// ctk_set_segments and the last start below the `T_total` steps of the whole slab (also ctk_anom_seg_* / ctk_anom_stream_*).
static int segment_starts_check(const char *who, const int64_t *starts, int64_t nseg, int64_t T_total)
{
    if (nseg < 0 || (nseg > 0 && !starts)) return ctk_set_error(CTK_E_INVALID, "%s: bad segment arguments (nseg=%lld)", who, (long long)nseg);
    if (nseg == 0) return CTK_OK;
    if (starts[0] != 0) return ctk_set_error(CTK_E_INVALID, "%s: segment starts[0] = %lld, must be 0", who, (long long)starts[0]);
    for (int64_t k = 1; k < nseg; k++)
        if (starts[k] <= starts[k - 1])
            return ctk_set_error(CTK_E_INVALID, "%s: segment starts must be strictly increasing (starts[%lld] = %lld after %lld)", who, (long long)k,
                                 (long long)starts[k], (long long)starts[k - 1]);
    if (starts[nseg - 1] >= T_total)
        return ctk_set_error(CTK_E_INVALID, "%s: the last segment starts at step %lld, the slab has %lld steps", who, (long long)starts[nseg - 1], (long long)T_total);
    return CTK_OK;
}
// ... for the track entries: and no sticky segments on the handle beside them
static int segment_args_check(const ctk_handle *h, const char *who, const int64_t *starts, int64_t nseg, int64_t T_total)
{
    if (!h->seg_starts.empty())
        return ctk_set_error(CTK_E_INVALID, "%s: segments are set on this handle (ctk_set_segments) and given as an argument; clear the handle's first", who);
    return segment_starts_check(who, starts, nseg, T_total);
}

// The edge table of the (checked) starts `st` over a slab of T_total steps; the steps [t_begin, t_begin + T) of it -- a time shard, or
// the whole slab -- become the current table of the launches and of the host.  One segment: no table, the unsegmented kernels.
static int segment_table_call(ctk_handle *h, const std::vector<int64_t> &st, int64_t T_total, int64_t t_begin, int64_t T)
{
    h->seg_cur = nullptr; h->seg_cur_host = nullptr;
    if (st.size() < 2 || T < 1) return CTK_OK;
    std::vector<uint8_t> &e = h->seg_edge_host;
    h->seg_edge_T = -1;                                        // (not the table segment_table remembers)
    e.assign((size_t)T_total, 0);
    for (size_t k = 0; k < st.size(); k++) {
        e[(size_t)st[k]] |= 1u;
        if (st[k] > 0) e[(size_t)st[k] - 1] |= 2u;
    }
    e[(size_t)T_total - 1] |= 2u;
    // a shard inside one segment launches the unsegmented kernels (the first step of the slab and its last one are edges to them too)
    bool any = false;
    for (int64_t t = t_begin; t < t_begin + T && !any; t++)
        any = (e[(size_t)t] & ~((t == 0 ? 1u : 0u) | (t == T_total - 1 ? 2u : 0u))) != 0;
    if (!any) return CTK_OK;
    CTKCHK(ensure(h, h->seg_edge, (size_t)T));
    HIPCHK(hipMemcpy(h->seg_edge.p, e.data() + t_begin, (size_t)T, hipMemcpyHostToDevice));
    h->seg_cur = P<uint8_t>(h->seg_edge);
    h->seg_cur_host = e.data() + t_begin;
    return CTK_OK;
}

// the device side of a field call: the float32 compare field for this op (from a float64 field, once per field and op) and the
// plane-major step order for launches of `chunk` steps (once per field and chunk length)
static int prepare_field(ctk_handle *h, bool f64, int cmp_op, int64_t chunk)
{
    hipStream_t s = h->stream;
    const int64_t n = h->fld_np * h->fld_ny * h->fld_nx;
    if (!f64 && h->fld_esz == 8 && h->fld_prep_op != cmp_op) {
        CTKCHK(ensure(h, h->fld_f32, (size_t)n * 4));
        const int g = (int)std::min<int64_t>((n + 255) / 256, 8192);
        const double *in = P<double>(h->fld_raw);
        float *out = P<float>(h->fld_f32);
        switch (cmp_op) {
        case 0: k_thr_field_prep<0><<<g, 256, 0, s>>>(in, out, n); break;
        case 1: k_thr_field_prep<1><<<g, 256, 0, s>>>(in, out, n); break;
        case 2: k_thr_field_prep<2><<<g, 256, 0, s>>>(in, out, n); break;
        default: k_thr_field_prep<3><<<g, 256, 0, s>>>(in, out, n); break;
        }
        HIPCHK(hipGetLastError());
        h->fld_prep_op = cmp_op;
    }
    if (h->fld_order_chunk != chunk) {
        const int64_t T = h->fld_T;
        std::vector<int32_t> &ord = h->fld_order_host;
        ord.resize((size_t)std::max<int64_t>(T, 1));
        for (int64_t c0 = 0; c0 < T; c0 += chunk) {
            const int64_t nt = std::min<int64_t>(chunk, T - c0);
            int32_t *o = ord.data() + c0;
            for (int64_t i = 0; i < nt; i++) o[i] = (int32_t)i;                    // step of the chunk, relative to its first step
            const int32_t *p = h->fld_pos_host.data() + c0;
            std::stable_sort(o, o + nt, [p](int32_t a, int32_t b) { return p[a] < p[b]; });
        }
        CTKCHK(ensure(h, h->fld_order, ord.size() * 4));
        HIPCHK(hipMemcpyAsync(h->fld_order.p, ord.data(), ord.size() * 4, hipMemcpyHostToDevice, s));
        h->fld_order_chunk = chunk;
    }
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// stage 1 in steps, called in this order by shard_label2d_impl: label2d_begin, label2d_stage_inputs, label2d_upload,
// label2d_threshold (launch_threshold, mask_placement_check), label2d_rowcount, label2d_speculate, label2d_wait_scan,
// label2d_regrow, label2d_finish_labels, label2d_compact.  What they hand to each other:
// ------------------------------------------------------------------------------------------------
struct Label2dCall {
    const void *anom_dev; bool f64; int64_t T; int ny, nx, W; const double *thr; int cmp_op; const float *wrow;
    bool defer_compact;                     // see shard_label2d_impl
    bool fld_call;                          // thr == NULL: the threshold field set on the handle (ctk_set_threshold_field), if its shape is this call's
    int64_t nrows;
    bool same_thr, same_w;                  // equal to the previous call's: already on the device
    double *thr32; int64_t *wlo;            // pinned staging (float32 thresholds in the first half when !f64)
    size_t w_bytes;                         // wlo[ny] whi[ny] (int64) next_tiny[ny+1] (int32)
    bool mask_fresh;                        // this call allocated the mask
    uint32_t scan_stamp;
    CtkLabelShape shape;
    bool spec;                              // a speculative labelling launch was made
    CtkVariantSet launched;
    int rc_launched, rc_groups; int64_t label_forms;   // (CTK_S_ROWCOUNT_THREADS, CTK_S_ROWCOUNT_GROUPS, CTK_S_LABEL_FORMS: recorded after the statistics are reset)
};

static int label2d_begin(ctk_handle *h, Label2dCall &c, int has_prev)
{
    const int64_t T = c.T;
    const int ny = c.ny, nx = c.nx;
    c.fld_call = T > 0 && !c.thr && h->fld_T == T && h->fld_ny == ny && h->fld_nx == nx;
    if (T > 0 && !c.thr && !c.fld_call && ny >= 1 && nx >= 1)
        return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d: thr is NULL and no threshold field of shape (T=%lld, ny=%d, nx=%d) is set%s", (long long)T, ny, nx,
                             h->fld_T >= 0 ? " (the field set has another shape)" : "");
    if (T < 0 || ny < 1 || nx < 1 || (T > 0 && ((!c.anom_dev && !h->sio) || (!c.thr && !c.fld_call))) || !c.wrow)
        return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d: bad shape (T=%lld ny=%d nx=%d) or null pointer", (long long)T, ny, nx);
    if (c.cmp_op < 0 || c.cmp_op > 3) return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d: cmp_op %d not in 0..3", c.cmp_op);
    if (nx > 65535 || ny > 65535) return ctk_set_error(CTK_E_RANGE, "ctk_shard_label2d: grid %dx%d exceeds 65535 per axis", ny, nx);
    // one workgroup of up to 1024 threads per timestep in several kernels; a HIP grid carries < 2^32 work-items
    if (T > 4000000ll) return ctk_set_error(CTK_E_RANGE, "ctk_shard_label2d: more than 4 000 000 timesteps in one shard");
    HIPCHK(hipSetDevice(h->device));
    memset(h->ms, 0, sizeof(h->ms));
    h->pass_no++;
    h->state = ST_IDLE;
    h->halo_valid = false; h->halo_v2 = c.defer_compact;
    h->T = T; h->ny = ny; h->nx = nx; h->W = (nx + 63) / 64; h->has_prev = has_prev ? 1 : 0; h->cmp_op = c.cmp_op;
    c.W = h->W;
    c.nrows = T * ny;
    c.shape = ctk_label_shape(T, ny, c.W);
    c.spec = false;
    c.launched = {false, false, false, false, false, false};
    c.rc_launched = 0; c.rc_groups = 0; c.label_forms = 0;
    return CTK_OK;
}

// host-side preparation: thresholds for the float32 compare, exact integer limbs of the row weights -- staged in
// pinned memory, so that the uploads are asynchronous and nothing has to be waited for before the first kernel.
// Thresholds / weights equal to the previous call's are already on the device: nothing is converted or uploaded.
static int label2d_stage_inputs(ctk_handle *h, Label2dCall &c)
{
    const int64_t T = c.T;
    const int ny = c.ny, nx = c.nx, cmp_op = c.cmp_op;
    const bool f64 = c.f64;
    const double *thr = c.thr;
    const float *wrow = c.wrow;
    const size_t thr_bytes = (size_t)std::max<int64_t>(T, 1) * 8;
    c.same_thr = c.fld_call || (h->c_thr_valid && h->c_T == T && h->c_f64 == f64 && h->c_cmp == cmp_op && (T == 0 || memcmp(h->c_thr.data(), thr, (size_t)T * 8) == 0));
    if (c.fld_call) h->c_thr_valid = false;                           // (a field call leaves no per-step thresholds behind)
    c.same_w = h->c_w_valid && (int)h->c_w.size() == ny && h->c_w_nx == nx && memcmp(h->c_w.data(), wrow, (size_t)ny * 4) == 0;
    double *thr32 = nullptr;
    int64_t *wlo = nullptr;
    c.w_bytes = (size_t)ny * 16 + ((size_t)ny + 2) * 4;
    if (!c.same_thr || !c.same_w) {
        CTKCHK(ensure_host(h, h->h_stage, thr_bytes + c.w_bytes));
        thr32 = (double *)h->h_stage.p;
        wlo = (int64_t *)((char *)h->h_stage.p + thr_bytes);
    }
    c.thr32 = thr32; c.wlo = wlo;
    if (!c.same_thr) {
        h->c_thr_valid = false;
        if (f64) for (int64_t t = 0; t < T; t++) thr32[t] = thr[t];
        else for (int64_t t = 0; t < T; t++) ((float *)thr32)[t] = adjust_threshold(thr[t], cmp_op);
        h->c_thr.assign(thr, thr + T);
        h->c_T = T; h->c_f64 = f64; h->c_cmp = cmp_op;
    }
    if (!c.same_w) {
        h->c_w_valid = false;
        CTKCHK(ctk_weights_to_limbs(wrow, ny, (int64_t)ny * nx, wlo, wlo + ny, &h->wshift, &h->limb_bits));
        h->c_w.assign(wrow, wrow + ny);
        h->c_w_nx = nx;
        // Lowest set bit of every integer row weight.  A float64 partial sum of rows whose lowest bits are all >= L is exact in
        // ANY order while it stays below 2^(L+53).  No area sum exceeds max|W| * ny * nx: rows with bits below that bound - 53
        // (the pole rows) are the only ones that can make numpy's pairwise sum differ from the exact sum rounded once.
        std::vector<int> lsb((size_t)ny, 127);
        int maxbl = 0;
        h->w_minlsb = 127;
        for (int y = 0; y < ny; y++) {
            const __int128 wi = (__int128)wlo[y] + ((__int128)wlo[ny + y] << h->limb_bits);
            if (wi == 0) continue;
            unsigned __int128 m = wi < 0 ? (unsigned __int128)(-wi) : (unsigned __int128)wi;
            int l = 0, bl = 0;
            while (!((m >> l) & 1)) l++;
            for (unsigned __int128 q = m; q; q >>= 1) bl++;
            lsb[(size_t)y] = l;
            maxbl = std::max(maxbl, bl);
            h->w_minlsb = std::min(h->w_minlsb, l);
        }
        if (h->w_minlsb == 127) h->w_minlsb = 0;
        int lg = 0;
        while (((int64_t)1 << lg) < (int64_t)ny * nx) lg++;
        int32_t *next_tiny = (int32_t *)(wlo + 2 * (size_t)ny);
        next_tiny[ny] = ny;
        for (int y = ny - 1; y >= 0; y--) next_tiny[y] = (lsb[(size_t)y] < maxbl + lg - 53) ? y : next_tiny[y + 1];
    }
    return CTK_OK;
}

// the per-row / per-step buffers of the shard and the uploads of what label2d_stage_inputs staged
static int label2d_upload(ctk_handle *h, Label2dCall &c)
{
    const int64_t T = c.T, nrows = c.nrows;
    const int W = c.W;
    hipStream_t s = h->stream;
    const void *mask_before = h->mask.p;
    CTKCHK(ensure(h, h->mask, (size_t)nrows * W * 8));
    c.mask_fresh = h->mask.p != mask_before;
    CTKCHK(ensure(h, h->wstart, (size_t)nrows * W * 2));
    CTKCHK(ensure(h, h->rowstart, (size_t)nrows * 4));
    CTKCHK(ensure(h, h->tcount, (size_t)T * 4));
    CTKCHK(ensure(h, h->run_base, (size_t)(T + 1) * 4));
    CTKCHK(ensure(h, h->ncomp, (size_t)T * 4));
    CTKCHK(ensure(h, h->cprefix, (size_t)(T + 2) * 4));                  // [-1] = 0: the halo components of a time shard come first
    CTKCHK(ensure(h, h->thr32, (size_t)T * 8));
    CTKCHK(ensure(h, h->wlo, c.w_bytes));                             // wlo[ny] whi[ny] next_tiny[ny+1] in one allocation
    CTKCHK(ensure(h, h->counters, CTK_CNT_WORDS * 4));
    CTKCHK(ensure_host(h, h->h_small, (size_t)(T + 1) * 4 + 1024));     // run_base copy + scalar downloads

    // (the device counters are zeroed by the first threshold launch of the pass; k_rowcount writes every tcount[t])
    if (T == 0) HIPCHK(hipMemsetAsync(h->counters.p, 0, CTK_CNT_ZEROED * 4, s));
    if (T > 0) {
        if (!c.same_thr) { HIPCHK(hipMemcpyAsync(h->thr32.p, c.thr32, (size_t)T * (c.f64 ? 8 : 4), hipMemcpyHostToDevice, s)); h->c_thr_valid = true; }
        if (c.fld_call) CTKCHK(prepare_field(h, c.f64, c.cmp_op, h->sio ? h->sio->chunk : T));
    }
    if (!c.same_w) { HIPCHK(hipMemcpyAsync(h->wlo.p, c.wlo, c.w_bytes, hipMemcpyHostToDevice, s)); h->c_w_valid = true; }    // same layout on both sides
    HT("uploads queued");
    return CTK_OK;
}

// the mask of timesteps [t0, t0 + nt) of the slab, which are at `src` on the device
static int launch_threshold(ctk_handle *h, const Label2dCall &c, const void *src, int64_t t0, int64_t nt)
{
    const int ny = c.ny, nx = c.nx, W = c.W;
    const bool f64 = c.f64;
    hipStream_t s = h->stream;
    const CtkThrForm f = ctk_threshold_form(nt, ny, nx, W, f64, ((uintptr_t)src & 15) == 0, c.fld_call);
    const int64_t rows = nt * ny;
    uint64_t *mk = P<uint64_t>(h->mask) + t0 * ny * W;
    uint32_t *zc = t0 == 0 ? P<uint32_t>(h->counters) : nullptr;
    if (c.fld_call) {                                    // the threshold field: its own kernels, launched here and nowhere else
        const float *f32 = h->fld_esz == 4 ? P<float>(h->fld_raw) : P<float>(h->fld_f32);
        const int32_t *pos = P<int32_t>(h->fld_pos) + t0, *ord = P<int32_t>(h->fld_order) + t0;
#define LAUNCH_FLD(OP)                                                                                                                      \
    do {                                                                                                                                \
        if (f.kind == CTK_THR_FIELD_VEC) k_threshold_field<OP, 4><<<f.grid, 256, 0, s>>>((const float *)src, f32, pos, ord, ny, nx, W, mk, f.rbt, zc); \
        else if (!f64) k_threshold_field_g<OP, float, float><<<f.grid, 256, 0, s>>>((const float *)src, f32, pos, rows, ny, nx, W, mk, zc);     \
        else if (h->fld_esz == 4) k_threshold_field_g<OP, double, float><<<f.grid, 256, 0, s>>>((const double *)src, P<float>(h->fld_raw), pos, rows, ny, nx, W, mk, zc); \
        else k_threshold_field_g<OP, double, double><<<f.grid, 256, 0, s>>>((const double *)src, P<double>(h->fld_raw), pos, rows, ny, nx, W, mk, zc); \
    } while (0)
        switch (c.cmp_op) {
        case 0: LAUNCH_FLD(0); break;
        case 1: LAUNCH_FLD(1); break;
        case 2: LAUNCH_FLD(2); break;
        default: LAUNCH_FLD(3); break;
        }
#undef LAUNCH_FLD
        HIPCHK(hipGetLastError());
        return CTK_OK;
    }
    const bool thr_probe = h->thr_probe || h->thr_nostore;                      // a launch of the mask placement check: its own kernel name
    const int nostore = h->thr_nostore ? 1 : 0;
    const float *t32 = P<float>(h->thr32) + t0;
#define LAUNCH_V7(OP, U)                                                                                                                    \
    case U:                                                                                                                             \
        if (thr_probe) k_threshold_probe<OP, U><<<f.grid, 256, 0, s>>>((const float *)src, t32, ny, nx, W, mk, f.rbt, zc, CTK_THR_XCD_TILE, nostore); \
        else k_threshold_v7<OP, U><<<f.grid, 256, 0, s>>>((const float *)src, t32, ny, nx, W, mk, f.rbt, zc, CTK_THR_XCD_TILE);                       \
        break
#define LAUNCH_THR(OP)                                                                                                                      \
    switch (f.kind) {                                                                                                                   \
    case CTK_THR_V6: k_threshold_v6<OP, 8><<<f.grid, 256, 0, s>>>((const float *)src, t32, ny, nx, W, mk, f.r6, f.nchunk_t, f.nchunks, zc); break; \
    case CTK_THR_F64: k_threshold<OP, double><<<f.grid, 256, 0, s>>>((const double *)src, P<double>(h->thr32) + t0, rows, ny, nx, W, mk, zc); break; \
    case CTK_THR_F32: k_threshold<OP, float><<<f.grid, 256, 0, s>>>((const float *)src, t32, rows, ny, nx, W, mk, zc); break;             \
    default:                                                                                                                            \
        switch (f.u7) { LAUNCH_V7(OP, 4); LAUNCH_V7(OP, 5); LAUNCH_V7(OP, 6); LAUNCH_V7(OP, 7); default: LAUNCH_V7(OP, 8); }              \
        break;                                                                                                                          \
    }
    switch (c.cmp_op) {
    case 0: LAUNCH_THR(0); break;
    case 1: LAUNCH_THR(1); break;
    case 2: LAUNCH_THR(2); break;
    default: LAUNCH_THR(3); break;
    }
#undef LAUNCH_THR
#undef LAUNCH_V7
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// Where the bit mask lies against the SLAB decides what its 1/32 write stream costs the 4 B/pixel read stream: device memory comes
// in two classes of physical regions (each hundreds of MB to many GB long, invisible in the virtual address), and a read stream
// and a write stream that run in the SAME class disturb each other -- k_threshold is then 11-18 % above its read-only time
// instead of 4-6 % (0.119 vs 0.106 ms at 2707 x 181 x 360, 0.36 vs 0.315 at 480 x 721 x 1440; profiles/NOTES.md round 5 and
// profiles/r05_rwmix_*.txt: slab region x mask region matrix, consistent with the write-to-read turnaround inside one DRAM rank).
// Allocations made right after each other usually share a class -- the "bimodal board" of rounds 2-4.  So a freshly allocated
// mask is checked against the slab: the kernel's time WITHOUT its stores (on the first 4 GB of a larger slab) is the yardstick,
// and if the kernel with its stores is more than 8.5 % above it, ONE other mask is allocated behind a 1 GB spacer that is freed
// again (round 6: bounded; see below).  Two launches per measurement, 4 in the usual case (the first mask is fine), at most 8; once
// per handle and mask size; CTK_MASK_TUNE=0 turns it off.
// WHEN: not in the call that allocated the mask but in the next one that uses it -- a one-shot run_contrack never pays for it (a
// few launches mean nothing to a handle that is used again and again, and are pure overhead for one that is not: round-4
// verdict).
static int mask_placement_check(ctk_handle *h, const Label2dCall &c)
{
    const int64_t T = c.T;
    const int ny = c.ny, nx = c.nx;
    const void *anom_dev = c.anom_dev;
    hipStream_t s = h->stream;
    if (c.mask_fresh) { h->mask_tries = 0; h->mask_ratio = 0.0; h->mask_check_pending = true; h->mask_check_retries = 0; }
    // (the whole slab up to 4 GB: the classes change along a slab and along a mask, a window of 256 MB told little about
    // the whole kernel -- measured)
    const int64_t nt_probe = std::min<int64_t>(T, std::max<int64_t>(1, ((int64_t)4 << 30) / ((int64_t)ny * nx * 4)));
    if (!(anom_dev && !c.fld_call && h->mask_check_pending && !c.mask_fresh && ctk_env().mask_tune && (size_t)T * ny * nx * 4 >= ((size_t)128 << 20))) return CTK_OK;
    // (only where the launches of the check are the probe builds of k_threshold_v7)
    if (ctk_threshold_form(nt_probe, ny, nx, c.W, c.f64, ((uintptr_t)anom_dev & 15) == 0, false).kind != CTK_THR_V7) return CTK_OK;
    h->mask_check_pending = false;
    h->mask_spacer_gb = 0.0;
    struct CheckTime { ctk_handle *h; double t0; ~CheckTime() { h->mask_check_ms = now_ms() - t0; } } check_time{h, now_ms()};
    Event e0, e1;
    if (e0.create() == hipSuccess && e1.create() == hipSuccess) {
        const size_t mbytes = (size_t)c.nrows * c.W * 8;
        auto time_it = [&](double *ms) -> int {
            CTKCHK(launch_threshold(h, c, anom_dev, 0, nt_probe));
            HIPCHK(hipEventRecord(e0, s));
            CTKCHK(launch_threshold(h, c, anom_dev, 0, nt_probe));
            HIPCHK(hipEventRecord(e1, s));
            HIPCHK(hipEventSynchronize(e1));
            float f = 0.f;
            HIPCHK(hipEventElapsedTime(&f, e0, e1));
            *ms = f;
            return CTK_OK;
        };
        int rc = CTK_OK;
        double ro_ms = 0.0, best_ms = 1e30;
        const double accept = 1.085;
        h->thr_probe = true;
        struct ProbeOff { ctk_handle *h; ~ProbeOff() { h->thr_probe = false; h->thr_nostore = false; } } probe_off{h};
        h->thr_nostore = true;                                                  // the yardstick: the same kernel without its stores
        rc = time_it(&ro_ms);
        h->thr_nostore = false;
        if (rc == CTK_OK) rc = time_it(&best_ms);
        h->mask_tries = 1;
        // Is the device ours?  With other work on it (other handles tracking their members at the same time) the times mean
        // nothing -- the kernel "with stores" came out at 0.3-0.85 of the one without in bench.py's four-handle block.  The
        // yardstick once more: apart by more than 4 %, or slower than the kernel with its stores, and the mask stays where it is.
        if (rc == CTK_OK && best_ms > accept * ro_ms) {
            double ro2 = 0.0;
            h->thr_nostore = true;
            rc = time_it(&ro2);
            h->thr_nostore = false;
            if (rc == CTK_OK && (ro2 > 1.04 * ro_ms || ro_ms > 1.04 * ro2 || best_ms < 0.98 * std::min(ro_ms, ro2))) { best_ms = 0.0; h->mask_tries = 0; if (++h->mask_check_retries <= 3) h->mask_check_pending = true; }      // (inconclusive: no search now; up to three later calls try again)
            else ro_ms = std::min(ro_ms, ro2);
        } else if (rc == CTK_OK && best_ms < 0.98 * ro_ms) h->mask_tries = 0;
        // Round 6 (verdict item 4): the search is OFF by default and BOUNDED when asked for -- at most one other allocation, behind one spacer of 1 GB that is
        // released before the call goes on; nothing is ever kept alive besides the mask itself (round 5 tried up to five
        // allocations behind 29 GB of spacers and two 6 GB arenas; on the boxes where it mattered it found nothing, and what it
        // cost a caller's second call was recorded nowhere).  Its host time and the spacer it held are in the statistics
        // (CTK_S_MASK_CHECK_US, CTK_S_MASK_SPACER_MB).  Where the first two candidates share the slab's class the kernel runs
        // at 5.9-6.1 instead of 6.5 TB/s; DESIGN.md section 3 says so.
        // DEFAULT: NO search at all -- the check only measures (4 launches) and reports; the kernel runs at 5.9 or 6.5 TB/s as
        // the allocator happened to place the mask.  (The one retry found memory of the other class for about a quarter of this
        // round's handles and cost 1.3-6 ms of the handle's second call, once 32 ms: hipMalloc / hipFree of the spacer synchronise
        // the device.)  CTK_MASK_TRIES=1: the one retry described above, opt-in.
        const int max_tries = ctk_env().mask_tries;
        std::vector<DevBuf> held;                                               // the spacer and the rejected mask: freed when the search is over
        for (int k = 0; rc == CTK_OK && k < max_tries && best_ms > accept * ro_ms; k++) {
            // (never into the last quarter of the device: other handles allocate their work spaces at the same time)
            size_t mem_free = 0, mem_total = 0;
            const size_t spacer = (size_t)1 << 30;
            if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess || mem_free < spacer + mbytes + mem_total / 4) { (void)hipGetLastError(); break; }
            DevBuf sp;
            if (sp.alloc(spacer) != hipSuccess) { (void)hipGetLastError(); break; }
            held.push_back(std::move(sp)); h->mask_spacer_gb = 1.0;
            DevBuf nb;
            if (ensure(h, nb, mbytes) != CTK_OK) break;                         // (no memory for another try: keep what there is)
            h->mask.swap(nb);                                                   // the candidate is the handle's mask while it is timed
            double ms = 0.0;
            rc = time_it(&ms);
            h->mask_tries++;
            if (rc == CTK_OK && ms < best_ms) best_ms = ms;
            else h->mask.swap(nb);                                              // (no better: the mask there was comes back)
            held.push_back(std::move(nb));                                      // the loser of the two
        }
        h->mask_ratio = ro_ms > 0 ? best_ms / ro_ms : 0.0;
        if (ctk_env().hosttrace) fprintf(stderr, "mask placement: %d allocation(s) tried, threshold kernel on a %lld-step window %.4f ms = %.3f x its time without stores (%.4f), mask at %p, slab at %p\n", h->mask_tries, (long long)nt_probe, best_ms, h->mask_ratio, ro_ms, h->mask.p, anom_dev);
        for (DevBuf &b : held) b.release();                                     // (in the order they were taken)
        if (rc != CTK_OK) return rc;
    }
    return CTK_OK;
}

static int label2d_threshold(ctk_handle *h, const Label2dCall &c)
{
    if (c.T == 0) return CTK_OK;
    Timer tm(h, CTK_K_THRESHOLD);
    CTKCHK(mask_placement_check(h, c));
    if (c.anom_dev) return launch_threshold(h, c, c.anom_dev, 0, c.T);
    // the slab arrives in chunks (ctk_track_stream_*)
    return stream_in(h, c.f64, c.T, c.ny, c.nx, [&](const void *src, int64_t t0, int64_t nt) { return launch_threshold(h, c, src, t0, nt); });
}

// runs per row, word and timestep, and their scan.  The host learns the run totals from the scan kernel's block of scalars in
// pinned memory and knows that it is complete by the stamp the kernel writes last (an event record after the kernel is a command
// of its own: 5 us of stream time).
struct RowcountInstance { void (*fn)(const uint64_t *, int, int, uint16_t *, uint32_t *, uint32_t *); int rcu; };
template <int RCU> static RowcountInstance rowcount_instance() { return {k_rowcount<RCU>, RCU}; }
static int label2d_rowcount(ctk_handle *h, Label2dCall &c)
{
    const int64_t T = c.T;
    c.scan_stamp = (uint32_t)(h->pass_no & 0x7fffffffu) | 0x80000000u;
    Timer tm(h, CTK_KI_ROWCOUNT);
    const int rc_threads = ctk_rowcount_threads(T, c.ny, c.W);
    const int rc_groups = ctk_rowcount_groups(rc_threads, c.ny, c.W);
    RowcountInstance ki = rowcount_instance<8>();
    switch (rc_groups) {
    case 4: ki = rowcount_instance<4>(); break;
    case 6: ki = rowcount_instance<6>(); break;
    default: break;
    }
    if (T > 0) ki.fn<<<(int)T, rc_threads, 0, h->stream>>>(P<uint64_t>(h->mask), c.ny, c.W, P<uint16_t>(h->wstart), P<uint32_t>(h->rowstart), P<uint32_t>(h->tcount));
    c.rc_launched = T > 0 ? rc_threads : 0;
    c.rc_groups = (T > 0 && ctk_rowcount_first_form(c.ny, c.W)) ? ki.rcu : 0;   // (the launched instance's own RCU: what the switch made of rc_groups)
    CTKCHK(launch_scan_u32(h, P<uint32_t>(h->tcount), T, P<uint32_t>(h->run_base), h->h_mail1, c.scan_stamp));
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// one launch of a set of labelling variants; v2 and v3 run on the side streams
static int launch_label2d(ctk_handle *h, Label2dCall &c, const CtkVariantSet &vs, uint32_t cap_runs)
{
    const int T = (int)c.T;
    hipStream_t s = h->stream;
    Label2dArgs a;
    a.mask = P<uint64_t>(h->mask); a.wstart = P<uint16_t>(h->wstart); a.rowstart = P<uint32_t>(h->rowstart);
    a.run_base = P<uint32_t>(h->run_base); a.run_comp = P<uint32_t>(h->run_comp); a.ncomp = P<uint32_t>(h->ncomp);
    a.cs_mrep = P<uint32_t>(h->cs_mrep); a.cs_box = P<uint32_t>(h->cs_box); a.cs_area = P<int64_t>(h->cs_area);
    a.seams = P<CtkSeam>(h->seams); a.seam_cnt = P<uint32_t>(h->seam_cnt); a.counters = P<uint32_t>(h->counters);
    a.wlo = P<int64_t>(h->wlo); a.whi = P<int64_t>(h->wlo) + h->ny;
    a.ny = c.ny; a.nx = c.nx; a.W = c.W; a.lds_cap = CTK_LDS_RUNS; a.cap_runs = cap_runs;
    a.g_x0 = P<uint16_t>(h->g_x0); a.g_x1 = P<uint16_t>(h->g_x1); a.g_y = P<uint16_t>(h->g_y);
    a.g_parent = P<uint32_t>(h->g_parent); a.g_root = P<uint32_t>(h->g_root); a.g_idmap = P<uint32_t>(h->g_idmap);
    if (vs.one) k_label2d_lds<CTK_LDS_RUNS, 512, -1, 1024><<<T, 1024, 0, s>>>(a);
    if (vs.v2 || vs.v3) HIPCHK(hipEventRecord(h->ev_fork, s));
    if (vs.v1) {
        if (c.shape.v0b) k_label2d_lds<CTK_LBL_V0B_RUNS, 272, -1, 256, 256><<<T, 256, 0, s>>>(a);
        else if (c.shape.v0_ok) k_label2d_lds<CTK_LBL_V0_RUNS, 240, -1, 256, 256><<<T, 256, 0, s>>>(a);
        else k_label2d_lds<CTK_LBL_V1_RUNS, 288, -1, 256><<<T, 256, 0, s>>>(a);
    }
    if (vs.v1hi) {
        if (c.shape.v0b) k_label2d_lds<CTK_LBL_V1_RUNS, 288, CTK_LBL_V0B_RUNS, 256><<<T, 256, 0, s>>>(a);
        else k_label2d_lds<CTK_LBL_V1_RUNS, 288, CTK_LBL_V0_RUNS, 256><<<T, 256, 0, s>>>(a);
    }
    c.label_forms |= ctk_label_form_bits(vs, c.shape);
    if (vs.v2) {
        HIPCHK(hipStreamWaitEvent(h->side[0], h->ev_fork, 0));
        k_label2d_lds<CTK_LBL_V2_RUNS, 512, CTK_LBL_V1_RUNS, 512><<<T, 512, 0, h->side[0]>>>(a);
        HIPCHK(hipEventRecord(h->ev_join[0], h->side[0]));
    }
    if (vs.v3) {
        HIPCHK(hipStreamWaitEvent(h->side[1], h->ev_fork, 0));
        k_label2d_lds<CTK_LDS_RUNS, 512, CTK_LBL_V2_RUNS, 1024><<<T, 1024, 0, h->side[1]>>>(a);
        HIPCHK(hipEventRecord(h->ev_join[1], h->side[1]));
    }
    if (vs.v2) HIPCHK(hipStreamWaitEvent(s, h->ev_join[0], 0));
    if (vs.v3) HIPCHK(hipStreamWaitEvent(s, h->ev_join[1], 0));
    if (vs.glb) k_label2d_glb<<<T, 256, 0, s>>>(a, P<uint32_t>(h->g_rs));
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// 2-D labelling.  Which variants are needed and how large the run-indexed buffers must be is known only after the run scan -- but
// a call on the same kind of data as the previous one needs the same: the launch is made SPECULATIVELY with the previous call's
// buffers and variant set before the host waits for the scan (every workgroup checks its runs against the buffers' capacity), and
// only what turns out to be missing is launched afterwards (label2d_finish_labels).
static int label2d_speculate(ctk_handle *h, Label2dCall &c)
{
    const int64_t T = c.T, nrows = c.nrows;
    if (nrows > 0x7fffffff) return ctk_set_error(CTK_E_RANGE, "ctk_shard_label2d: more than 2^31 rows in one shard");
    h->seam_cap = (uint32_t)nrows;
    CTKCHK(ensure(h, h->seams, (size_t)nrows * sizeof(CtkSeam)));
    CTKCHK(ensure(h, h->seam_cnt, (size_t)T * 4));
    CTKCHK(ensure(h, h->seam_off, (size_t)(T + 1) * 4));
    c.spec = T > 0 && h->runs_cap > 0 && h->spec_ny == c.ny && h->spec_nx == c.nx && (!h->spec_set.glb || h->spec_T >= T);
    if (c.spec) {
        Timer tm(h, CTK_K_LABEL2D);
        c.launched = ctk_label_speculative(h->spec_set, c.shape);
        CTKCHK(launch_label2d(h, c, c.launched, h->runs_cap));
    }
    return CTK_OK;
}

// the scan kernel wrote total / maximum / overflow / last count into the pinned mailbox; the statistics of the pass start here
static int label2d_wait_scan(ctk_handle *h, const Label2dCall &c)
{
    HT("thr+scan launched");
    {   // not the stream: the speculative labelling may still be running
        volatile uint32_t *vm = h->h_mail1;
        for (uint64_t spins = 0; vm[4] != c.scan_stamp; spins++) {
            // (the health check is rare on purpose: a hipStreamQuery on a busy stream makes the runtime enqueue a marker behind the
            // speculatively launched labelling kernel -- a 6 us bubble in front of the next kernel of every pass)
            if ((spins & 0xfffff) == 0xfffff) {
                const hipError_t q = hipStreamQuery(h->stream);
                if (q == hipSuccess) { if (vm[4] != c.scan_stamp) return ctk_set_error(CTK_E_INTERNAL, "stage 1: the run scan did not report"); break; }
                if (q != hipErrorNotReady) return ctk_set_error(CTK_E_NODEVICE, "stage 1: %s", hipGetErrorString(q));
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    const uint32_t m_total = h->h_mail1[0], m_max = h->h_mail1[1], m_ovf = h->h_mail1[2], m_last = h->h_mail1[3];
    HT("sync1 done");
    if (m_ovf & CTK_OVF_RUNS) return ctk_set_error(CTK_E_RANGE, "ctk_shard_label2d: more than 2^32-1 runs in one shard");
    h->total_runs = m_total;
    h->max_runs_step = m_max;
    h->rb_total = m_total; h->rb_last = m_total - m_last;
    h->need_glb = ctk_label_need_glb(h->max_runs_step, c.ny);
    memset(h->stats, 0, sizeof(h->stats));
    h->stats[CTK_S_RUNS] = h->total_runs; h->stats[CTK_S_MAX_RUNS_STEP] = h->max_runs_step;
    h->stats[CTK_S_MASK_TRIES] = h->mask_tries; h->stats[CTK_S_MASK_RATIO] = (int64_t)(h->mask_ratio * 1000.0 + 0.5);      // (sticky: of the last placement check)
    h->stats[CTK_S_MASK_CHECK_US] = (int64_t)(h->mask_check_ms * 1000.0 + 0.5); h->stats[CTK_S_MASK_SPACER_MB] = (int64_t)(h->mask_spacer_gb * 1024.0 + 0.5);
    return CTK_OK;
}

// the run-indexed buffers for the totals the scan reported
static int label2d_regrow(ctk_handle *h, Label2dCall &c)
{
    const size_t R = h->total_runs;
    const bool fits = c.spec && R <= h->runs_cap;
    if (!fits) {
        // run-indexed buffers with head room, so that the next calls on similar data can launch speculatively
        const size_t Rc = R + R / 8 + 1024;
        CTKCHK(ensure(h, h->run_comp, Rc * 4));
        CTKCHK(ensure(h, h->run_val, Rc * 4));
        CTKCHK(ensure(h, h->cs_mrep, Rc * 4));
        CTKCHK(ensure(h, h->cs_box, Rc * 16));
        CTKCHK(ensure(h, h->cs_area, Rc * 16));
        CTKCHK(ensure(h, h->d_mrep, Rc * 4));
        CTKCHK(ensure(h, h->d_box, Rc * 8));
        CTKCHK(ensure(h, h->d_area, Rc * 16));
        CTKCHK(ensure(h, h->d_comp_t, Rc * 4));
        if (h->need_glb || h->spec_set.glb) {
            CTKCHK(ensure(h, h->g_x0, Rc * 2)); CTKCHK(ensure(h, h->g_x1, Rc * 2)); CTKCHK(ensure(h, h->g_y, Rc * 2));
            CTKCHK(ensure(h, h->g_parent, Rc * 4)); CTKCHK(ensure(h, h->g_root, Rc * 4)); CTKCHK(ensure(h, h->g_idmap, Rc * 4));
        }
        h->runs_cap = (uint32_t)std::min<size_t>(Rc, 0xffffffffu);
        c.launched = {false, false, false, false, false, false};       // whatever ran speculatively ran on too small buffers
        if (c.spec) c.label_forms |= CTK_LABEL_DISCARDED;
    }
    if (c.defer_compact) {
        // room for the halo's components in front of the shard's own (at most one per two pixels of a row)
        const size_t Rd = (size_t)h->runs_cap + (size_t)c.ny * ((size_t)c.nx / 2 + 1);
        CTKCHK(ensure(h, h->d_mrep, Rd * 4)); CTKCHK(ensure(h, h->d_box, Rd * 8)); CTKCHK(ensure(h, h->d_area, Rd * 16)); CTKCHK(ensure(h, h->d_comp_t, Rd * 4));
    }
    if (h->need_glb) {
        const size_t Rc = h->runs_cap;
        CTKCHK(ensure(h, h->g_x0, Rc * 2)); CTKCHK(ensure(h, h->g_x1, Rc * 2)); CTKCHK(ensure(h, h->g_y, Rc * 2));
        CTKCHK(ensure(h, h->g_parent, Rc * 4)); CTKCHK(ensure(h, h->g_root, Rc * 4)); CTKCHK(ensure(h, h->g_idmap, Rc * 4));
        CTKCHK(ensure(h, h->g_rs, (size_t)c.T * (c.ny + 1) * 4));
    }
    return CTK_OK;
}

// what the speculative launch did not cover, and the set the next call will launch speculatively
static int label2d_finish_labels(ctk_handle *h, Label2dCall &c)
{
    if (c.T > 0) {
        const CtkLabelPlan p = ctk_label_plan(c.T, c.ny, c.shape, h->max_runs_step, c.launched);
        if (ctk_variants_any(p.missing)) {
            HT("before label2d launch");
            Timer tm(h, CTK_K_LABEL2D);
            CTKCHK(launch_label2d(h, c, p.missing, h->runs_cap));
        }
        h->spec_set = p.next;
        h->spec_ny = c.ny; h->spec_nx = c.nx; h->spec_T = c.T;
    }
    h->stats[CTK_S_LABEL_FORMS] = c.label_forms; h->stats[CTK_S_ROWCOUNT_THREADS] = c.rc_launched; h->stats[CTK_S_ROWCOUNT_GROUPS] = c.rc_groups; h->stats[CTK_S_DEVICE_CUS] = h->n_cus;
    return CTK_OK;
}

// the dense component tables of the shard (not with defer_compact: shard_label2d_impl)
static int label2d_compact(ctk_handle *h, const Label2dCall &c)
{
    const int64_t T = c.T;
    hipStream_t s = h->stream;
    h->fz_init = false;
    if (c.defer_compact) return CTK_OK;
    if (T > 0 && h->use_device_resolve && async_wanted(h)) {
        // fused one-call path: prefix of the component counts, compaction and the initialisation of the resolver's per-component
        // arrays in one launch (k_compact_init)
        const size_t R = h->total_runs ? h->total_runs : 1;
        CTKCHK(ensure(h, h->rv_F, R * 16)); CTKCHK(ensure(h, h->rv_B, R * 16));
        CTKCHK(ensure(h, h->rv_keep0, R)); CTKCHK(ensure(h, h->rv_keep1, R));
        CTKCHK(ensure(h, h->rv_touch, R * 4)); CTKCHK(ensure(h, h->rv_parent, R * 4));
        CTKCHK(ensure(h, h->rv_changed, (size_t)(CTK_MAX_JACOBI + 8) * CTK_CHG_SLOTS * 4));
        CTKCHK(ensure(h, h->rv_scalars, 64));
        CTKCHK(ensure(h, h->rv_pstate, (size_t)(T + 1) * 4 * CTK_PSTATE_STRIDE));
        CompInit ci;
        ci.F = P<int64_t>(h->rv_F); ci.B = P<int64_t>(h->rv_B); ci.keep0 = P<uint8_t>(h->rv_keep0); ci.keep1 = P<uint8_t>(h->rv_keep1);
        ci.touch = P<uint32_t>(h->rv_touch); ci.parent = P<uint32_t>(h->rv_parent); ci.changed = P<uint32_t>(h->rv_changed);
        ci.ambig = P<uint32_t>(h->rv_scalars) + 1; ci.pstate = P<uint32_t>(h->rv_pstate);
        ci.next_tiny = (const int32_t *)(P<int64_t>(h->wlo) + 2 * (size_t)h->ny);
        ci.nchanged = (CTK_MAX_JACOBI + 1) * CTK_CHG_SLOTS; ci.pstride = CTK_PSTATE_STRIDE; ci.T = T;
        ci.base_ptr = nullptr; ci.ovr_slot = nullptr; ci.amb_cnt = nullptr; ci.dcount = nullptr; ci.bsum = nullptr;
        Timer tm(h, CTK_K_SCAN);
        if (T > 4 * CTK_CI_BLOCK) {                                // (every workgroup sums the counts in front of it: two levels beyond a few thousand steps)
            const int nb = (int)((T + CTK_CI_BLOCK - 1) / CTK_CI_BLOCK);
            CTKCHK(ensure(h, h->ci_bsum, (size_t)nb * 4));
            k_sum_blocks<<<nb, CTK_CI_BLOCK, 0, s>>>(P<uint32_t>(h->ncomp), T, P<uint32_t>(h->ci_bsum));
            ci.bsum = P<uint32_t>(h->ci_bsum);
        }
        // (round 6: the same work inside k_overlap -- one launch less -- was built and measured: k_scan group -6.5 us, k_overlap +8.3 us; the
        // small kernels of this pass cost their dependent loads and their instructions, not their launches.  NOTES round 6.)
        k_compact_init<<<(int)T, ctk_compact_init_threads(CTK_PATH_FUSED, T, h->small_threads[2]), 0, s>>>(
            P<uint32_t>(h->run_base), P<uint32_t>(h->ncomp), CPX(h), P<uint32_t>(h->cs_mrep), P<uint32_t>(h->cs_box), P<int64_t>(h->cs_area),
            P<uint32_t>(h->d_mrep), P<uint16_t>(h->d_box), P<int64_t>(h->d_area), P<uint32_t>(h->d_comp_t), ci);
        HIPCHK(hipGetLastError());
        h->fz_init = true;
    } else {
        Timer tm(h, CTK_K_SCAN);
        CTKCHK(launch_scan_u32(h, P<uint32_t>(h->ncomp), T, CPX(h)));
        HIPCHK(hipGetLastError());
        if (T > 0) {
            k_compact_comps<<<(int)T, 256, 0, s>>>(P<uint32_t>(h->run_base), P<uint32_t>(h->ncomp), CPX(h), P<uint32_t>(h->cs_mrep),
                                                   P<uint32_t>(h->cs_box), P<int64_t>(h->cs_area), P<uint32_t>(h->d_mrep), P<uint16_t>(h->d_box),
                                                   P<int64_t>(h->d_area), P<uint32_t>(h->d_comp_t));
            HIPCHK(hipGetLastError());
        }
    }
    return CTK_OK;
}

// defer_compact (time-sharded path): the dense component tables are built after the halo has arrived, because the halo's
// components come first in them
static int shard_label2d_impl(ctk_handle *h, const void *anom_dev, bool f64, int64_t T, int ny, int nx, const double *thr,
                              int cmp_op, const float *wrow, int has_prev, bool defer_compact = false)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    Label2dCall c = {};
    c.anom_dev = anom_dev; c.f64 = f64; c.T = T; c.ny = ny; c.nx = nx; c.thr = thr; c.cmp_op = cmp_op; c.wrow = wrow; c.defer_compact = defer_compact;
    CTKCHK(label2d_begin(h, c, has_prev));
    CTKCHK(label2d_stage_inputs(h, c));
    CTKCHK(label2d_upload(h, c));
    CTKCHK(label2d_threshold(h, c));
    CTKCHK(label2d_rowcount(h, c));
    CTKCHK(label2d_speculate(h, c));
    CTKCHK(label2d_wait_scan(h, c));
    CTKCHK(label2d_regrow(h, c));
    CTKCHK(label2d_finish_labels(h, c));
    CTKCHK(label2d_compact(h, c));
    h->state = ST_LABELLED;
    return CTK_OK;
}

extern "C" int ctk_shard_label2d(ctk_handle *h, const float *anom_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                                 const float *wrow, int has_prev)
{
    if (h && !h->seg_starts.empty()) return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d: segments are set on this handle (ctk_set_segments); the staged entries do not take them");
    if (h && T > 0 && !thr) return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d: thr is NULL (the staged entries take per-step thresholds, not a threshold field)");
    return shard_label2d_impl(h, anom_dev, false, T, ny, nx, thr, cmp_op, wrow, has_prev);
}
extern "C" int ctk_shard_label2d_f64(ctk_handle *h, const double *anom_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                                     const float *wrow, int has_prev)
{
    if (h && !h->seg_starts.empty()) return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d_f64: segments are set on this handle (ctk_set_segments); the staged entries do not take them");
    if (h && T > 0 && !thr) return ctk_set_error(CTK_E_INVALID, "ctk_shard_label2d_f64: thr is NULL (the staged entries take per-step thresholds, not a threshold field)");
    return shard_label2d_impl(h, anom_dev, true, T, ny, nx, thr, cmp_op, wrow, has_prev);
}

// ------------------------------------------------------------------------------------------------
// halo (last labelled timestep of this shard, for the next rank)
//   layout: [uint64 mask[ny*W]] [uint16 wstart[ny*W] (padded to 8 B)] [uint32 rowstart[ny] (padded)] [uint32 run_comp[max]]
// ------------------------------------------------------------------------------------------------
static size_t halo_off_wstart(const ctk_handle *h) { return (size_t)h->ny * h->W * 8; }
static size_t halo_off_rowstart(const ctk_handle *h) { return halo_off_wstart(h) + ctk_align8((size_t)h->ny * h->W * 2); }
static size_t halo_off_runcomp(const ctk_handle *h) { return halo_off_rowstart(h) + ctk_align8((size_t)h->ny * 4); }
static size_t halo_max_bytes(const ctk_handle *h) { return halo_off_runcomp(h) + (size_t)h->ny * ((size_t)h->nx / 2 + 1) * 4; }

extern "C" int ctk_shard_halo_size(ctk_handle *h, size_t *max_bytes)
{
    if (!h || !max_bytes) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state < ST_LABELLED) return ctk_set_error(CTK_E_STATE, "ctk_shard_halo_size before ctk_shard_label2d");
    *max_bytes = halo_max_bytes(h);
    return CTK_OK;
}

extern "C" int ctk_shard_halo_export(ctk_handle *h, void **blob_dev, size_t *nbytes)
{
    if (!h || !blob_dev || !nbytes) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state < ST_LABELLED) return ctk_set_error(CTK_E_STATE, "ctk_shard_halo_export before ctk_shard_label2d");
    HIPCHK(hipSetDevice(h->device));
    CTKCHK(ensure(h, h->halo_out, halo_max_bytes(h)));
    char *dst = (char *)h->halo_out.p;
    hipStream_t s = h->stream;
    if (h->T > 0) {
        const int64_t t = h->T - 1;
        const uint32_t hb_t = h->rb_last, n = h->rb_total - h->rb_last;       // run_base[T-1], runs of the last timestep
        HIPCHK(hipMemcpyAsync(dst, P<uint64_t>(h->mask) + t * h->ny * h->W, (size_t)h->ny * h->W * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(dst + halo_off_wstart(h), P<uint16_t>(h->wstart) + t * h->ny * h->W, (size_t)h->ny * h->W * 2, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(dst + halo_off_rowstart(h), P<uint32_t>(h->rowstart) + t * h->ny, (size_t)h->ny * 4, hipMemcpyDeviceToDevice, s));
        if (n) HIPCHK(hipMemcpyAsync(dst + halo_off_runcomp(h), P<uint32_t>(h->run_comp) + hb_t, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        *nbytes = halo_off_runcomp(h) + (size_t)n * 4;
    } else {
        HIPCHK(hipMemsetAsync(dst, 0, halo_off_runcomp(h), s));
        *nbytes = halo_off_runcomp(h);
    }
    HIPCHK(hipStreamSynchronize(s));
    *blob_dev = dst;
    return CTK_OK;
}

extern "C" int ctk_shard_halo_import(ctk_handle *h, const void *blob_dev, size_t nbytes)
{
    if (!h || !blob_dev) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state != ST_LABELLED) return ctk_set_error(CTK_E_STATE, "ctk_shard_halo_import needs a labelled shard");
    if (nbytes < halo_off_runcomp(h) || nbytes > halo_max_bytes(h)) return ctk_set_error(CTK_E_INVALID, "halo blob has %zu bytes, expected %zu..%zu", nbytes, halo_off_runcomp(h), halo_max_bytes(h));
    HIPCHK(hipSetDevice(h->device));
    CTKCHK(ensure(h, h->halo_in, halo_max_bytes(h)));
    h->halo_in_zero = false;                                     // (the blob overwrites the HaloHeader a first time shard keeps zeroed)
    HIPCHK(hipMemcpyAsync(h->halo_in.p, blob_dev, nbytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->halo_valid = true;
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// stage 2
// ------------------------------------------------------------------------------------------------
static int launch_overlap(ctk_handle *h)
{
    OverlapArgs a;
    a.mask = P<uint64_t>(h->mask); a.wstart = P<uint16_t>(h->wstart); a.rowstart = P<uint32_t>(h->rowstart); a.run_base = P<uint32_t>(h->run_base);
    a.run_comp = P<uint32_t>(h->run_comp);
    const char *hl = (const char *)h->halo_in.p;
    const size_t o0 = h->halo_v2 ? 16 : 0;                               // (HaloHeader of ctk_sharded.hip)
    a.halo_mask = (const uint64_t *)(hl ? hl + o0 : nullptr);
    a.halo_wstart = hl ? (const uint16_t *)(hl + o0 + halo_off_wstart(h)) : nullptr;
    a.halo_rowstart = hl ? (const uint32_t *)(hl + o0 + halo_off_rowstart(h)) : nullptr;
    a.halo_run_comp = hl ? (const uint32_t *)(hl + o0 + halo_off_runcomp(h)) : nullptr;
    a.has_prev = (h->has_prev && hl) ? 1 : 0;
    a.pairs = P<CtkPair>(h->pairs); a.pair_cap = h->pair_cap; a.counters = P<uint32_t>(h->counters);
    a.pair_base = P<uint32_t>(h->pair_base); a.pair_cnt = P<uint32_t>(h->pair_cnt);
    a.wlo = P<int64_t>(h->wlo); a.whi = P<int64_t>(h->wlo) + h->ny;
    a.ny = h->ny; a.nx = h->nx; a.W = h->W;
    a.cprefix = nullptr; a.mrep = nullptr; a.p_rc = nullptr; a.p_rd = nullptr; a.p_gc = nullptr; a.p_gd = nullptr; a.F = nullptr;
    a.pslot = 0; a.upair_cap = h->pair_cap;
    h->fz_pslot = 0;
    if (h->fz_init && (uint64_t)h->T * CTK_PSLOT + 4096 <= (uint64_t)h->pair_cap) {
        a.pslot = CTK_PSLOT; a.upair_cap = h->pair_cap - (uint32_t)(h->T * CTK_PSLOT);
        h->fz_pslot = CTK_PSLOT;
    }
    if (h->fz_init) {
        const size_t PC = h->pair_cap ? h->pair_cap : 1;
        CTKCHK(ensure(h, h->rv_prc, PC * 4)); CTKCHK(ensure(h, h->rv_prd, PC * 4)); CTKCHK(ensure(h, h->rv_pgc, PC * 4)); CTKCHK(ensure(h, h->rv_pgd, PC * 4));
        a.cprefix = CPX(h); a.mrep = P<uint32_t>(h->d_mrep); a.F = P<int64_t>(h->rv_F);
        a.p_rc = P<uint32_t>(h->rv_prc); a.p_rd = P<uint32_t>(h->rv_prd); a.p_gc = P<uint32_t>(h->rv_pgc); a.p_gd = P<uint32_t>(h->rv_pgd);
    }
    Timer tm(h, CTK_K_OVERLAP);
    OverlapArgsSeg as;                                                   // (segment breaks: the SEG builds, which read the edge table)
    static_cast<OverlapArgs &>(as) = a;
    as.seg_edge = h->seg_cur;
    const int form = ctk_overlap_form(h->T, h->ny, h->W);
#define CTK_OVERLAP(OVB, TH, WPE)                                                                        \
    case CTK_OVERLAP_CODE(OVB, TH, WPE):                                                                 \
        if (as.seg_edge) k_overlap<OVB, TH, WPE, true><<<(int)h->T, TH, 0, h->stream>>>(as);             \
        else k_overlap<OVB, TH, WPE><<<(int)h->T, TH, 0, h->stream>>>(a);                                \
        break
    switch (form) {
    CTK_OVERLAP(4, 128, 5);
    CTK_OVERLAP(4, 512, 1);
    CTK_OVERLAP(4, 256, 1);
    CTK_OVERLAP(5, 256, 1);
    CTK_OVERLAP(6, 256, 1);
    CTK_OVERLAP(8, 256, 1);
    default: return ctk_set_error(CTK_E_INTERNAL, "k_overlap: no instance of form %d", form);
    }
#undef CTK_OVERLAP
    h->stats[CTK_S_OVERLAP_FORM] = (as.seg_edge ? CTK_OVERLAP_SEG : 0) + form;
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

extern "C" int ctk_shard_overlap(ctk_handle *h)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (h->state != ST_LABELLED) return ctk_set_error(CTK_E_STATE, "ctk_shard_overlap needs ctk_shard_label2d first");
    HIPCHK(hipSetDevice(h->device));
    if (h->has_prev && (!h->halo_in.p || !h->halo_valid))
        return ctk_set_error(CTK_E_STATE, "ctk_shard_overlap: has_prev set but no halo imported since ctk_shard_label2d");
    size_t want = (size_t)h->total_runs / 2 + (size_t)h->T * 8 + 4096;
    if (h->fz_init) want = std::max<size_t>(want, (size_t)h->T * CTK_PSLOT + (size_t)h->T * 8 + 8192);       // fixed slots per timestep + ungrouped
    if (want > 0x7fffffffull) want = 0x7fffffffull;
    if (h->pair_cap < want || !h->pairs.p) {
        CTKCHK(ensure(h, h->pairs, want * sizeof(CtkPair)));
        h->pair_cap = (uint32_t)std::min<size_t>(h->pairs.cap / sizeof(CtkPair), 0x7fffffffull);
    }
    if (h->debug_pair_cap) { h->pair_cap = std::min(h->pair_cap, h->debug_pair_cap); h->debug_pair_cap = 0; }
    CTKCHK(ensure(h, h->pair_base, (size_t)h->T * 4));
    CTKCHK(ensure(h, h->pair_cnt, (size_t)h->T * 4));
    if (h->T > 0) CTKCHK(launch_overlap(h));
    h->state = ST_OVERLAPPED;
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// tables: download into the blob layout of ctk_tables.h
// ------------------------------------------------------------------------------------------------
static int build_tables_blob(ctk_handle *h, bool to_device, const void **blob, size_t *nbytes)
{
    if (!h || !blob || !nbytes) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state != ST_OVERLAPPED && h->state != ST_TABLES) return ctk_set_error(CTK_E_STATE, "ctk_shard_tables needs ctk_shard_overlap first");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const double t0 = now_ms();
    uint32_t *hc = (uint32_t *)h->h_small.p + (h->T + 2);                       // after the run_base copy
    uint32_t cnt[CTK_CNT_N], ctot = 0, stot = 0;
    // seam rows: row-indexed scratch -> dense (t, y) order
    CTKCHK(launch_scan_u32(h, P<uint32_t>(h->seam_cnt), h->T, P<uint32_t>(h->seam_off)));
    HIPCHK(hipGetLastError());
    for (int attempt = 0;; attempt++) {
        HIPCHK(hipMemcpyAsync(hc, h->counters.p, CTK_CNT_N * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hc + CTK_CNT_N, CPX(h) + h->T, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hc + CTK_CNT_N + 1, P<uint32_t>(h->seam_off) + h->T, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        memcpy(cnt, hc, sizeof(cnt));
        ctot = hc[CTK_CNT_N];
        stot = hc[CTK_CNT_N + 1];
        if (!(cnt[CTK_CNT_OVERFLOW] & CTK_OVF_PAIRS) && (uint64_t)cnt[CTK_CNT_PAIRS] + cnt[CTK_CNT_UPAIRS] <= h->pair_cap) break;
        if (attempt >= 6) return ctk_set_error(CTK_E_RANGE, "pair table keeps overflowing");
        h->stats[CTK_S_PAIR_REGROW]++;
        // grow the pair table to what was asked for and redo the histogram
        size_t want = std::max<size_t>((size_t)cnt[CTK_CNT_PAIRS] + cnt[CTK_CNT_UPAIRS] + 1024, (size_t)h->pair_cap * 2);
        if (want > 0xfffffff0ull) return ctk_set_error(CTK_E_RANGE, "pair table beyond 2^32 records");
        CTKCHK(ensure(h, h->pairs, want * sizeof(CtkPair)));
        h->pair_cap = (uint32_t)std::min<size_t>(h->pairs.cap / sizeof(CtkPair), 0xfffffff0ull);
        uint32_t zero[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(P<uint32_t>(h->counters) + CTK_CNT_PAIRS, zero, 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(P<uint32_t>(h->counters) + CTK_CNT_UPAIRS, zero, 4, hipMemcpyHostToDevice, s));
        uint32_t ovf = cnt[CTK_CNT_OVERFLOW] & ~CTK_OVF_PAIRS;
        HIPCHK(hipMemcpyAsync(P<uint32_t>(h->counters) + CTK_CNT_OVERFLOW, &ovf, 4, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
        h->fz_init = false;                                    // (the synchronous resolver prepares the pair arrays itself)
        CTKCHK(launch_overlap(h));
    }
    h->total_comps = ctot;
    const int64_t T = h->T, NC = ctot, NPG = cnt[CTK_CNT_PAIRS], NPU = cnt[CTK_CNT_UPAIRS], NP = NPG + NPU, NS = stot;
    if (NS) {
        CTKCHK(ensure(h, h->d_seams, (size_t)NS * sizeof(CtkSeam)));
        k_compact_seams<<<(int)T, 256, 0, s>>>(P<CtkSeam>(h->seams), P<uint32_t>(h->seam_cnt), P<uint32_t>(h->seam_off), h->ny, P<CtkSeam>(h->d_seams));
        HIPCHK(hipGetLastError());
    }
    const size_t bytes = ctk_blob_bytes(T, NC, NP, NS);
    char *p;
    if (to_device) { CTKCHK(ensure(h, h->d_blob, bytes)); p = (char *)h->d_blob.p; }
    else { CTKCHK(ensure_host(h, h->h_blob, bytes)); p = (char *)h->h_blob.p; }
    const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    CtkBlobHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.magic = CTK_BLOB_MAGIC; hdr.T = T; hdr.ny = h->ny; hdr.nx = h->nx; hdr.wshift = h->wshift; hdr.limb_bits = h->limb_bits; hdr.has_prev = (h->has_prev && h->halo_in.p) ? 1 : 0;
    hdr.ncomps = NC; hdr.npairs = NP; hdr.nseams = NS; hdr.npairs_grouped = NPG;
    if (to_device) HIPCHK(hipMemcpyAsync(p, &hdr, sizeof(hdr), hipMemcpyHostToDevice, s)); else memcpy(p, &hdr, sizeof(hdr));
    p += sizeof(CtkBlobHeader);
    if (T) HIPCHK(hipMemcpyAsync(p, h->ncomp.p, (size_t)T * 4, kind, s));
    p += ctk_align8((size_t)T * 4);
    if (NC) HIPCHK(hipMemcpyAsync(p, h->d_mrep.p, (size_t)NC * 4, kind, s));
    p += ctk_align8((size_t)NC * 4);
    if (NC) HIPCHK(hipMemcpyAsync(p, h->d_box.p, (size_t)NC * 8, kind, s));
    p += ctk_align8((size_t)NC * 8);
    if (NC) HIPCHK(hipMemcpyAsync(p, h->d_area.p, (size_t)NC * 16, kind, s));
    p += (size_t)NC * 16;
    if (NPG) HIPCHK(hipMemcpyAsync(p, h->pairs.p, (size_t)NPG * sizeof(CtkPair), kind, s));
    if (NPU) HIPCHK(hipMemcpyAsync(p + (size_t)NPG * sizeof(CtkPair), P<CtkPair>(h->pairs) + (h->pair_cap - NPU), (size_t)NPU * sizeof(CtkPair), kind, s));
    p += (size_t)NP * sizeof(CtkPair);
    if (NS) HIPCHK(hipMemcpyAsync(p, h->d_seams.p, (size_t)NS * sizeof(CtkSeam), kind, s));
    p += (size_t)NS * sizeof(CtkSeam);
    if (T) HIPCHK(hipMemcpyAsync(p, h->pair_base.p, (size_t)T * 4, kind, s));
    p += ctk_align8((size_t)T * 4);
    if (T) HIPCHK(hipMemcpyAsync(p, h->pair_cnt.p, (size_t)T * 4, kind, s));
    HIPCHK(hipStreamSynchronize(s));
    h->h_blob_bytes = bytes;
    *blob = to_device ? h->d_blob.p : h->h_blob.p;
    *nbytes = bytes;
    h->ms[CTK_T_D2H] += now_ms() - t0;
    h->state = ST_TABLES;
    return CTK_OK;
}

extern "C" int ctk_shard_tables(ctk_handle *h, const void **blob, size_t *nbytes) { return build_tables_blob(h, false, blob, nbytes); }

// ------------------------------------------------------------------------------------------------
// stage 3
// ------------------------------------------------------------------------------------------------
static FoldArgs fold_args(const ctk_handle *h)
{
    FoldArgs f;
    f.ops = P<CtkOp>(h->ops); f.first = P<int32_t>(h->op_first); f.next = h->d_op_next; f.nops = h->nops;
    return f;
}

// ops in execution order -> device, plus the per-label chains (first[label], next[op]) the folds walk.
// One pinned staging block, one H2D copy: [CtkOp ops[n]] [int32 next[n]] [int32 hi_label[nf]] [int32 first_op[nf]]
static int prepare_op_first(ctk_handle *h, int64_t n_labels)
{
    CTKCHK(ensure(h, h->op_first, (size_t)(n_labels + 1) * 4));
    HIPCHK(hipMemsetAsync(h->op_first.p, 0xff, (size_t)(n_labels + 1) * 4, h->stream));    // all -1
    return CTK_OK;
}

static int upload_ops(ctk_handle *h, const CtkOp *ops, int64_t nops, int64_t n_labels)
{
    hipStream_t s = h->stream;
    h->nops = (int32_t)nops;
    if (!nops) return CTK_OK;
    const size_t bytes = (size_t)nops * (sizeof(CtkOp) + 4 + 8);
    CTKCHK(ensure_host(h, h->h_ops, bytes));
    CTKCHK(ensure(h, h->ops, bytes));
    CtkOp *s_ops = (CtkOp *)h->h_ops.p;
    int32_t *s_next = (int32_t *)(s_ops + nops), *s_label = s_next + nops, *s_first = s_label + nops;
    memcpy(s_ops, ops, (size_t)nops * sizeof(CtkOp));
    std::vector<int32_t> &last = h->sd_last;                                   // scratch: last op seen per `hi`
    last.assign((size_t)n_labels + 1, -1);
    size_t nf = 0;
    for (int32_t i = 0; i < (int32_t)nops; i++) {
        const int32_t hi = ops[i].hi;
        s_next[i] = -1;
        if (last[(size_t)hi] >= 0) s_next[last[(size_t)hi]] = i; else { s_label[nf] = hi; s_first[nf] = i; nf++; }
        last[(size_t)hi] = i;
    }
    HIPCHK(hipMemcpyAsync(h->ops.p, h->h_ops.p, bytes, hipMemcpyHostToDevice, s));
    const int32_t *d_next = (const int32_t *)(P<CtkOp>(h->ops) + nops);
    h->d_op_next = d_next;
    k_scatter_i32<<<(int)((nf + 255) / 256), 256, 0, s>>>(d_next + nops, d_next + 2 * nops, (int)nf, P<int32_t>(h->op_first));
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// Same for the device-resolver path: the seam driver already holds the chains (dense first[] / next[]).  The staging
// block is read by the ingest kernel straight from pinned host memory (no copy command).
static int upload_ops_dense(ctk_handle *h, const std::vector<CtkOp> &ops, const int32_t *orig, int64_t nd)
{
    hipStream_t s = h->stream;
    const int64_t nops = (int64_t)ops.size();
    h->nops = (int32_t)nops;
    const size_t bytes = (size_t)std::max<int64_t>(nops, 1) * (sizeof(CtkOp) + 4 + 8);
    CTKCHK(ensure_host(h, h->h_ops, bytes));
    CTKCHK(ensure(h, h->ops, bytes));
    CtkOp *s_ops = (CtkOp *)h->h_ops.p;
    int32_t *s_next = (int32_t *)(s_ops + nops), *s_label = s_next + nops, *s_first = s_label + nops;
    int32_t nf = 0;
    if (nops) {
        memcpy(s_ops, ops.data(), (size_t)nops * sizeof(CtkOp));
        memcpy(s_next, h->sd.next.data(), (size_t)nops * 4);
        for (int64_t d = 0; d < nd; d++)
            if (h->sd.first[(size_t)d] >= 0) { s_label[nf] = orig[d]; s_first[nf] = h->sd.first[(size_t)d]; nf++; }
    }
    int32_t *d_next = (int32_t *)(P<CtkOp>(h->ops) + nops);
    h->d_op_next = d_next;
    const int64_t work = std::max<int64_t>(nops * 9, h->n_labels + 1);
    k_ops_ingest<<<(int)std::min<int64_t>((work + 255) / 256, 1024), 256, 0, s>>>((const int32_t *)h->h_ops.p, nops, nf, P<int32_t>(h->ops), P<int32_t>(h->op_first),
                                                                                  P<int32_t>(h->ext), h->n_labels, P<uint32_t>(h->counters));
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

static int launch_extents(ctk_handle *h, bool ext_filled = false, bool with_final = false)
{
    hipStream_t s = h->stream;
    CTKCHK(ensure(h, h->ext, (size_t)(h->n_labels + 1) * 8));
    Timer tm(h, CTK_K_EXTENT);
    const int64_t n1 = h->n_labels + 1;
    if (!ext_filled) {                                            // (the device-resolver path did it in k_ops_ingest)
        k_fill_ext<<<(int)std::min<int64_t>((n1 + 255) / 256, 4096), 256, 0, s>>>(P<int32_t>(h->ext), h->n_labels, P<uint32_t>(h->counters));
        HIPCHK(hipGetLastError());
    }
    if (h->T > 0) {
        ExtentArgs a;
        a.guard = h->guard_on ? P<uint32_t>(h->counters) : nullptr;
        a.mask = P<uint64_t>(h->mask); a.rowstart = P<uint32_t>(h->rowstart); a.run_base = P<uint32_t>(h->run_base);
        a.run_comp = P<uint32_t>(h->run_comp); a.ncomp = P<uint32_t>(h->ncomp); a.cprefix = CPX(h);
        a.comp_label = P<int32_t>(h->comp_label); a.lab = with_final ? P<int32_t>(h->rv_lab) : nullptr; a.comp_label_w = P<int32_t>(h->comp_label);
        a.box = P<uint16_t>(h->d_box); a.ext = P<int32_t>(h->ext); a.n_labels = h->n_labels; a.t_begin = h->t_begin;
        a.fold = fold_args(h); a.ny = h->ny; a.nx = h->nx; a.W = h->W;
        a.T = h->T;
        const int form = ctk_extent_form(h->T, h->nx, h->small_threads[0]);
        if (form == CTK_EXTENT_BLK) k_extent_blk<<<(int)((h->T + EX_TW - 1) / EX_TW), 64 * EX_TW, 0, s>>>(a);
        else k_extent<<<(int)h->T, form, 0, s>>>(a);
        h->stats[CTK_S_EXTENT_FORM] = form;
        HIPCHK(hipGetLastError());
    }
    return CTK_OK;
}

extern "C" int ctk_shard_extents(ctk_handle *h, const ctk_result *r, int shard, int64_t t_begin, int32_t **ext_dev, int64_t *n_labels)
{
    if (!h || !r) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state != ST_TABLES) return ctk_set_error(CTK_E_STATE, "ctk_shard_extents needs ctk_shard_tables first");
    if (shard < 0 || shard >= r->nshards) return ctk_set_error(CTK_E_INVALID, "shard %d out of range", shard);
    const int64_t c0 = r->shard_comp_off[shard], c1 = r->shard_comp_off[shard + 1];
    if (c1 - c0 != (int64_t)h->total_comps || r->shard_t_off[shard + 1] - r->shard_t_off[shard] != h->T)
        return ctk_set_error(CTK_E_INVALID, "result does not belong to this shard (%lld components vs %u)", (long long)(c1 - c0), h->total_comps);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const double t0 = now_ms();
    h->n_labels = r->n_labels; h->t_begin = t_begin;
    CTKCHK(ensure(h, h->comp_label, (size_t)(c1 - c0) * 4));
    if (c1 > c0) HIPCHK(hipMemcpyAsync(h->comp_label.p, r->comp_label + c0, (size_t)(c1 - c0) * 4, hipMemcpyHostToDevice, s));
    CTKCHK(prepare_op_first(h, r->n_labels));
    CTKCHK(upload_ops(h, r->ops, r->nops, r->n_labels));
    HIPCHK(hipStreamSynchronize(s));
    h->ms[CTK_T_H2D] += now_ms() - t0;
    CTKCHK(launch_extents(h));
    if (ext_dev) *ext_dev = P<int32_t>(h->ext);
    if (n_labels) *n_labels = r->n_labels;
    h->state = ST_EXTENTS;
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// device resolver (single shard): R1..R5 of ctk_resolve_dev.hip + the host seam driver
// ------------------------------------------------------------------------------------------------
// Tables the device resolver works on: the shard's own (single GPU) or the concatenation of all shards'.
struct ResolveIn {
    int64_t T;                                   // timesteps covered by the tables
    size_t R;                                    // upper bound of the number of components
    const uint32_t *ncomp, *cprefix, *mrep, *comp_t;
    const uint16_t *box;
    const int64_t *area;
    const CtkPair *pairs;
    uint32_t pair_cap;
    const uint32_t *counters;                    // [CTK_CNT_PAIRS] grouped, [CTK_CNT_UPAIRS] ungrouped, [CTK_CNT_OVERFLOW]
    const uint32_t *pair_base, *pair_cnt;
    const CtkSeam *seams;
    const uint32_t *seam_cnt, *seam_off;         // record i of timestep t: seams[seam_off[t] + i]
    int64_t seam_cap;                            // upper bound of the surviving seam rows
    int32_t *comp_label;                         // out: [components]
    size_t extra_dense = 0;                      // dense label ids beyond those of candidate records (time shards)
};

// Filter launches: with segment breaks (h->seg_cur) the SEG builds, which never filter the first and last step of a segment;
// else the SEG = false builds, the kernels the unsegmented call has always launched.
static void launch_rs_pass(const ctk_handle *h, int grid, const ResolveDev &r, int it, const uint32_t *pair_base, const uint32_t *pair_cnt, uint8_t *tdirty)
{
    if (h->seg_cur) k_rs_pass<true><<<grid, 64, 0, h->stream>>>(r, it, pair_base, pair_cnt, tdirty, h->seg_cur);
    else k_rs_pass<false><<<grid, 64, 0, h->stream>>>(r, it, pair_base, pair_cnt, tdirty, nullptr);
}
// two_pc: the build with two workgroups per CU (k_rs_pass_blk_2pc)
static void launch_rs_pass_blk(const ctk_handle *h, bool two_pc, int nb, const ResolveDev &r, int it0, int K, const uint32_t *pair_base, const uint32_t *pair_cnt,
                               uint32_t *pstate, int prep_inline, int do_unite)
{
    hipStream_t s = h->stream;
    if (h->seg_cur) {
        if (two_pc) k_rs_pass_blk_2pc<true><<<nb, 64 * PB_G, 0, s>>>(r, it0, K, pair_base, pair_cnt, pstate, prep_inline, do_unite, h->seg_cur);
        else k_rs_pass_blk<true><<<nb, 64 * PB_G, 0, s>>>(r, it0, K, pair_base, pair_cnt, pstate, prep_inline, do_unite, h->seg_cur);
    } else {
        if (two_pc) k_rs_pass_blk_2pc<false><<<nb, 64 * PB_G, 0, s>>>(r, it0, K, pair_base, pair_cnt, pstate, prep_inline, do_unite, nullptr);
        else k_rs_pass_blk<false><<<nb, 64 * PB_G, 0, s>>>(r, it0, K, pair_base, pair_cnt, pstate, prep_inline, do_unite, nullptr);
    }
}

// returns CTK_OK, a negative error, or +1 = "take the host path" (pair table overflow / filter not converged)
// work space + kernel argument block of the resolver kernels for the tables `in`
struct ResolvePlan {
    ResolveDev r;
    CandMail mail;
    int nsb = 1, gc = 1, gp = 1;
};
static int rs_prepare(ctk_handle *h, const ResolveIn &in, double overlap, int twosided, ResolvePlan &pl)
{
    const size_t R = in.R ? in.R : 1;
    const size_t PC = in.pair_cap ? in.pair_cap : 1;
    const int64_t T = in.T;
    CTKCHK(ensure(h, h->rv_prc, PC * 4)); CTKCHK(ensure(h, h->rv_prd, PC * 4));
    CTKCHK(ensure(h, h->rv_pgc, PC * 4)); CTKCHK(ensure(h, h->rv_pgd, PC * 4));
    CTKCHK(ensure(h, h->rv_F, R * 16)); CTKCHK(ensure(h, h->rv_B, R * 16));
    CTKCHK(ensure(h, h->rv_keep0, R)); CTKCHK(ensure(h, h->rv_keep1, R));
    CTKCHK(ensure(h, h->rv_changed, (size_t)(CTK_MAX_JACOBI + 8) * CTK_CHG_SLOTS * 4));
    CTKCHK(ensure(h, h->rv_parent, R * 4)); CTKCHK(ensure(h, h->rv_isroot, R * 4)); CTKCHK(ensure(h, h->rv_rank, (R + 1) * 4));
    CTKCHK(ensure(h, h->rv_lab, R * 4));
    const int nsb = (int)ctk_rank_blocks(in.R);                               // blocks of the rank scan (k_rs_roots / k_rs_rank)
    CTKCHK(ensure(h, h->rv_bsum, (size_t)nsb * 4)); CTKCHK(ensure(h, h->rv_boff, (size_t)(nsb + 1) * 4));
    CTKCHK(ensure(h, h->rv_cand_cnt, (size_t)T * 4)); CTKCHK(ensure(h, h->rv_cand_off, (size_t)(T + 1) * 4));
    CTKCHK(ensure(h, h->rv_cand, (size_t)std::max<int64_t>(in.seam_cap, 1) * sizeof(CtkCand)));
    CTKCHK(ensure(h, h->rv_cand_scratch, (size_t)std::max<int64_t>(T * h->ny, 1) * sizeof(CtkCand)));
    CTKCHK(ensure(h, h->rv_seam_res, (size_t)std::max<int64_t>(T * h->ny, 1) * 8));
    CTKCHK(ensure(h, h->rv_scalars, 64));
    CTKCHK(ensure(h, h->rv_tdirty, (size_t)2 * (size_t)(T + 1)));        // two passes x (halo timestep + T)
    CTKCHK(ensure(h, h->rv_mark, R + 1));
    CTKCHK(ensure(h, h->rv_inv, R * 8)); CTKCHK(ensure(h, h->rv_ff, R * 8));
    const size_t DC = std::min<size_t>(R + 1, (size_t)2 * std::max<int64_t>(in.seam_cap, 1) + in.extra_dense);       // labels in candidate records
    CTKCHK(ensure(h, h->rv_dmap, (R + 1) * 4)); CTKCHK(ensure(h, h->rv_dorig, DC * 4)); CTKCHK(ensure(h, h->rv_dbox, DC * 24));
    CTKCHK(ensure(h, h->op_first, (R + 1) * 4));
    CTKCHK(ensure(h, h->rv_inex, R));
    CTKCHK(ensure(h, h->rv_touch, R * 4));

    ResolveDev r;
    r.ncomp = in.ncomp; r.cprefix = in.cprefix; r.mrep = in.mrep; r.comp_t = in.comp_t;
    r.box = in.box; r.A = in.area; r.pairs = in.pairs; r.counters = in.counters;
    r.pair_cap = in.pair_cap; r.T = T; r.wshift = h->wshift; r.limb_bits = h->limb_bits; r.overlap = overlap; r.twosided = twosided;
    r.p_rc = P<uint32_t>(h->rv_prc); r.p_rd = P<uint32_t>(h->rv_prd); r.p_gc = P<uint32_t>(h->rv_pgc); r.p_gd = P<uint32_t>(h->rv_pgd);
    r.F = P<int64_t>(h->rv_F); r.B = P<int64_t>(h->rv_B); r.keep0 = P<uint8_t>(h->rv_keep0); r.keep1 = P<uint8_t>(h->rv_keep1);
    r.changed = P<uint32_t>(h->rv_changed); r.parent = P<uint32_t>(h->rv_parent); r.isroot = P<uint32_t>(h->rv_isroot);
    r.rank = P<uint32_t>(h->rv_rank); r.lab = P<int32_t>(h->rv_lab); r.lab_root = nullptr;
    r.mark = P<uint8_t>(h->rv_mark); r.inv = P<double>(h->rv_inv); r.ff = P<double>(h->rv_ff);
    r.dmap = P<uint32_t>(h->rv_dmap); r.dorig = P<int32_t>(h->rv_dorig); r.dbox = P<int32_t>(h->rv_dbox); r.dcount = P<uint32_t>(h->rv_scalars); r.op_first = P<int32_t>(h->op_first);
    r.inex = P<uint8_t>(h->rv_inex); r.ambig = P<uint32_t>(h->rv_scalars) + 1; r.minlsb = h->w_minlsb;
    r.next_tiny = (const int32_t *)(P<int64_t>(h->wlo) + 2 * (size_t)h->ny); r.touch = P<uint32_t>(h->rv_touch);
    r.nh_ptr = nullptr; r.t_lo = 1; r.t_hi = (int)T - 2;                // one slab: timesteps 1 .. T-2 are filtered, no halo
    r.ovr_slot = nullptr; r.ovr_val = nullptr; r.amb_cnt = P<uint32_t>(h->rv_scalars) + 2; r.amb_list = nullptr; r.amb_cap = 0;
    r.spin_limit = h->spin_limit; r.poison = P<uint32_t>(h->counters) + CTK_CNT_POISON; r.dbg_stall = h->debug_stall;
    r.cl_parent = nullptr; r.cl_tmin = nullptr; r.cl_tmax = nullptr; r.cl_nops = nullptr; r.lbox = nullptr; r.pstate = nullptr; r.ext = nullptr; r.ext_off = 0; r.counters_w = nullptr;      // (fused one-call path only)

    const int gc = (int)std::min<size_t>((R + 255) / 256, 2048), gp = (int)std::min<size_t>((PC + 255) / 256, 2048);
    // mailbox in pinned host memory: the last resolver kernel writes scalars, candidate records and dense label tables
    // there itself -- one stream synchronisation, no copy commands.  Capacities follow the previous calls; a call that
    // needs more falls back to explicit copies and enlarges the mailbox for the next one.
    if (h->mail_want_c > h->mail_cap_c || h->mail_want_d > h->mail_cap_d || !h->h_mail.p) {
        h->mail_cap_c = std::max<size_t>(std::max<size_t>(h->mail_want_c, h->mail_cap_c), 4096);
        h->mail_cap_d = std::max<size_t>(std::max<size_t>(h->mail_want_d, h->mail_cap_d), 8192);
        CTKCHK(ensure_host(h, h->h_mail, CTK_MAIL_SCALARS * 4 + h->mail_cap_c * sizeof(CtkCand) + h->mail_cap_d * 28, true));
    }
    CandMail mail;
    mail.scal = (uint32_t *)h->h_mail.p;
    mail.cand = (CtkCand *)((char *)h->h_mail.p + CTK_MAIL_SCALARS * 4);
    mail.dorig = (int32_t *)((char *)mail.cand + h->mail_cap_c * sizeof(CtkCand));
    mail.dbox = mail.dorig + h->mail_cap_d;
    mail.cap_c = (uint32_t)h->mail_cap_c; mail.cap_d = (uint32_t)h->mail_cap_d;
    if (h->debug_mail_c) mail.cap_c = std::min(mail.cap_c, h->debug_mail_c);
    if (h->debug_mail_d) mail.cap_d = std::min(mail.cap_d, h->debug_mail_d);
    pl.r = r; pl.mail = mail; pl.nsb = nsb; pl.gc = gc; pl.gp = gp;
    return CTK_OK;
}

static int device_resolve(ctk_handle *h, const ResolveIn &in, double overlap, int twosided, bool final_in_extent = false, bool local = false)
{
    hipStream_t s = h->stream;
    const int64_t T = in.T;
    ResolvePlan pl;
    CTKCHK(rs_prepare(h, in, overlap, twosided, pl));
    ResolveDev &r = pl.r;
    CandMail &mail = pl.mail;
    const int nsb = pl.nsb, gc = pl.gc, gp = pl.gp;
    uint32_t hs[CTK_MAIL_SCALARS];
    const double t0 = now_ms();
    int it_done = 0;
    const int ROUND = h->filter_round;
    for (;;) {
        Timer tm(h, CTK_K_RESOLVE);
        if (it_done == 0) {
            k_rs_init<<<gc, 256, 0, s>>>(r);
            k_rs_pairs<<<gp, 256, 0, s>>>(r);
            k_rs_prep<<<gc, 256, 0, s>>>(r);
        }
        // overlap filter: a round of passes (passes after the fixed point return at once)
        if (T > 2)
            for (int it = it_done; it < it_done + ROUND; it++)
                launch_rs_pass(h, (int)(T - 2), r, it, in.pair_base, in.pair_cnt, P<uint8_t>(h->rv_tdirty));        // t_lo = 1 .. t_hi = T-2
        it_done += ROUND;
        if (it_done > ROUND) k_rs_parent_init<<<gc, 256, 0, s>>>(r);          // the first round's parents were set by k_rs_init
        k_rs_unite<<<gp, 256, 0, s>>>(r);
        h->stats[CTK_S_FILTER_FORMS] |= ctk_filter_bits_sync(T, h->seg_cur != nullptr);
        const uint32_t *ncp = in.cprefix + T;
        k_rs_roots<<<nsb, 256, 0, s>>>(r, P<uint32_t>(h->rv_bsum));                       // (nsb blocks of 256 components)
        k_rs_rank<<<nsb, 256, 0, s>>>(r.isroot, ncp, P<uint32_t>(h->rv_bsum), r.rank, P<uint32_t>(h->rv_boff) + nsb);
        k_rs_labels<<<gc, 256, 0, s>>>(r);
        if (T > 0) {
            k_rs_cand_mark<<<(int)T, 256, 0, s>>>(r, in.seams, in.seam_cnt, in.seam_off, h->ny, P<uint8_t>(h->rv_mark), P<int2>(h->rv_seam_res));
            k_rs_cand_groups<<<(int)((T + FZ_TW - 1) / FZ_TW), 64 * FZ_TW, 0, s>>>(r, in.seams, in.seam_cnt, in.seam_off, P<int2>(h->rv_seam_res), P<uint8_t>(h->rv_mark),
                                                   h->ny, 0, P<uint32_t>(h->rv_cand_cnt), P<CtkCand>(h->rv_cand_scratch));
        }
        CTKCHK(launch_scan_u32(h, P<uint32_t>(h->rv_cand_cnt), T, P<uint32_t>(h->rv_cand_off)));
        k_compact_cands<<<(int)std::max<int64_t>(T, 1), 64, 0, s>>>(r, P<CtkCand>(h->rv_cand_scratch), P<uint32_t>(h->rv_cand_cnt), P<uint32_t>(h->rv_cand_off),
                                                                    h->ny, P<CtkCand>(h->rv_cand), P<uint32_t>(h->rv_boff) + nsb, it_done - ROUND, ROUND, mail);
        HIPCHK(hipGetLastError());
        HT("resolver launched");
        HIPCHK(hipStreamSynchronize(s));
        HT("sync2 done");
        memcpy(hs, mail.scal, sizeof(hs));
        if ((hs[CTK_CNT_OVERFLOW] & CTK_OVF_PAIRS) || (uint64_t)hs[CTK_CNT_PAIRS] + hs[CTK_CNT_UPAIRS] > in.pair_cap) {
            h->stats[CTK_S_HOST_REASON] |= 1;
            return 1;                                                         // the host path regrows the pair table
        }
        int conv = -1;
        for (int k = 0; k < ROUND; k++) if (hs[CTK_MAIL_CHANGED + k] == 0) { conv = it_done - ROUND + k; break; }
        if (conv >= 0) { h->stats[CTK_S_FILTER_PASSES] = conv + 1; h->stats[CTK_S_FILTER_ROUNDS] = it_done / ROUND; break; }
        if (it_done + ROUND > CTK_MAX_JACOBI) { h->stats[CTK_S_HOST_REASON] |= 2; return 1; }      // very long removal cascade: host resolver
    }
    const int64_t NC = hs[CTK_MAIL_NC], ncand = hs[CTK_MAIL_NCAND], nlab = hs[CTK_MAIL_NLAB];
    // ids are int32 here; scipy (and with it the reference) switches to int64 labels for slabs of 2^31 - 2 pixels and more
    // (contrack.py:687, :751).  More ids than int32 holds must be an error, never a wrap-around.
    if (nlab > 0x7ffffffell) return ctk_set_error(CTK_E_RANGE, "%lld ids do not fit the int32 flag variable", (long long)nlab);
    const size_t nd = hs[CTK_MAIL_ND];                                        // labels on surviving seam rows (dense ids)
    h->n_labels = nlab;
    CTKCHK(ensure(h, h->ext, (size_t)(nlab + 1) * 8));
    h->stats[CTK_S_COMPONENTS] = NC; h->stats[CTK_S_PAIRS] = (int64_t)hs[CTK_CNT_PAIRS] + hs[CTK_CNT_UPAIRS]; h->stats[CTK_S_SEAM_ROWS] = ncand; h->stats[CTK_S_LABELS] = nlab;
    h->stats[CTK_S_UPAIRS] = hs[CTK_CNT_UPAIRS];
    h->stats[CTK_S_AMBIGUOUS] = hs[CTK_MAIL_AMBIG];
    if (hs[CTK_MAIL_AMBIG] && local) return 1;         // single GPU: the host resolver re-evaluates those decisions in numpy's order
    h->mail_want_c = std::max<size_t>(h->mail_want_c, (size_t)ncand + (size_t)ncand / 2);
    h->mail_want_d = std::max<size_t>(h->mail_want_d, nd + nd / 2);
    std::vector<CtkOp> &ops = h->sd_ops;
    ops.clear();
    if (ncand) {
        const size_t cb = (size_t)ncand * sizeof(CtkCand), need = cb + nd * 28;
        h->sd_cand.resize(need);
        char *dst = (char *)h->sd_cand.data();
        if ((size_t)ncand <= mail.cap_c && nd <= mail.cap_d) {
            h->ms[CTK_T_D2H] += now_ms() - t0;
            // work on a pageable copy: CPU reads of pinned memory are uncached (fine-grained) or slow (coarse-grained) on
            // this platform -- measured 173 / 111 us for the candidate loop vs 20 us + 20 us for copy + loop
            const double tc = now_ms();
            memcpy(dst, mail.cand, cb);
            memcpy(dst + cb, mail.dorig, nd * 4);
            memcpy(dst + cb + nd * 4, mail.dbox, nd * 24);
            h->stats[11] = (int64_t)((now_ms() - tc) * 1e6);
        } else {
            // the mailbox was too small for this call: explicit copies from the device arrays
            HIPCHK(hipMemcpyAsync(dst, h->rv_cand.p, cb, hipMemcpyDeviceToHost, s));
            if (nd) {
                HIPCHK(hipMemcpyAsync(dst + cb, h->rv_dorig.p, nd * 4, hipMemcpyDeviceToHost, s));
                HIPCHK(hipMemcpyAsync(dst + cb + nd * 4, h->rv_dbox.p, nd * 24, hipMemcpyDeviceToHost, s));
            }
            HIPCHK(hipStreamSynchronize(s));
            h->ms[CTK_T_D2H] += now_ms() - t0;
        }
        HT("mail copied");
        const double t1 = now_ms();
        const CtkCand *hc = (const CtkCand *)dst;
        const int32_t *ho = (const int32_t *)(dst + cb), *hb = ho + nd;
        h->sd.run(hc, ncand, ho, hb, (int64_t)nd, h->nx, ops);
        if (ctk_env().seamstats) {
            // clusters of candidate labels (connected through shared seam rows): what a parallel device-side driver would see
            std::vector<int32_t> uf(nd);
            for (size_t i = 0; i < nd; i++) uf[i] = (int32_t)i;
            auto find = [&](int32_t i) { while (uf[(size_t)i] != i) { uf[(size_t)i] = uf[(size_t)uf[(size_t)i]]; i = uf[(size_t)i]; } return i; };
            for (int64_t k = 0; k < ncand; k++) { const int32_t a = find(hc[k].ll), b = find(hc[k].lr); if (a != b) uf[(size_t)std::max(a, b)] = std::min(a, b); }
            std::vector<int32_t> nrec(nd, 0), nops(nd, 0), nrows(nd, 0), tmin(nd, INT32_MAX), tmax(nd, -1), ndiff(nd, 0);
            for (int64_t k = 0; k < ncand; k++) { const int32_t r = find(hc[k].ll); nrec[r]++; nrows[r] += (int32_t)(((uint32_t)hc[k].yy >> 16) - (hc[k].yy & 0xffff) + 1); tmin[r] = std::min(tmin[r], hc[k].t); tmax[r] = std::max(tmax[r], hc[k].t); if (hc[k].ll != hc[k].lr) ndiff[r]++; }
            std::vector<int32_t> dense_of(1);
            for (size_t i = 0; i < ops.size(); i++) { for (size_t d = 0; d < nd; d++) if (ho[d] == ops[i].hi) { nops[find((int32_t)d)]++; break; } }
            int ncl = 0, mrec = 0, mops = 0, mspan = 0, ntriv = 0; int64_t sumspan = 0;
            std::vector<int> hist(12, 0);
            for (size_t d = 0; d < nd; d++) if (nrec[d]) { ncl++; mrec = std::max(mrec, nrec[d]); mops = std::max(mops, nops[d]); mspan = std::max(mspan, tmax[d] - tmin[d] + 1); sumspan += tmax[d] - tmin[d] + 1; if (!ndiff[d]) ntriv++; int b = 0; while ((1 << b) < nrec[d]) b++; hist[std::min(b, 11)]++; }
            fprintf(stderr, "SEAMSTATS ncand %lld nd %zu ops %zu clusters %d (trivial %d) max_records %d max_ops %d max_span %d sum_span %lld hist(log2 records):", (long long)ncand, nd, ops.size(), ncl, ntriv, mrec, mops, mspan, (long long)sumspan);
            for (int b = 0; b < 12; b++) fprintf(stderr, " %d", hist[b]);
            fprintf(stderr, "\n");
            // the heaviest clusters
            std::vector<std::pair<int, int>> top;
            for (size_t d = 0; d < nd; d++) if (nrec[d]) top.emplace_back(nrec[d], (int)d);
            std::sort(top.rbegin(), top.rend());
            for (size_t i = 0; i < std::min<size_t>(top.size(), 8); i++) fprintf(stderr, "  cluster records %d rows %d ops %d span %d\n", top[i].first, nrows[top[i].second], nops[top[i].second], tmax[top[i].second] - tmin[top[i].second] + 1);
        }
        h->stats[9] = h->sd.loop_ns;                              // ns spent in the candidate loop
        h->stats[10] = h->sd.nfold;
        h->ms[CTK_T_HOST_RESOLVE] += now_ms() - t1;
        HT("driver done");
        const double t2 = now_ms();
        h->stats[CTK_S_OPS] = (int64_t)ops.size();
        CTKCHK(upload_ops_dense(h, ops, ho, (int64_t)nd));
        h->ms[CTK_T_H2D] += now_ms() - t2;
        HT("ingest launched");
    } else {
        h->ms[CTK_T_D2H] += now_ms() - t0;
        h->stats[CTK_S_OPS] = 0;
        CTKCHK(upload_ops_dense(h, ops, nullptr, 0));                         // no ops: the launch still prepares ext / counters
    }
    (void)final_in_extent;                                                    // (k_extent computes the final id of every component)
    return CTK_OK;
}


// ------------------------------------------------------------------------------------------------
// numpy-order area sums of one merged component, from the tables and mask of the current shard (host resolver
// path, single GPU).  Only called for decisions flagged ambiguous (exact areas): a handful of
// small downloads, a scan of three mask planes on the host.
// ------------------------------------------------------------------------------------------------
namespace {
struct ExactFromDevice : CtkExactAreas {
    ctk_handle *h;
    std::vector<uint32_t> run_base, cprefix;
    struct Step {
        int64_t t = -1;
        std::vector<uint64_t> mask;
        std::vector<uint16_t> wstart;
        std::vector<uint32_t> rowstart, run_comp, mrep;
    };
    Step cache[3];
    bool ok = true;
    explicit ExactFromDevice(ctk_handle *h_) : h(h_) {}
    bool fetch(int64_t t, Step *&out)
    {
        Step &s = cache[t % 3];
        out = &s;
        if (s.t == t) return true;
        const size_t nw = (size_t)h->ny * h->W;
        if (run_base.empty()) {
            run_base.resize((size_t)h->T + 1); cprefix.resize((size_t)h->T + 1);
            if (hipMemcpy(run_base.data(), h->run_base.p, run_base.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (hipMemcpy(cprefix.data(), CPX(h), cprefix.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
        }
        const uint32_t nr = run_base[(size_t)t + 1] - run_base[(size_t)t], nc = cprefix[(size_t)t + 1] - cprefix[(size_t)t];
        s.mask.resize(nw); s.wstart.resize(nw); s.rowstart.resize((size_t)h->ny); s.run_comp.resize(nr); s.mrep.resize(nc);
        bool good = hipMemcpy(s.mask.data(), P<uint64_t>(h->mask) + (size_t)t * nw, nw * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(s.wstart.data(), P<uint16_t>(h->wstart) + (size_t)t * nw, nw * 2, hipMemcpyDeviceToHost) == hipSuccess &&
                    hipMemcpy(s.rowstart.data(), P<uint32_t>(h->rowstart) + (size_t)t * h->ny, (size_t)h->ny * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (good && nr) good = hipMemcpy(s.run_comp.data(), P<uint32_t>(h->run_comp) + run_base[(size_t)t], (size_t)nr * 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (good && nc) good = hipMemcpy(s.mrep.data(), P<uint32_t>(h->d_mrep) + cprefix[(size_t)t], (size_t)nc * 4, hipMemcpyDeviceToHost) == hipSuccess;
        s.t = good ? t : -1;
        return good;
    }
    // no-wrap component of pixel (y, x), or -1
    int64_t comp_at(const Step &s, int y, int x) const
    {
        const int W = h->W, w = x >> 6, b = x & 63;
        const uint64_t m = s.mask[(size_t)y * W + w];
        if (!((m >> b) & 1ull)) return -1;
        const uint64_t carry = w > 0 ? s.mask[(size_t)y * W + w - 1] >> 63 : 0ull;
        const uint64_t starts = m & ~((m << 1) | carry);
        const uint64_t below = b == 63 ? ~0ull : ((1ull << (b + 1)) - 1ull);
        const uint32_t k = s.rowstart[(size_t)y] + s.wstart[(size_t)y * W + w] + (uint32_t)__builtin_popcountll(starts & below) - 1u;
        return k < s.run_comp.size() ? (int64_t)s.run_comp[k] : -1;
    }
    int min_lsb() const override { return h->w_minlsb; }
    bool sums(int64_t t, uint32_t comp, const std::function<bool(uint32_t)> &kept_prev, double out[3]) override
    {
        if (!ok || t < 1 || t + 1 >= h->T || (int)h->c_w.size() != h->ny) return false;
        Step *cur, *prv, *nxt;
        if (!fetch(t, cur) || !fetch(t - 1, prv) || !fetch(t + 1, nxt)) { ok = false; return false; }
        const int ny = h->ny, nx = h->nx, W = h->W;
        std::vector<double> sa, sf, sb;                       // the gathered weights, raster order (contrack.py:717-719)
        for (int y = 0; y < ny; y++) {
            const double wy = (double)h->c_w[(size_t)y];
            for (int w = 0; w < W; w++) {
                uint64_t m = cur->mask[(size_t)y * W + w];
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const int x = w * 64 + b;
                    if (x >= nx) break;
                    const int64_t c = comp_at(*cur, y, x);
                    if (c < 0 || (size_t)c >= cur->mrep.size() || cur->mrep[(size_t)c] != comp) continue;
                    sa.push_back(wy);
                    if ((nxt->mask[(size_t)y * W + w] >> b) & 1ull) sf.push_back(wy);
                    const int64_t d = comp_at(*prv, y, x);
                    if (d >= 0 && kept_prev((uint32_t)d)) sb.push_back(wy);
                }
            }
        }
        out[0] = ctk_np_sum(sa.data(), sa.size());
        out[1] = ctk_np_sum(sf.data(), sf.size());
        out[2] = ctk_np_sum(sb.data(), sb.size());
        return true;
    }
};
}  // namespace

// the shard's own tables (single GPU)
static int device_resolve_local(ctk_handle *h, double overlap, int twosided)
{
    const size_t R = h->total_runs ? h->total_runs : 1;
    CTKCHK(ensure(h, h->comp_label, R * 4));
    CTKCHK(ensure(h, h->seam_rowoff, (size_t)(h->T + 1) * 4));
    if (h->T > 0 && (h->rowoff_T != h->T || h->rowoff_ny != h->ny || h->rowoff_p != h->seam_rowoff.p)) {      // t * ny: unchanged between calls on one grid
        k_iota_mul<<<(int)((h->T + 255) / 256), 256, 0, h->stream>>>(P<uint32_t>(h->seam_rowoff), (uint32_t)h->T, (uint32_t)h->ny);
        h->rowoff_T = h->T; h->rowoff_ny = h->ny; h->rowoff_p = h->seam_rowoff.p;
    }
    ResolveIn in;
    in.T = h->T; in.R = R;
    in.ncomp = P<uint32_t>(h->ncomp); in.cprefix = CPX(h); in.mrep = P<uint32_t>(h->d_mrep); in.comp_t = P<uint32_t>(h->d_comp_t);
    in.box = P<uint16_t>(h->d_box); in.area = P<int64_t>(h->d_area);
    in.pairs = P<CtkPair>(h->pairs); in.pair_cap = h->pair_cap; in.counters = P<uint32_t>(h->counters);
    in.pair_base = P<uint32_t>(h->pair_base); in.pair_cnt = P<uint32_t>(h->pair_cnt);
    in.seams = P<CtkSeam>(h->seams); in.seam_cnt = P<uint32_t>(h->seam_cnt); in.seam_off = P<uint32_t>(h->seam_rowoff);
    in.seam_cap = h->T * h->ny;
    in.comp_label = P<int32_t>(h->comp_label);
    int rv = device_resolve(h, in, overlap, twosided, true, true);
    if (rv == 0) { h->total_comps = (uint32_t)h->stats[CTK_S_COMPONENTS]; h->t_begin = 0; }
    return rv;
}

// the plan of the write launch over the whole shard (ctk_forms.h); the chunk-ordered copy of the run values
// (k_run_values -> the write kernel) is built for its chunks
static CtkWritePlan write_plan(const ctk_handle *h, const int32_t *flag_dev, int64_t nt)
{
    return ctk_write_plan(h->T, nt, h->ny, h->nx, h->W, ((uintptr_t)flag_dev & 15) == 0);
}
static int32_t *chunk_vals_for(ctk_handle *h, const int32_t *flag_dev, int *rows)
{
    const CtkWritePlan p = write_plan(h, flag_dev, h->T);
    *rows = p.rb;
    if (h->rle_out) return nullptr;                                   // (no write kernel in this call)
    if (!ctk_write_chunk_copy(p)) return nullptr;
    if (ensure(h, h->chunk_vals, (size_t)h->T * (size_t)p.nchunk * CTK_CV * 4) != CTK_OK) return nullptr;
    return P<int32_t>(h->chunk_vals);
}

// timesteps [t0, t0 + nt) of the shard into flag_dev (which starts at t0); nt < 0: the whole shard
static int launch_relabel(ctk_handle *h, int persistence, int32_t *flag_dev, bool with_fold, const int32_t *chunk_vals, int64_t t0, int64_t nt)
{
    if (h->rle_out) { h->stats[CTK_S_RELABEL_KERNEL] = -1; return CTK_OK; }      // the result leaves as run tables (deliver_runs expands them on the host)
    if (nt < 0) nt = h->T;
    const CtkWritePlan p = write_plan(h, flag_dev, nt);
    RelabelArgs a;
    a.mask = P<uint64_t>(h->mask) + t0 * h->ny * h->W; a.wstart = P<uint16_t>(h->wstart) + t0 * h->ny * h->W;
    a.rowstart = P<uint32_t>(h->rowstart) + t0 * h->ny; a.run_base = P<uint32_t>(h->run_base) + t0;
    a.run_val = P<int32_t>(h->run_val); a.ext = P<int32_t>(h->ext); a.n_labels = h->n_labels; a.persistence = persistence;
    a.t_begin = h->t_begin + t0;
    if (with_fold) a.fold = fold_args(h); else { a.fold.ops = nullptr; a.fold.first = nullptr; a.fold.next = nullptr; a.fold.nops = 0; }
    a.flag = flag_dev; a.counters = P<uint32_t>(h->counters);
    a.nrows = nt * h->ny; a.ny = h->ny; a.nx = h->nx; a.W = h->W;
    a.chunk_vals = chunk_vals && p.kernel != CTK_WR_GENERIC ? chunk_vals + t0 * p.nchunk * CTK_CV : nullptr;
    a.guard = h->guard_on ? P<uint32_t>(h->counters) : nullptr;
    a.plain_stores = 0; a.fast_zero = 0;                   // (kept in the kernel for its register allocation: ctk_kernels.hip, RelabelArgs)
    a.xcd_remap = h->xcd_rel_tuned >= 0 ? h->xcd_rel_tuned : 0;
    a.tab_batched = p.tab_batched;
    switch (p.kernel) {
    case CTK_WR_V5:
        if (h->rel_probe) k_relabel_probe<256><<<p.grid, 256, p.lds, h->stream>>>(a, p.rb, CTK_RV5, p.sub);      // (tune_relabel's launches: their own kernel name)
        else if (h->rel_variant == 1) k_relabel_v5_allsgpr<256><<<p.grid, 256, p.lds, h->stream>>>(a, p.rb, CTK_RV5, p.sub);
        else k_relabel_v5<256><<<p.grid, 256, p.lds, h->stream>>>(a, p.rb, CTK_RV5, p.sub);
        break;
    case CTK_WR_V4: k_relabel_v4<<<p.grid, 256, p.lds, h->stream>>>(a, p.rb, CTK_RVCAP); break;
    case CTK_WR_GENERIC: k_relabel<<<p.grid, 256, 0, h->stream>>>(a); break;
    default: break;                                        // (no timestep)
    }
    if (p.kernel != CTK_WR_NONE) { h->stats[CTK_S_RELABEL_KERNEL] = p.kernel; h->stats[CTK_S_RELABEL_SHAPE] |= p.shape; }
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

extern "C" int ctk_shard_write(ctk_handle *h, int persistence, int32_t *flag_dev, int64_t *n_alive_local, int *wrote_background)
{
    if (!h || (h->T > 0 && !flag_dev && !h->sio)) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state != ST_EXTENTS) return ctk_set_error(CTK_E_STATE, "ctk_shard_write needs ctk_shard_extents first");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (h->T > 0) {
        int cv_rows = 0;
        int32_t *cv = chunk_vals_for(h, flag_dev, &cv_rows);
        {
            Timer tm(h, CTK_K_RUNLABEL);
            const int rv_threads = ctk_runval_threads(CTK_PATH_STAGED, h->T, h->total_runs, h->small_threads[1]);
            k_run_values<<<(int)h->T, rv_threads, 0, s>>>(P<uint32_t>(h->run_base), P<uint32_t>(h->run_comp), CPX(h), P<int32_t>(h->comp_label),
                                                          P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->d_mrep), 0, 0, P<int32_t>(h->run_val),
                                                          P<uint32_t>(h->rowstart), h->ny, cv_rows, cv);
            HIPCHK(hipGetLastError());
            h->stats[CTK_S_RUNVAL_FORM] = ctk_runval_code(rv_threads, cv != nullptr);
        }
        {
            Timer tm(h, CTK_K_RELABEL);
            CTKCHK((flag_dev || !h->sio) ? launch_relabel(h, persistence, flag_dev, true, cv) : stream_out(h, persistence, cv));
        }
    }
    {
        Timer tm(h, CTK_K_COUNT);
        // (the counters were zeroed by k_fill_ext / k_ops_ingest; the last workgroup writes the results to pinned memory)
        const int form = ctk_count_form_staged(h->n_labels);
        if (form == CTK_COUNT_W1)
            k_count_alive_1<<<1, 1024, 0, s>>>(P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->counters), h->h_mail1 + 8, AsyncMail{});
        else
            k_count_alive<<<(int)std::min<int64_t>((h->n_labels + 255) / 256 + 1, 4096), 256, 0, s>>>(P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->counters),
                                                                                                    h->h_mail1 + 8, AsyncMail{});
        h->stats[CTK_S_COUNT_FORM] |= form;
        HIPCHK(hipGetLastError());
    }
    HT("tail launched");
    HIPCHK(hipStreamSynchronize(s));
    HT("sync3 done");
    h->last_alive = h->h_mail1[8];
    if (n_alive_local) *n_alive_local = h->last_alive;
    if (wrote_background) *wrote_background = h->h_mail1[9] ? 1 : 0;
    collect_event_times(h);
    h->state = ST_TABLES;           // extents may be recomputed (e.g. another persistence) from the same tables
    return CTK_OK;
}

extern "C" int ctk_shard_count_tracked(ctk_handle *h, int64_t *n_alive)
{
    if (!h || !n_alive) return ctk_set_error(CTK_E_INVALID, "null argument");
    *n_alive = h->last_alive;
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// fused one-call path: everything behind k_overlap without a host hand-off.  The resolver kernels, the device seam driver
// (ctk_seam_dev.hip), extents, run values, the write pass and the count are enqueued in one go; the counting kernel leaves a
// block of scalars in pinned memory; the host synchronises ONCE and validates: co-occurrence table intact, filter converged
// within the passes launched, no decision on a rounding boundary, seam clusters within the driver's tables.  Anything else:
// returns 1 and the caller repeats the resolution on the synchronous path (which handles all of those).
// ------------------------------------------------------------------------------------------------
static bool async_wanted(ctk_handle *h)
{
    if (h->use_async < 0) h->use_async = ctk_env().async ? 1 : 0;
    return h->use_async == 1 && h->in_one_call && !h->sio && h->T >= 1 && !(h->async_off_ny == h->ny && h->async_off_nx == h->nx);
}

static int resolve_async(ctk_handle *h, double overlap, int twosided, int persistence, int32_t *flag_dev, int64_t *n_tracked)
{
    hipStream_t s = h->stream;
    const int64_t T = h->T;
    const size_t R = h->total_runs ? h->total_runs : 1;
    CTKCHK(ensure(h, h->comp_label, R * 4));
    CTKCHK(ensure(h, h->seam_rowoff, (size_t)(T + 1) * 4));
    if (h->rowoff_T != T || h->rowoff_ny != h->ny || h->rowoff_p != h->seam_rowoff.p) {
        k_iota_mul<<<(int)((T + 255) / 256), 256, 0, s>>>(P<uint32_t>(h->seam_rowoff), (uint32_t)T, (uint32_t)h->ny);
        h->rowoff_T = T; h->rowoff_ny = h->ny; h->rowoff_p = h->seam_rowoff.p;
    }
    ResolveIn in;
    in.T = T; in.R = R;
    in.ncomp = P<uint32_t>(h->ncomp); in.cprefix = CPX(h); in.mrep = P<uint32_t>(h->d_mrep); in.comp_t = P<uint32_t>(h->d_comp_t);
    in.box = P<uint16_t>(h->d_box); in.area = P<int64_t>(h->d_area);
    in.pairs = P<CtkPair>(h->pairs); in.pair_cap = h->pair_cap; in.counters = P<uint32_t>(h->counters);
    in.pair_base = P<uint32_t>(h->pair_base); in.pair_cnt = P<uint32_t>(h->pair_cnt);
    in.seams = P<CtkSeam>(h->seams); in.seam_cnt = P<uint32_t>(h->seam_cnt); in.seam_off = P<uint32_t>(h->seam_rowoff);
    in.seam_cap = T * h->ny;
    in.comp_label = P<int32_t>(h->comp_label);
    ResolvePlan pl;
    CTKCHK(rs_prepare(h, in, overlap, twosided, pl));
    ResolveDev &r = pl.r;
    const int nsb = pl.nsb, gc = pl.gc, gp = pl.gp;
    // label-indexed tables of the device seam driver (ids <= components <= runs: only the entries of real ids are ever touched)
    CTKCHK(ensure(h, h->sd_parent, (R + 1) * 4)); CTKCHK(ensure(h, h->sd_tmin, (R + 1) * 4)); CTKCHK(ensure(h, h->sd_tmax, (R + 1) * 4));
    CTKCHK(ensure(h, h->sd_nops, (R + 1) * 4)); CTKCHK(ensure(h, h->sd_lbox, (R + 1) * 24));
    CTKCHK(ensure(h, h->sd_root, (size_t)std::max<int64_t>(T * h->ny, 1) * 4));
    // op slots: SD_OPS_OWN per label id (sized after the previous pass) + a shared tail for the clusters with more and the ids beyond
    // (before any pass has said how many ids this kind of slab has: one per 32 runs -- the bench slabs have one per 80-90)
    const size_t ids_guess = h->last_nlab ? (size_t)h->last_nlab + h->last_nlab / 4 : R / 32;
    const uint32_t own_ids = (uint32_t)std::min<size_t>(std::max<size_t>(ids_guess, 8192), R + 1);
    if (!h->last_nlab) h->op_cap_hint = std::max<uint32_t>(h->op_cap_hint, (uint32_t)std::min<size_t>(R / 256, 1u << 24));
    // (more op slots than int32 indices: not an error of the slab -- the synchronous resolver needs no such slots.  Round-5 advisor finding.)
    if ((uint64_t)own_ids * SD_OPS_OWN + h->op_cap_hint > 0x7ffffff0ull) { h->stats[CTK_S_HOST_REASON] |= 1024; return 1; }
    const uint32_t op_cap = own_ids * SD_OPS_OWN + h->op_cap_hint;
    CTKCHK(ensure(h, h->ops, (size_t)op_cap * (sizeof(CtkOp) + 4)));
    // ids <= components <= runs: R + 1 is the offset of the second half of ext (only the entries of real ids are ever touched)
    CTKCHK(ensure(h, h->ext, (R + 1) * 8));
    if (!h->h_amail) { HIPCHK(h->amail_pin.alloc(CTK_AM_WORDS * 4, hipHostMallocDefault)); h->h_amail = (uint32_t *)h->amail_pin.p; }
    memset(h->h_amail, 0, CTK_AM_WORDS * 4);
    h->n_labels = (int64_t)R; h->t_begin = 0;
    r.cl_parent = P<uint32_t>(h->sd_parent); r.cl_tmin = P<int32_t>(h->sd_tmin); r.cl_tmax = P<int32_t>(h->sd_tmax); r.cl_nops = P<uint32_t>(h->sd_nops);
    r.lbox = P<int32_t>(h->sd_lbox);
    CTKCHK(ensure(h, h->rv_lab_root, (R + 1) * 4));
    r.lab_root = P<int32_t>(h->rv_lab_root);
    r.ext = P<int32_t>(h->ext); r.ext_off = (int64_t)R + 1; r.counters_w = P<uint32_t>(h->counters);
    SeamDev sd;
    sd.dummy = nullptr; sd.own_base = 0; sd.cl_shared = nullptr;
    sd.cl_parent = r.cl_parent; sd.cl_tmin = r.cl_tmin; sd.cl_tmax = r.cl_tmax; sd.cl_nops = r.cl_nops; sd.lbox = r.lbox; sd.mark = P<uint8_t>(h->rv_mark);
    sd.rec_root = P<uint32_t>(h->sd_root); sd.recs = P<CtkCand>(h->rv_cand_scratch); sd.rec_cnt = P<uint32_t>(h->rv_cand_cnt);
    sd.t_nops = P<uint32_t>(h->rv_cand_off);              // ([T + 1], unused on this path otherwise)
    sd.ops = P<CtkOp>(h->ops); sd.op_next = (int32_t *)(P<CtkOp>(h->ops) + op_cap); sd.op_first = r.op_first;
    sd.op_count = P<uint32_t>(h->counters) + CTK_CNT_NOPS; sd.op_cap = op_cap; sd.own_ids = own_ids;
    sd.poison = P<uint32_t>(h->counters) + CTK_CNT_POISON; sd.ny = h->ny; sd.nx = h->nx; sd.T = T;
    sd.dbg = ctk_env().sd_dbg;
    sd.lab_cap = h->debug_sd_lab ? std::min(h->debug_sd_lab, SD_LAB) : SD_LAB; sd.ops_cap = h->debug_sd_ops ? std::min(h->debug_sd_ops, 64) : 64;
    h->d_op_next = sd.op_next;
    h->nops = 1;                                                  // (unknown here; nonzero = the folds look at the chains)
    const CtkFilterPlan fp = ctk_filter_plan_fused(T, h->async_passes, h->no_sys, h->n_cus, h->seg_cur != nullptr, h->fz_pslot, nsb);
    const int NP = fp.passes;
    if (fp.sys) { CTKCHK(ensure(h, h->rv_pstate, (size_t)(T + 1) * 4 * CTK_PSTATE_STRIDE)); r.pstate = P<uint32_t>(h->rv_pstate); }
    h->guard_on = true;
    struct GuardOff { ctk_handle *h; ~GuardOff() { h->guard_on = false; } } guard_off{h};
    {
        Timer tm(h, CTK_K_RESOLVE);
        if (!h->fz_init) {                                             // (else: k_compact_init and k_overlap did both)
            k_rs_init<<<gc, 256, 0, s>>>(r);
            k_rs_pairs<<<gp, 256, 0, s>>>(r);
        }
        if (fp.round.blk)                                              // (k_rs_pass_blk prepares its own timesteps and unites their pairs)
            launch_rs_pass_blk(h, fp.round.two_pc, fp.round.nb, r, 0, NP, in.pair_base, in.pair_cnt, r.pstate, 1, 1);
        else {
            k_rs_prep<<<gc, 256, 0, s>>>(r);
            for (int it = 0; it < NP; it++)
                launch_rs_pass(h, (int)(T - 2), r, it, in.pair_base, in.pair_cnt, P<uint8_t>(h->rv_tdirty));
        }
        switch (fp.unite) {
        case CTK_UNITE_SLOTS: k_rs_unite_slots<<<(int)std::min<int64_t>((T * h->fz_pslot + 255) / 256 + 1, 4096), 256, 0, s>>>(r, in.pair_cnt, h->fz_pslot); break;
        case CTK_UNITE_PAIRS: k_rs_unite<<<gp, 256, 0, s>>>(r); break;
        default: break;
        }
        h->stats[CTK_S_FILTER_FORMS] |= fp.bits;
        if (!fp.merged) r.lab_root = nullptr;
        k_rs_roots<<<nsb, 256, 0, s>>>(r, P<uint32_t>(h->rv_bsum));
        if (fp.merged) {
            // numbering of the components and marking of the seam rows in one launch (the marks derive the labels they need)
            const int nblk_max = (int)std::min<int64_t>(nsb, ((int64_t)h->total_runs + 255) / 256 + 1);      // (components <= runs)
            k_fz_rank_mark<<<std::max(nblk_max, (int)((T + 3) / 4)), 256, (size_t)nsb * 4, s>>>(r, sd, in.seams, in.seam_cnt, in.seam_off, P<int2>(h->rv_seam_res),
                                                                                               P<uint32_t>(h->rv_bsum), (uint32_t)nsb, P<uint32_t>(h->rv_boff) + nsb);
        } else {
            k_rs_rank<<<nsb, 256, 0, s>>>(r.isroot, in.cprefix + T, P<uint32_t>(h->rv_bsum), r.rank, P<uint32_t>(h->rv_boff) + nsb);
            k_rs_labels<<<gc, 256, 0, s>>>(r);
            k_fz_mark<<<(int)T, 64, 0, s>>>(r, sd, in.seams, in.seam_cnt, in.seam_off, P<int2>(h->rv_seam_res));
        }
        k_fz_groups<<<(int)((T + FZ_TW - 1) / FZ_TW), 64 * FZ_TW, 0, s>>>(r, sd, in.seams, in.seam_cnt, in.seam_off, P<int2>(h->rv_seam_res), 0);
        k_seam_driver<<<(int)std::min<int64_t>(T, 65536), 64, 0, s>>>(sd, 0);
        HIPCHK(hipGetLastError());
    }
    CTKCHK(launch_extents(h, true, true));
    h->state = ST_EXTENTS;
    int cv_rows = 0;
    int32_t *cv = chunk_vals_for(h, flag_dev, &cv_rows);
    {
        Timer tm(h, CTK_K_RUNLABEL);
        const int rv_threads = ctk_runval_threads(CTK_PATH_FUSED, T, h->total_runs, h->small_threads[1]);
        h->stats[CTK_S_RUNVAL_FORM] = ctk_runval_code(rv_threads, cv != nullptr);
        k_run_values<<<(int)T, rv_threads, 0, s>>>(P<uint32_t>(h->run_base), P<uint32_t>(h->run_comp), CPX(h), P<int32_t>(h->comp_label),
                                            P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->d_mrep), 0, 0, P<int32_t>(h->run_val),
                                            P<uint32_t>(h->rowstart), h->ny, cv_rows, cv, P<uint32_t>(h->counters),
                                            P<uint32_t>(h->rv_boff) + nsb, P<uint32_t>(h->seam_off) /* t_alive: [T + 1], unused on this path otherwise */);
        HIPCHK(hipGetLastError());
    }
    {
        Timer tm(h, CTK_K_RELABEL);
        CTKCHK(launch_relabel(h, persistence, flag_dev, true, cv));
    }
    AsyncMail am;
    am.scal = h->h_amail; am.nlab_ptr = P<uint32_t>(h->rv_boff) + nsb; am.nc_ptr = in.cprefix + T;
    am.stamp = (uint32_t)(h->pass_no & 0x7fffffffu) | 0x80000000u;
    am.changed = r.changed; am.ambig = r.ambig; am.rec_cnt = P<uint32_t>(h->rv_cand_cnt); am.t_nops = sd.t_nops; am.pair_cnt = in.pair_cnt; am.t_alive = P<uint32_t>(h->seam_off); am.T = T; am.passes = NP;
    {
        Timer tm(h, CTK_K_COUNT);
        const int form = ctk_count_form_fused(h->last_nlab, NP);
        switch (form) {
        case CTK_COUNT_F: k_count_alive_f<<<1, 1024, 0, s>>>(P<uint32_t>(h->counters), h->h_mail1 + 8, am); break;
        case CTK_COUNT_1: k_count_alive_1<<<1, 1024, 0, s>>>(P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->counters), h->h_mail1 + 8, am); break;
        default: k_count_alive<<<1024, 256, 0, s>>>(P<int32_t>(h->ext), h->n_labels, persistence, P<uint32_t>(h->counters), h->h_mail1 + 8, am); break;
        }
        h->stats[CTK_S_COUNT_FORM] |= form;
        HIPCHK(hipGetLastError());
    }
    HT("fused pass launched");
    {
        // The last kernel of the pass writes the block of scalars into pinned memory and its stamp last: the host spins on the
        // stamp instead of waiting for the stream's completion signal (which arrives several microseconds later); every kernel
        // of the pass has finished when the stamp is there -- they run in stream order.  The health check is rare (a query on a
        // busy stream enqueues a marker).
        const bool poll = h->timing < 2;                  // (level-2 timing has an event BEHIND the last kernel: wait for the stream)
        volatile uint32_t *vm = h->h_amail;
        bool done = false;
        if (poll)
            for (uint64_t spins = 1;; spins++) {
                if (vm[CTK_AM_DONE] == am.stamp) { done = true; break; }
                if ((spins & 0xfffff) == 0) {
                    const hipError_t q = hipStreamQuery(s);
                    if (q == hipSuccess) break;
                    if (q != hipErrorNotReady) return ctk_set_error(CTK_E_NODEVICE, "fused pass: %s", hipGetErrorString(q));
                }
            }
        if (!done) HIPCHK(hipStreamSynchronize(s));
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
    }
    HT("fused pass done");
    const uint32_t *m = h->h_amail;
    if (m[CTK_AM_DONE] != am.stamp) return ctk_set_error(CTK_E_INTERNAL, "fused pass: the device did not report");
    h->state = ST_TABLES;
    const uint32_t *cnt = m + CTK_AM_COUNTERS;
    // ---- validation: anything the host would have seen at one of its (removed) hand-offs -----------------------------------
    if ((cnt[CTK_CNT_OVERFLOW] & CTK_OVF_PAIRS) || (uint64_t)cnt[CTK_CNT_PAIRS] + cnt[CTK_CNT_UPAIRS] > in.pair_cap) { h->stats[CTK_S_HOST_REASON] |= 32; return 1; }      // (the synchronous path regrows the table)
    const int64_t npairs_grouped = h->fz_pslot ? (int64_t)m[CTK_AM_NPAIRS] : (int64_t)cnt[CTK_CNT_PAIRS];
    if (NP > 0 && m[CTK_AM_CONV] == 0) { h->async_passes = std::min(CTK_MAX_JACOBI, NP * 2); h->stats[CTK_S_HOST_REASON] |= 64; return 1; }          // longer removal cascade than launched for
    if (m[CTK_AM_AMBIG]) { h->stats[CTK_S_HOST_REASON] |= 128; return 1; }                                                                               // decisions on rounding boundaries
    if (ctk_env().sd_dbg) fprintf(stderr, "SDDBG max row steps %u, max fold iterations %u, max process time %.2f us, max cluster time %.2f us, fold cycles (clock64) %u\n", cnt[10], cnt[11], cnt[12] * 0.01, cnt[13] * 0.01, cnt[14]);
    const uint32_t poison = cnt[CTK_CNT_POISON];
    if (poison) {
        // an inter-workgroup wait of the systolic filter pass gave up (a workgroup waited for was not running): this handle
        // launches one kernel per filter pass from now on -- no waits between workgroups at all
        if (poison & CTK_POISON_SPIN) { h->no_sys = true; h->stats[CTK_S_HOST_REASON] |= 8; }
        if (poison & CTK_POISON_OPCAP) h->stats[CTK_S_HOST_REASON] |= 256;
        if (poison & CTK_POISON_CLUSTER) h->stats[CTK_S_HOST_REASON] |= 512;
        if (poison & CTK_POISON_OPCAP) h->op_cap_hint = std::max(h->op_cap_hint * 2, cnt[CTK_CNT_NOPS] + cnt[CTK_CNT_NOPS] / 2 + 1024);
        if (m[CTK_AM_NLAB] && m[CTK_AM_NLAB] <= 0x7ffffffeu) h->last_nlab = m[CTK_AM_NLAB];      // (the ids were numbered in front of the seam driver: the next pass sizes its own slots by them)
        if (poison & CTK_POISON_CLUSTER) { h->async_off_ny = h->ny; h->async_off_nx = h->nx; }                 // this kind of slab: host driver from now on
        return 1;
    }
    const int64_t nlab = m[CTK_AM_NLAB];
    if (nlab > 0x7ffffffell) return ctk_set_error(CTK_E_RANGE, "%lld ids do not fit the int32 flag variable", (long long)nlab);
    if (NP > 0) h->async_passes = std::max<int>(CTK_JACOBI_ROUND, (int)m[CTK_AM_CONV] + 2);
    h->op_cap_hint = std::max<uint32_t>(h->op_cap_hint, cnt[CTK_CNT_NOPS] * 2 + 1024);
    h->nops = (int32_t)cnt[CTK_CNT_NOPS];
    h->last_nlab = nlab;
    h->total_comps = m[CTK_AM_NC];
    h->stats[CTK_S_COMPONENTS] = m[CTK_AM_NC]; h->stats[CTK_S_PAIRS] = npairs_grouped + cnt[CTK_CNT_UPAIRS];
    h->stats[CTK_S_UPAIRS] = cnt[CTK_CNT_UPAIRS]; h->stats[CTK_S_SEAM_ROWS] = m[CTK_AM_NCAND]; h->stats[CTK_S_LABELS] = nlab;
    h->stats[CTK_S_OPS] = cnt[CTK_CNT_NOPS]; h->stats[CTK_S_FILTER_PASSES] = NP > 0 ? m[CTK_AM_CONV] : 0; h->stats[CTK_S_FILTER_ROUNDS] = NP > 0 ? 1 : 0;
    h->stats[CTK_S_AMBIGUOUS] = 0; h->stats[CTK_S_FUSED] = 1;
    h->last_alive = h->h_mail1[8];
    if (n_tracked) *n_tracked = (int64_t)h->h_mail1[8] + (h->h_mail1[9] ? 1 : 0) - 1;       // len(np.unique(flag)) - 1, contrack.py:793
    collect_event_times(h);
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// whole path, one GPU
// ------------------------------------------------------------------------------------------------
struct ctk_comm;
static int track_sharded_impl(ctk_handle *h, ctk_comm *c, const void *anom_dev, bool f64, int64_t T, int64_t t_begin, int64_t T_total, int ny, int nx,
                              const double *thr, int cmp_op, const float *wrow, double overlap, int persistence, int twosided, int32_t *flag_dev,
                              int64_t *n_tracked);                                                      // ctk_sharded.hip

// How the chunks of the write kernel are dealt to the XCDs decides a few per cent of its time, and which way is best depends on the
// grid and on where the caller's `flag` lies (2707 x 181 x 360: one contiguous eighth per XCD -5 ... -8 % against launch order,
// 480 x 721 x 1440: launch order best by 2-5 %; NOTES round 4).  After the first pass on a new shape / output buffer the kernel is
// timed in the three ways on the finished tables (it writes the same flags again) and the fastest kept.  ~1 ms, once.
static void tune_relabel(ctk_handle *h, int persistence, int32_t *flag_dev)
{
    if (!ctk_env().mask_tune || h->sio || h->rle_out || !flag_dev || h->state != ST_TABLES) return;
    // once per SHAPE (round 4 also keyed on the output pointer: a caller that alternates output buffers re-tuned on every call --
    // advisor finding); slabs beyond 8 GB keep the launch order (nine extra passes of the write kernel would cost ~100 ms at
    // 14 600 x 721 x 1440, where launch order measured best anyway)
    if (h->rel_tuned_T == h->T && h->rel_tuned_ny == h->ny && h->rel_tuned_nx == h->nx) return;
    if ((size_t)h->T * h->ny * h->nx * 4 < ((size_t)128 << 20)) return;
    // (like the mask check: at the SECOND pass on a shape, so that a one-shot call does not pay nine extra launches)
    if (!(h->rel_seen_T == h->T && h->rel_seen_ny == h->ny && h->rel_seen_nx == h->nx)) { h->rel_seen_T = h->T; h->rel_seen_ny = h->ny; h->rel_seen_nx = h->nx; return; }
    h->rel_tuned_T = h->T; h->rel_tuned_ny = h->ny; h->rel_tuned_nx = h->nx; h->rel_tuned_flag = flag_dev;
    // (beyond 8 GB nothing is timed: by the shape -- one contiguous eighth per XCD won on every narrow grid it was timed on (2707 x 181 x 360:
    // -5 ... -8 %; 438 000 x 192 x 288, round 6: 18.75 -> 18.07 ms), the launch order on 1440-wide ones)
    if ((size_t)h->T * h->ny * h->nx * 4 > ((size_t)8 << 30)) { h->xcd_rel_tuned = h->nx < 1024 ? 1 : -1; return; }
    Event e0, e1;
    if (e0.create() != hipSuccess || e1.create() != hipSuccess) return;
    int rows = 0;
    const int32_t *cv = chunk_vals_for(h, flag_dev, &rows);
    const int modes[3] = {0, 1, 16};
    h->rel_probe = true;
    struct ProbeOff { ctk_handle *h; ~ProbeOff() { h->rel_probe = false; } } probe_off{h};
    double best = 1e30;
    int best_mode = -1;
    bool ok = true;
    for (int m = 0; m < 3 && ok; m++) {
        h->xcd_rel_tuned = modes[m];
        ok = launch_relabel(h, persistence, flag_dev, true, cv) == CTK_OK && hipEventRecord(e0, h->stream) == hipSuccess;
        ok = ok && launch_relabel(h, persistence, flag_dev, true, cv) == CTK_OK && launch_relabel(h, persistence, flag_dev, true, cv) == CTK_OK;
        ok = ok && hipEventRecord(e1, h->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
        float f = 0.f;
        ok = ok && hipEventElapsedTime(&f, e0, e1) == hipSuccess;
        if (ok && f < best) { best = f; best_mode = modes[m]; }
    }
    h->xcd_rel_tuned = ok ? best_mode : -1;
    if (ctk_env().hosttrace) fprintf(stderr, "write kernel: chunk -> XCD mode %d, %.2f TB/s\n", h->xcd_rel_tuned, (double)h->T * h->ny * h->nx * 4 / 1e9 / (0.5 * best));
    (void)hipStreamSynchronize(h->stream);
}

static int track_dev_impl(ctk_handle *h, const void *anom_dev, bool f64, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                          const float *wrow, double overlap, int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    const double t0 = now_ms();
    HT0();
    h->in_one_call = true;
    struct OneCall { ctk_handle *h; ~OneCall() { h->in_one_call = false; h->seg_cur = nullptr; h->seg_cur_host = nullptr; } } one_call{h};
    if (!h->seg_starts.empty()) {
        HIPCHK(hipSetDevice(h->device));
        CTKCHK(segment_table(h, T));
    } else if (!h->seg_call.empty()) {                         // the starts a streaming entry was given (checked there against this T)
        HIPCHK(hipSetDevice(h->device));
        CTKCHK(segment_table_call(h, h->seg_call, T, 0, T));
    }
    CTKCHK(shard_label2d_impl(h, anom_dev, f64, T, ny, nx, thr, cmp_op, wrow, 0));
    HT("label2d stage done");
    CTKCHK(ctk_shard_overlap(h));
    HT("overlap launched");
    if (h->use_device_resolve && async_wanted(h) && T > 0) {
        const int ra = resolve_async(h, overlap, twosided, persistence, flag_dev, n_tracked);
        if (ra <= 0) { if (ra == 0) tune_relabel(h, persistence, flag_dev); h->ms[CTK_T_TOTAL] += now_ms() - t0; return ra; }
        h->stats[CTK_S_FUSED] = 0;                           // fell off the fused path: the synchronous one resolves the same tables
        if (h->fz_pslot) {
            // ... which wants the co-occurrence records in one contiguous range: the histogram again, ranges from the counter
            const uint32_t ovf_keep = h->h_amail[CTK_AM_COUNTERS + CTK_CNT_OVERFLOW] & ~CTK_OVF_PAIRS;
            HIPCHK(hipMemsetAsync(P<uint32_t>(h->counters) + CTK_CNT_PAIRS, 0, 4, h->stream));
            HIPCHK(hipMemsetAsync(P<uint32_t>(h->counters) + CTK_CNT_UPAIRS, 0, 4, h->stream));
            HIPCHK(hipMemcpyAsync(P<uint32_t>(h->counters) + CTK_CNT_OVERFLOW, &ovf_keep, 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            h->fz_init = false;
            CTKCHK(launch_overlap(h));
        }
    }
    int rv = h->use_device_resolve ? device_resolve_local(h, overlap, twosided) : 1;
    if (rv < 0) return rv;
    if (rv == 1 && h->use_device_resolve && h->stats[CTK_S_AMBIGUOUS] && !(h->stats[CTK_S_HOST_REASON] & 3)) {
        // Decisions on rounded area sums within rounding distance of the threshold (exact ties on components with pole-row
        // pixels): the time-shard path re-evaluates exactly those on the device with numpy-order sums (its "exact fix-up").
        // A shard that is the whole slab, a communicator of one rank: no exchange happens, the result is the one-call result.
        h->stats[CTK_S_HOST_REASON] = 4;
        ctk_comm self;
        self.rank = 0; self.world = 1; self.kind = 0; self.device = h->device; self.stream = h->stream;
        const int rc = track_sharded_impl(h, &self, anom_dev, f64, T, 0, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag_dev, n_tracked);
        h->stats[CTK_S_HOST_REASON] = 4;
        h->ms[CTK_T_TOTAL] = now_ms() - t0;
        return rc;
    }
    if (rv == 0) {
        CTKCHK(launch_extents(h, true, true));                  // + the final id of every component (k_rs_final's work)
        h->state = ST_EXTENTS;
    } else {
        // host path: download the tables, resolve with the GPU-free reference implementation, upload
        h->stats[CTK_S_HOST_PATH] = 1;
        const void *blob = nullptr;
        size_t nbytes = 0;
        CTKCHK(ctk_shard_tables(h, &blob, &nbytes));
        const double t1 = now_ms();
        ctk_result *res = nullptr;
        ExactFromDevice exact(h);                                 // numpy-order sums for decisions flagged ambiguous
        CTKCHK(ctk_resolve_ex(&blob, &nbytes, 1, overlap, twosided, &exact, &res, h->seg_cur ? h->seg_cur_host : nullptr));
        h->ms[CTK_T_HOST_RESOLVE] += now_ms() - t1;
        h->stats[CTK_S_AMBIGUOUS] = res->n_ambiguous;
        h->stats[CTK_S_EXACT_FIXUPS] = res->n_exact;
        h->stats[CTK_S_OPS] = res->nops;                          // (the host resolver's own seam merge: ctk_resolve.cpp, step 4b)
        int rc = ctk_shard_extents(h, res, 0, 0, nullptr, nullptr);
        ctk_result_free(res);
        CTKCHK(rc);
    }
    int64_t alive = 0;
    int wrote0 = 0;
    CTKCHK(ctk_shard_write(h, persistence, flag_dev, &alive, &wrote0));
    if (n_tracked) *n_tracked = alive + (wrote0 ? 1 : 0) - 1;       // len(np.unique(flag)) - 1, contrack.py:793
    tune_relabel(h, persistence, flag_dev);
    h->ms[CTK_T_TOTAL] += now_ms() - t0;
    return CTK_OK;
}


// ------------------------------------------------------------------------------------------------
// host-array entries (what the drop-in class calls): H2D, the device path, D2H.
// Measured on the MI355X box (2 x EPYC 9575F, PCIe Gen5; tools/e2e_probe.py, 705.6 MB each way):
//   * H2D: a plain hipMemcpy of the caller's pageable slab runs at 56 GB/s (12.6 ms) -- nothing to add.
//   * D2H: the result usually lands in an array fresh from np.empty, i.e. in pages that do not exist yet; a plain hipMemcpy
//     then crawls at 25 GB/s behind first-touch page faults taken by one thread (28 ms).  Eight threads, each draining its
//     own double-buffered pinned bounce buffer with memcpy, take those faults in parallel: 14.9 ms.  The bounce buffers are
//     hipHostMallocNonCoherent: the CPU reads the default, fine-grained pinned memory uncached (that kept the first version
//     of this scheme at 22 GB/s in both directions whatever the number of threads).
//   Populating the pages from helper threads while the input travels (MADV_POPULATE_WRITE) was tried and is worse: the
//   faults contend with the page pinning of the concurrent H2D copy (H2D 12.6 -> 25-37 ms).
// ------------------------------------------------------------------------------------------------
static bool host_is_pinned(const void *p, size_t n);
namespace {
// to_device: host -> device, else device -> host.  Lane i moves the chunks i, i + kLanes, ...
// false = not done: the caller issues a plain hipMemcpy (small copies; pinned / registered host memory, which takes ONE DMA at PCIe
// rate -- ctk_host_alloc, ctk_host_register: the bounce threads exist for the page faults of fresh pageable arrays)
bool bounce_copy(BouncePool &pool, int device, void *dev, void *host, size_t bytes, bool to_device)
{
    if (bytes < 4 * kBounce || host_is_pinned(host, bytes) || !pool.init()) return false;
    const size_t nchunk = (bytes + kBounce - 1) / kBounce;
    std::atomic<bool> ok(true);
    auto work = [&](int li) {
        if (hipSetDevice(device) != hipSuccess) { ok = false; return; }
        BounceLane &L = pool.lane[li];
        int b = 0;
        size_t pending[2] = {(size_t)-1, (size_t)-1};
        auto drain = [&](int bb) {                                               // device -> host: finish the copy out of buffer bb
            if (pending[bb] == (size_t)-1) return;
            if (hipEventSynchronize(L.ev[bb]) != hipSuccess) ok = false;
            if (!to_device) {
                const size_t off = pending[bb] * kBounce, len = std::min(kBounce, bytes - off);
                memcpy((char *)host + off, L.pin[bb].p, len);
            }
            pending[bb] = (size_t)-1;
        };
        for (size_t c = (size_t)li; c < nchunk && ok; c += kLanes, b ^= 1) {
            drain(b);                                                             // the buffer is free again
            const size_t off = c * kBounce, len = std::min(kBounce, bytes - off);
            if (to_device) {
                memcpy(L.pin[b].p, (const char *)host + off, len);
                if (hipMemcpyAsync((char *)dev + off, L.pin[b].p, len, hipMemcpyHostToDevice, L.st) != hipSuccess) ok = false;
            } else {
                if (hipMemcpyAsync(L.pin[b].p, (const char *)dev + off, len, hipMemcpyDeviceToHost, L.st) != hipSuccess) ok = false;
            }
            if (hipEventRecord(L.ev[b], L.st) != hipSuccess) ok = false;
            pending[b] = c;
        }
        drain(0); drain(1);
    };
    std::thread th[kLanes];
    for (int i = 0; i < kLanes; i++) th[i] = std::thread(work, i);
    for (int i = 0; i < kLanes; i++) th[i].join();
    return ok;
}
}  // namespace

// a finished result from device memory into the caller's host array: the bounce lanes; plain hipMemcpy for small results / if the lanes fail
static int download(ctk_handle *h, const void *dev, void *host, size_t bytes)
{
    if (!h->bounce) h->bounce.reset(new (std::nothrow) BouncePool());
    if (!h->bounce || !bounce_copy(*h->bounce, h->device, const_cast<void *>(dev), host, bytes, false))
        HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// The result of a host-array entry over PCIe.  The device pass ends with the value of every foreground RUN (k_run_values) and the
// bit mask the runs were cut from: 30 MB at 2707 x 181 x 360, where the dense int32 slab k_relabel would write is 706 MB -- 12.4 ms
// of a 25.8 ms call at PCIe rate.  So the host entries do not launch the write kernel at all: the tables of a block of timesteps
// (mask words, first run of every row, run values) travel into a lane's pinned buffer and the lane writes the block of the
// caller's array from them -- zeros, then each run's id over its pixels.  No labelling happens here: every value was computed on the
// device, this is the decoder of a run-length transfer format.  Runs of "complex" components (negative value: their pixels are
// folded one by one through the seam operations, fold_pixel) are left to the device: the blocks that hold one are written by
// k_relabel into a block-sized device buffer afterwards and copied densely.
//   device-resident entries (ctk_track_*_dev, the time-shard path, the streaming entries): unchanged, k_relabel_v5 writes `flag`.
//   CTK_RLE_OUT=0 / ctk_set_result_transfer(h, 0): the dense copy for the host entries too.
// ------------------------------------------------------------------------------------------------
namespace {
// A row of the result leaves the core through non-temporal stores: the zeros of an empty row straight from a register, a row with
// runs from a scratch row in L1.  Plain stores (memset + fills) into the array take a read-for-ownership of every line first and
// hold a core at ~15 GB/s: 5 ms for the 706 MB of the 1 degree slab on sixteen lanes; only the partial lines at both ends of a
// row are written that way.
inline void stream_row(int32_t *dst, const int32_t *src /* nullptr: zeros */, size_t n)
{
    unsigned char *d = reinterpret_cast<unsigned char *>(dst);
    const unsigned char *s = reinterpret_cast<const unsigned char *>(src);
    size_t bytes = n * 4;
    size_t head = (64 - ((uintptr_t)d & 63)) & 63;
    if (head > bytes) head = bytes;
    if (head) { if (s) { memcpy(d, s, head); s += head; } else memset(d, 0, head); d += head; bytes -= head; }
    const size_t body = bytes & ~(size_t)63;
    if (s) {
        for (size_t i = 0; i < body; i += 64) {
            const __m128i a0 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i)), a1 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i + 16));
            const __m128i a2 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i + 32)), a3 = _mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i + 48));
            _mm_stream_si128(reinterpret_cast<__m128i *>(d + i), a0); _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 16), a1);
            _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 32), a2); _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 48), a3);
        }
        if (bytes > body) memcpy(d + body, s + body, bytes - body);
    } else {
        const __m128i z = _mm_setzero_si128();
        for (size_t i = 0; i < body; i += 64) {
            _mm_stream_si128(reinterpret_cast<__m128i *>(d + i), z); _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 16), z);
            _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 32), z); _mm_stream_si128(reinterpret_cast<__m128i *>(d + i + 48), z);
        }
        if (bytes > body) memset(d + body, 0, bytes - body);
    }
}

// one block: tables in `buf` ([mask nt*ny*W u64][rowstart nt*ny u32, padded to 8][run values nr i32]) -> flag rows
void rle_expand_block(const unsigned char *buf, const RleBlock &c, const uint32_t *run_base, int ny, int nx, int W, int32_t *flag, int32_t *scratch /* [W * 64] */,
                      bool &zero, bool &complex_run)
{
    const size_t nrow = (size_t)c.nt * ny;
    const uint64_t *mask = reinterpret_cast<const uint64_t *>(buf);
    const uint32_t *rowstart = reinterpret_cast<const uint32_t *>(buf + nrow * W * 8);
    const int32_t *rv = reinterpret_cast<const int32_t *>(buf + nrow * W * 8 + ((nrow * 4 + 7) & ~(size_t)7));
    const int tail = nx - (W - 1) * 64;
    const uint64_t last_valid = tail < 64 ? ((1ull << tail) - 1ull) : ~0ull;
    bool z = false, cx = false;
    for (int64_t t = 0; t < c.nt; t++) {
        const int32_t *rvt = rv + (run_base[c.t0 + t] - c.r0);
        for (int y = 0; y < ny; y++) {
            const size_t row = (size_t)t * ny + y;
            int32_t *out = flag + ((size_t)(c.t0 + t) * ny + y) * (size_t)nx;
            const uint64_t *mw = mask + row * W;
            uint64_t any = 0;
            for (int w = 0; w < W; w++) any |= mw[w];
            if (!any) { stream_row(out, nullptr, (size_t)nx); z = true; continue; }
            memset(scratch, 0, (size_t)nx * 4);
            uint32_t k = rowstart[row];
            uint64_t prev = 0;
            int32_t cur = 0;
            int fg = 0;
            for (int w = 0; w < W; w++) {
                uint64_t m = mw[w];
                if (w == W - 1) m &= last_valid;
                if (!m) { prev = 0; continue; }
                fg += __builtin_popcountll(m);
                uint64_t mm = m;
                int32_t *ow = scratch + (size_t)w * 64;
                while (mm) {
                    const int b = __builtin_ctzll(mm);
                    const uint64_t sh = mm >> b;
                    const int n = (~sh == 0ull) ? 64 : __builtin_ctzll(~sh);
                    if (!(b == 0 && prev)) cur = rvt[k++];                      // a new run (else: the run continues from the word before)
                    if (cur > 0) { for (int q = b; q < b + n; q++) ow[q] = cur; }
                    else if (cur == 0) z = true;                               // filtered out (persistence): the zeros are there
                    else cx = true;
                    mm = (n >= 64 - b) ? 0ull : (mm & ~(((1ull << n) - 1ull) << b));
                }
                prev = m >> 63;
            }
            if (fg != nx) z = true;
            stream_row(out, scratch, (size_t)nx);
        }
    }
    _mm_sfence();
    if (z) zero = true;
    if (cx) complex_run = true;
}
}  // namespace

// blocks of timesteps whose tables fit a lane buffer of `cap` bytes (a single timestep always does: rle_need)
static size_t rle_per_t(int ny, int W) { return (size_t)ny * W * 8 + (size_t)ny * 4 + 16; }
static size_t rle_need(const uint32_t *run_base, int64_t T, int ny, int W)
{
    uint32_t mx = 0;
    for (int64_t t = 0; t < T; t++) mx = std::max(mx, run_base[t + 1] - run_base[t]);
    return rle_per_t(ny, W) + (size_t)mx * 4;
}
static bool rle_blocks(const uint32_t *run_base, int64_t T, int ny, int W, size_t cap, std::vector<RleBlock> &out)
{
    const size_t per_t = rle_per_t(ny, W);
    const int per_lane = 8;
    const int64_t want = std::max<int64_t>(1, (T + kRleLanes * per_lane - 1) / (kRleLanes * per_lane));        // ~8 blocks per lane (probe: tools/exp/rle_probe.py)
    out.clear();
    for (int64_t t0 = 0; t0 < T;) {
        int64_t nt = 0;
        while (t0 + nt < T && nt < want) {
            const size_t bytes = (size_t)(nt + 1) * per_t + (size_t)(run_base[t0 + nt + 1] - run_base[t0]) * 4;
            if (bytes > cap) break;
            nt++;
        }
        if (nt == 0) return false;
        out.push_back(RleBlock{t0, nt, run_base[t0], run_base[t0 + nt] - run_base[t0]});
        t0 += nt;
    }
    return true;
}

// The decoder alone, on host tables (no device involved): what the CPU tests hold against a dense expansion in numpy.
extern "C" int ctk_expand_runs_host(const uint64_t *mask, const uint32_t *rowstart, const uint32_t *run_base, const int32_t *run_val, int64_t T, int ny, int nx,
                                    int32_t *flag, int *wrote_background, int *complex_runs)
{
    if (T < 0 || ny < 1 || nx < 1 || (T > 0 && (!mask || !rowstart || !run_base || !flag))) return ctk_set_error(CTK_E_INVALID, "ctk_expand_runs_host: bad argument");
    const int W = (nx + 63) / 64;
    const size_t nrow = (size_t)ny;
    std::vector<unsigned char> buf;
    std::vector<int32_t> scratch((size_t)W * 64 + 16);
    bool z = false, cx = false;
    for (int64_t t = 0; t < T; t++) {
        const uint32_t r0 = run_base[t], nr = run_base[t + 1] - r0;
        if (nr && !run_val) return ctk_set_error(CTK_E_INVALID, "ctk_expand_runs_host: runs without values");
        const size_t off_rs = nrow * W * 8, off_rv = off_rs + ((nrow * 4 + 7) & ~(size_t)7);
        buf.resize(off_rv + (size_t)nr * 4 + 8);
        memcpy(buf.data(), mask + (size_t)t * nrow * W, nrow * W * 8);
        memcpy(buf.data() + off_rs, rowstart + (size_t)t * nrow, nrow * 4);
        if (nr) memcpy(buf.data() + off_rv, run_val + r0, (size_t)nr * 4);
        rle_expand_block(buf.data(), RleBlock{t, 1, r0, nr}, run_base, ny, nx, W, flag, scratch.data(), z, cx);
    }
    if (wrote_background) *wrote_background = z ? 1 : 0;
    if (complex_runs) *complex_runs = cx ? 1 : 0;
    return CTK_OK;
}

// The pass is over (tables in ST_TABLES state, nothing running on the handle's stream): expand the result into `flag`.
#define CTK_RLE_UNAVAILABLE 2          // deliver_runs: the run transfer could not be set up / carried out; the pass itself is fine
static int deliver_runs(ctk_handle *h, int persistence, int32_t *flag, int *wrote_background)
{
    const int64_t T = h->T;
    const int ny = h->ny, nx = h->nx, W = h->W;
    const double tr_begin = now_ms();
    std::vector<uint32_t> &rb = h->rle_run_base;
    rb.resize((size_t)T + 1);
    HIPCHK(hipMemcpy(rb.data(), h->run_base.p, (size_t)(T + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<RleBlock> &blocks = h->rle_blocks;
    if (!h->rle) h->rle.reset(new (std::nothrow) RlePool());
    // What can go wrong HERE leaves the device pass intact: the caller repeats it with the dense result (CTK_RLE_UNAVAILABLE; until round 5
    // a shortage of pinned memory failed the whole call -- advisor finding).  rle_mode 2: a test hook that takes this exit.
    if (h->rle_mode == 2) { (void)ctk_set_error(CTK_E_NOMEM, "result transfer: made unavailable (test hook)"); return CTK_RLE_UNAVAILABLE; }
    if (!h->rle || !h->rle->init(rle_need(rb.data(), T, ny, W))) { (void)ctk_set_error(CTK_E_NOMEM, "result transfer: no pinned memory for the lane buffers"); return CTK_RLE_UNAVAILABLE; }
    if (!rle_blocks(rb.data(), T, ny, W, h->rle->cap, blocks)) { (void)ctk_set_error(CTK_E_INTERNAL, "result transfer: a timestep's tables do not fit a lane buffer"); return CTK_RLE_UNAVAILABLE; }
    const size_t nb = blocks.size();
    const int lanes = (int)std::min<size_t>(kRleLanes, nb);
    std::atomic<int64_t> wait_us(0), exp_us(0);
    std::atomic<bool> ok(true), zero(false);
    std::vector<unsigned char> cx(nb, 0);                                          // blocks that hold a run of a complex component
    const uint64_t *d_mask = P<uint64_t>(h->mask);
    const uint32_t *d_rowstart = P<uint32_t>(h->rowstart);
    const int32_t *d_rv = P<int32_t>(h->run_val);
    auto work = [&](int li) {
        if (hipSetDevice(h->device) != hipSuccess) { ok = false; return; }
        BounceLane &L = h->rle->lane[li];
        auto fetch = [&](size_t bi, int b) {
            const RleBlock &c = blocks[bi];
            const size_t nrow = (size_t)c.nt * ny;
            unsigned char *dst = (unsigned char *)L.pin[b].p;
            bool good = hipMemcpyAsync(dst, d_mask + (size_t)c.t0 * ny * W, nrow * W * 8, hipMemcpyDeviceToHost, L.st) == hipSuccess;
            good = good && hipMemcpyAsync(dst + nrow * W * 8, d_rowstart + (size_t)c.t0 * ny, nrow * 4, hipMemcpyDeviceToHost, L.st) == hipSuccess;
            if (c.nr) good = good && hipMemcpyAsync(dst + nrow * W * 8 + ((nrow * 4 + 7) & ~(size_t)7), d_rv + c.r0, (size_t)c.nr * 4, hipMemcpyDeviceToHost, L.st) == hipSuccess;
            good = good && hipEventRecord(L.ev[b], L.st) == hipSuccess;
            if (!good) ok = false;
        };
        int b = 0;
        std::vector<int32_t> scratch((size_t)W * 64 + 16);
        if ((size_t)li < nb) fetch((size_t)li, 0);
        for (size_t bi = (size_t)li; bi < nb && ok; bi += (size_t)lanes, b ^= 1) {
            if (bi + (size_t)lanes < nb) fetch(bi + (size_t)lanes, b ^ 1);              // the next block travels while this one is expanded
            const double w0 = now_ms();
            if (hipEventSynchronize(L.ev[b]) != hipSuccess) { ok = false; break; }
            const double w1 = now_ms();
            bool z = false, c1 = false;
            rle_expand_block((const unsigned char *)L.pin[b].p, blocks[bi], rb.data(), ny, nx, W, flag, scratch.data(), z, c1);
            if (ctk_env().hosttrace) { wait_us += (int64_t)((w1 - w0) * 1e3); exp_us += (int64_t)((now_ms() - w1) * 1e3); }
            if (z) zero = true;
            if (c1) cx[bi] = 1;
        }
        (void)hipStreamSynchronize(L.st);                                             // (nothing of this call is left in flight on an error path)
    };
    const double tr1 = now_ms();
    if (!h->rle->crew.run(lanes, work)) ok = false;
    if (ctk_env().hosttrace) fprintf(stderr, "runs: %zu blocks on %d lanes | setup %.2f ms, lanes %.2f ms (per lane: waiting %.2f, expanding %.2f)\n", nb, lanes, tr1 - tr_begin, now_ms() - tr1, wait_us / 1e3 / lanes, exp_us / 1e3 / lanes);
    if (!ok) { (void)ctk_set_error(CTK_E_NODEVICE, "result transfer (run tables) failed: %s", hipGetErrorString(hipGetLastError())); return CTK_RLE_UNAVAILABLE; }
    // blocks with complex components: the write kernel, block by block
    int64_t ndense = 0;
    const size_t plane = (size_t)ny * nx;
    for (size_t bi = 0; bi < nb; bi++) {
        if (!cx[bi]) continue;
        const RleBlock &c = blocks[bi];
        CTKCHK(claim_io(h, h->io_out, (size_t)c.nt * plane * 4));
        h->rle_out = false;
        const int rc = launch_relabel(h, persistence, P<int32_t>(h->io_out), true, nullptr, c.t0, c.nt);
        h->rle_out = true;
        CTKCHK(rc);
        int32_t *dst = flag + (size_t)c.t0 * plane;
        HIPCHK(hipMemcpyAsync(dst, h->io_out.p, (size_t)c.nt * plane * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (!zero) { for (size_t i = 0; i < (size_t)c.nt * plane; i++) if (dst[i] == 0) { zero = true; break; } }
        ndense++;
    }
    h->stats[CTK_S_RLE_OUT] = 1 + ndense;
    *wrote_background = zero ? 1 : 0;
    return 0;
}

// (grids beyond 8 M pixels per timestep: the dense copy -- a timestep's tables are meant to fit a lane buffer of a few MB)
static bool runs_wanted(const ctk_handle *h, int ny, int nx)
{
    return (h->rle_mode < 0 ? ctk_env().rle_out : h->rle_mode >= 1) && rle_per_t(ny, (nx + 63) / 64) <= kRleBuf / 2;
}

// device pass + delivery of the result into the caller's host array (ctk_track_f32 / _f64 / ctk_track_resident)
static int track_to_host(ctk_handle *h, const void *a_dev, bool f64, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                         double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, double *t_pass_end)
{
    const size_t n = (size_t)T * ny * nx;
    bool want_runs = n > 0 && runs_wanted(h, ny, nx);
    int32_t *f_dev = nullptr;
    int rc;
    for (int attempt = 0; attempt < 2; attempt++) {
        // the dense result lives in the handle (grow-only); with the run transfer only the blocks of complex components ever need it
        CTKCHK(claim_io(h, h->io_out, want_runs ? 256 : std::max<size_t>(n * 4, 256)));
        f_dev = P<int32_t>(h->io_out);
        h->stats[CTK_S_RLE_OUT] = 0;
        h->rle_out = want_runs;
        struct RleOff { ctk_handle *h; ~RleOff() { h->rle_out = false; } } rle_off{h};
        rc = track_dev_impl(h, a_dev, f64, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, f_dev, n_tracked);
        if (t_pass_end) *t_pass_end = now_ms();
        if (rc != CTK_OK || !n) return rc;
        // huge pages where the allocation allows (the pages of a fresh result do not exist yet)
        const uintptr_t a0 = ((uintptr_t)flag + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1), a1 = ((uintptr_t)flag + n * 4) & ~(((uintptr_t)2 << 20) - 1);
        if (a1 > a0) (void)madvise((void *)a0, a1 - a0, MADV_HUGEPAGE);
        if (want_runs) {
            int wrote0 = 0;
            rc = deliver_runs(h, persistence, flag, &wrote0);
            if (rc == CTK_RLE_UNAVAILABLE) { want_runs = false; continue; }                // the pass again, with the write kernel and the dense copy
            if (rc != CTK_OK) return rc;
            if (n_tracked) *n_tracked = h->last_alive + (wrote0 ? 1 : 0) - 1;              // len(np.unique(flag)) - 1, contrack.py:793
            return CTK_OK;
        }
        break;
    }
    return download(h, f_dev, flag, n * 4);
}

static int track_host_impl(ctk_handle *h, const void *anom, bool f64, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                           double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (T < 0 || ny < 1 || nx < 1 || (T > 0 && (!anom || !flag))) return ctk_set_error(CTK_E_INVALID, "ctk_track: bad shape or null pointer");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)T * ny * nx, esz = f64 ? 8 : 4;
    void *a_dev = nullptr;
    if (n) {
        // the device copy of the caller's slab lives in the handle (grow-only), like every other buffer
        CTKCHK(claim_io(h, h->io_in, n * esz));
        a_dev = h->io_in.p;
    }
    const double e0 = now_ms();
    if (n) {
        hipError_t e = hipMemcpy(a_dev, anom, n * esz, hipMemcpyHostToDevice);
        if (e != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "H2D copy failed: %s", hipGetErrorString(e));
    }
    const double e1 = now_ms();
    double e2 = e1;
    const int rc = track_to_host(h, a_dev, f64, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag, n_tracked, &e2);
    const double e3 = now_ms();
    if (ctk_env().hosttrace) fprintf(stderr, "e2e: H2D %.1f ms | device path %.2f ms | result %.1f ms (%s)\n", e1 - e0, e2 - e1, e3 - e2, h->stats[CTK_S_RLE_OUT] ? "runs" : "dense");
    h->ms[CTK_T_H2D] = e1 - e0; h->ms[CTK_T_D2H] = e3 - e2; h->ms[CTK_T_TOTAL] = e3 - e0;      // (whole-call figures of the host entry)
    return rc;
}

// ------------------------------------------------------------------------------------------------
// streaming entries (next row N4): see include/contrack_hip.h.  The two pixel passes of the path (k_threshold, k_relabel) are
// independent per timestep; everything between them works on the bit mask and the tables.
// ------------------------------------------------------------------------------------------------
static int stream_setup(ctk_handle *h, size_t in_bytes, size_t out_bytes, bool pinned)
{
    HIPCHK(h->copy_stream.create(hipStreamNonBlocking));
    for (int b = 0; b < 2; b++)
        for (Event *e : {&h->ev_h2d[b], &h->ev_thr[b], &h->ev_rel[b], &h->ev_d2h[b]}) HIPCHK(e->create(hipEventDisableTiming));
    if (in_bytes) CTKCHK(claim_io(h, h->io_in, 2 * in_bytes));
    if (out_bytes) CTKCHK(claim_io(h, h->io_out, 2 * out_bytes));
    if (pinned) {
        if (h->pin_in.grow(in_bytes, hipHostMallocNonCoherent) != hipSuccess) return ctk_set_error(CTK_E_NOMEM, "pinned chunk buffer (%zu bytes)", in_bytes);
        if (h->pin_out.grow(out_bytes, hipHostMallocNonCoherent) != hipSuccess) return ctk_set_error(CTK_E_NOMEM, "pinned chunk buffer (%zu bytes)", out_bytes);
    }
    return CTK_OK;
}

// input phase: chunk k+1 travels (reader + H2D on the copy stream) while `consume` (k_threshold) works on chunk k.  A `consume` that
// only queues work returns at once and the loop goes on to the next chunk; one that waits for the device (io.ahead) is called after
// the next chunk has been sent off.
static int stream_in(ctk_handle *h, bool f64, int64_t T, int ny, int nx, const std::function<int(const void *, int64_t, int64_t)> &consume)
{
    StreamIO &io = *h->sio;
    const size_t plane = (size_t)ny * nx * io.esz, cbytes = (size_t)io.chunk * plane;
    (void)f64;
    const size_t plane2 = (size_t)ny * nx * io.esz2, cbytes2 = (size_t)io.chunk * plane2;
    CTKCHK(stream_setup(h, cbytes, 0, io.read != nullptr));
    if (io.esz2) CTKCHK(stream_setup(h, 0, cbytes2, io.read2 != nullptr));
    const double t_in = now_ms();
    io.passes_in++;
    struct Chunk { int b = 0; int64_t t0 = 0, nt = 0; const void *dev = nullptr, *dev2 = nullptr; } prev;
    auto use = [&](const Chunk &c) -> int {
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_h2d[c.b], 0));
        io.dev2 = c.dev2;
        CTKCHK(consume(c.dev, c.t0, c.nt));
        HIPCHK(hipEventRecord(h->ev_thr[c.b], h->stream));
        return CTK_OK;
    };
    int k = 0;
    for (int64_t t0 = 0; t0 < T; t0 += io.chunk, k++) {
        const int b = k & 1;
        const int64_t nt = std::min<int64_t>(io.chunk, T - t0);
        char *dev = (char *)h->io_in.p + (size_t)b * cbytes;
        Chunk cur;
        cur.b = b; cur.t0 = t0; cur.nt = nt; cur.dev = dev;
        if (k >= 2) HIPCHK(hipEventSynchronize(h->ev_thr[b]));                 // the device buffer (and its pinned twin) is free again
        if (io.esz2) {
            char *dev2 = (char *)h->io_out.p + (size_t)b * cbytes2;
            const void *src2 = (const char *)io.host_in2 + (size_t)t0 * plane2;
            if (io.read2) {
                const double r0 = now_ms();
                const int rc = io.read2(io.read2_user, t0, nt, h->pin_out[b]);
                io.ms_read += now_ms() - r0;
                if (rc) return ctk_set_error(CTK_E_INVALID, "the reader of the second slab returned %d for timesteps [%lld, %lld)", rc, (long long)t0, (long long)(t0 + nt));
                src2 = h->pin_out[b];
            }
            HIPCHK(hipMemcpyAsync(dev2, src2, (size_t)nt * plane2, hipMemcpyHostToDevice, h->copy_stream));
            cur.dev2 = dev2;
        }
        if (io.read) {
            const double r0 = now_ms();
            const int rc = io.read(io.read_user, t0, nt, h->pin_in[b]);
            io.ms_read += now_ms() - r0;
            if (rc) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream: the reader returned %d for timesteps [%lld, %lld)", rc, (long long)t0, (long long)(t0 + nt));
            HIPCHK(hipMemcpyAsync(dev, h->pin_in[b], (size_t)nt * plane, hipMemcpyHostToDevice, h->copy_stream));
        } else {
            // pageable source: the runtime stages it; the call returns when the data has left the caller's array
            HIPCHK(hipMemcpyAsync(dev, (const char *)io.host_in + (size_t)t0 * plane, (size_t)nt * plane, hipMemcpyHostToDevice, h->copy_stream));
        }
        HIPCHK(hipEventRecord(h->ev_h2d[b], h->copy_stream));
        if (io.ahead) {                                  // chunk k is on its way: now the chunk before it
            if (k > 0) CTKCHK(use(prev));
            prev = cur;
        } else CTKCHK(use(cur));
    }
    if (io.ahead && k > 0) CTKCHK(use(prev));
    io.ms_in += now_ms() - t_in;
    return CTK_OK;
}

// The streamed producers (vertical mean, reversal index, pass 2 of the streamed anomalies): a slab comes in chunk by chunk, a kernel
// runs on each chunk, a field of the same length leaves.  stream_produce owns the pipeline -- two input chunks in io_in, chunk k + 1
// travels in while the kernel works on chunk k and the output of chunk k - 1 leaves -- and a producer hands it what differs:
//   upload    queues the H2D copies of the chunk on copy_stream: from in.src, the pinned chunk the reader filled, or (null) from io.host_in
//   launch    queues the kernel(s) on the handle's stream, everything that must be done before the input chunk is reused included,
//             and says which output steps came out and where they lie (out.t0 < 0: none from this chunk)
//   download  optional: the copy of an output chunk into the host array where it is not whole steps (default: the bounce pool)
// The caller has called stream_setup; a writer gets the output through pin_out on side[0].
struct ProduceIn { int b = 0; int64_t c0 = 0, nt = 0; char *dev = nullptr; const char *src = nullptr; };      // chunk [c0, c0 + nt) in buffer b at dev
struct ProduceOut { int64_t t0 = -1, nt = 0; char *dev = nullptr; };
struct Producer {
    size_t in_bytes = 0;                           // of one input buffer, as passed to stream_setup
    size_t out_step = 0;                           // bytes of one output step
    std::function<int(const ProduceIn &)> upload;
    std::function<int(const ProduceIn &, ProduceOut &)> launch;
    std::function<int(const ProduceOut &, char *dst)> download;
};

static int stream_produce(ctk_handle *h, StreamIO &io, int64_t steps, const char *name, const Producer &p)
{
    const bool sink = io.host_out_v || io.write_v;
    const double t_pass = now_ms();
    io.passes_in++;
    if (io.host_out_v && !h->bounce) h->bounce.reset(new (std::nothrow) BouncePool());
    struct Pending { ProduceOut o; int b = 0; } pend;
    auto drain = [&](const Pending &q) -> int {                                  // output chunk q leaves the device
        if (q.o.t0 < 0) return CTK_OK;
        const double d0 = now_ms();
        const size_t bytes = (size_t)q.o.nt * p.out_step;
        HIPCHK(hipEventSynchronize(h->ev_rel[q.b]));
        if (io.write_v) {
            HIPCHK(hipMemcpyAsync(h->pin_out[q.b], q.o.dev, bytes, hipMemcpyDeviceToHost, h->side[0]));
            HIPCHK(hipEventRecord(h->ev_d2h[q.b], h->side[0]));
            HIPCHK(hipEventSynchronize(h->ev_d2h[q.b]));
            const double w0 = now_ms();
            const int rc = io.write_v(io.write_user, q.o.t0, q.o.nt, h->pin_out[q.b]);
            io.ms_write += now_ms() - w0;
            if (rc) return ctk_set_error(CTK_E_INVALID, "%s: the writer returned %d for steps [%lld, %lld)", name, rc, (long long)q.o.t0, (long long)(q.o.t0 + q.o.nt));
        } else {
            char *dst = (char *)io.host_out_v + (size_t)q.o.t0 * p.out_step;
            if (p.download) CTKCHK(p.download(q.o, dst));
            else if (!h->bounce || !bounce_copy(*h->bounce, h->device, q.o.dev, dst, bytes, false))
                HIPCHK(hipMemcpy(dst, q.o.dev, bytes, hipMemcpyDeviceToHost));
        }
        io.ms_out += now_ms() - d0;
        return CTK_OK;
    };
    int k = 0;
    for (int64_t c0 = 0; c0 < steps; c0 += io.chunk, k++) {
        ProduceIn in;
        const int b = in.b = k & 1;
        in.c0 = c0; in.nt = std::min<int64_t>(io.chunk, steps - c0);
        in.dev = (char *)h->io_in.p + (size_t)b * p.in_bytes;
        if (k >= 2) HIPCHK(hipEventSynchronize(h->ev_thr[b]));                 // the input chunk (and its pinned twin) is free again
        if (io.read) {
            const double r0 = now_ms();
            const int rc = io.read(io.read_user, c0, in.nt, h->pin_in[b]);
            io.ms_read += now_ms() - r0;
            if (rc) return ctk_set_error(CTK_E_INVALID, "%s: the reader returned %d for steps [%lld, %lld)", name, rc, (long long)c0, (long long)(c0 + in.nt));
            in.src = (const char *)h->pin_in[b];
        }
        CTKCHK(p.upload(in));
        HIPCHK(hipEventRecord(h->ev_h2d[b], h->copy_stream));
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_h2d[b], 0));
        ProduceOut out;
        CTKCHK(p.launch(in, out));
        if (out.t0 >= 0) HIPCHK(hipEventRecord(h->ev_rel[b], h->stream));
        HIPCHK(hipEventRecord(h->ev_thr[b], h->stream));
        CTKCHK(drain(pend));                                                    // (the chunk before this one; its output buffer is the other one)
        pend = Pending();
        if (sink && out.t0 >= 0) { pend.o = out; pend.b = b; }
    }
    CTKCHK(drain(pend));
    io.ms_in += now_ms() - t_pass - io.ms_out;
    return CTK_OK;
}

// the end of a streamed producer's call, rc what its chunks returned: after a failure nothing stays in flight; after a success the
// stream is idle and the handle has the timings of the call that began at t_call
static int stream_produce_end(ctk_handle *h, const StreamIO &io, int rc, double t_call)
{
    if (rc != CTK_OK) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamSynchronize(h->stream); return rc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    stream_ms_set(h, io);
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_D2H] = io.ms_out; h->ms[CTK_T_TOTAL] = now_ms() - t_call;
    return CTK_OK;
}

// What the producers of one plane per step share around stream_produce, as small functions each takes what fits it: ctk_level.hip the
// output side, ctk_subset.hip the upload, ctk_reversal.hip and ctk_lwa.hip all of it through the row-band producer below.

// the io of a *_stream_cb export of values: reader and writer as given, elem_bytes and the reader checked; who: the export
static int stream_cb_io(const char *who, const ctk_handle *h, int elem_bytes, ctk_read_chunk_fn reader, void *reader_user, ctk_write_values_fn writer, void *writer_user,
                        StreamIO &io)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "%s: elem_bytes must be 4 (float32) or 8 (float64)", who);
    if (h && !reader) return ctk_set_error(CTK_E_INVALID, "%s: null reader", who);
    io.read = reader; io.read_user = reader_user; io.write_v = writer; io.write_user = writer_user;
    return CTK_OK;
}

// Producer::upload of chunks that travel whole: c.nt steps of `step` bytes, from the pinned chunk the reader filled or from io.host_in
static int upload_steps(ctk_handle *h, const StreamIO &io, const ProduceIn &c, size_t step)
{
    const char *src = c.src ? c.src : (const char *)io.host_in + (size_t)c.c0 * step;
    HIPCHK(hipMemcpyAsync(c.dev, src, (size_t)c.nt * step, hipMemcpyHostToDevice, h->copy_stream));
    return CTK_OK;
}

// the output side of a call that may keep its result: with keep_resident all `steps` planes stay in `resident` and chunk buffers are
// wanted for a writer only; without, two chunks in io_out, with pinned twins for a writer
static int produce_out_setup(ctk_handle *h, const StreamIO &io, DevBuf &resident, int64_t steps, size_t plane, int keep_resident)
{
    if (keep_resident) {
        CTKCHK(ensure(h, resident, (size_t)steps * plane));
        if (io.write_v) CTKCHK(stream_setup(h, 0, (size_t)io.chunk * plane, true));
    } else {
        CTKCHK(stream_setup(h, 0, (size_t)io.chunk * plane, io.write_v != nullptr));
    }
    return CTK_OK;
}
// ... and where the planes of chunk c go then
static char *produce_out_dev(ctk_handle *h, const StreamIO &io, const DevBuf &resident, const ProduceIn &c, size_t plane, int keep_resident)
{
    return keep_resident ? (char *)resident.p + (size_t)c.c0 * plane : (char *)h->io_out.p + (size_t)c.b * (size_t)io.chunk * plane;
}

// rows of every plane of `out` (steps, ny, nx) outside the `width` bytes from byte `off` on: zero
static void zero_other_rows(void *out, int64_t steps, size_t plane, size_t off, size_t width)
{
    if (width == plane) return;
    for (int64_t s = 0; s < steps; s++) {
        char *p = (char *)out + (size_t)s * plane;
        memset(p, 0, off);
        memset(p + off + width, 0, plane - off - width);
    }
}

// The row-band plane producer (ctk_reversal_*, ctk_lwa_*): a kernel over (steps, ny, nx) planes that reads only the rows [r0, r1) of a
// plane and writes zeros outside its rows [a0, a1).  Of a host array only rows [r0, r1) of every plane travel to the device (one
// strided copy per chunk, the plane as pitch) and only rows [a0, a1) travel back; the rest of the output array is zeroed on the host.
// The device chunks keep the full-plane layout, readers fill and writers get whole planes.  keep_resident: the full-plane result is
// written into the resident slot of the field to track (an_slab), where ctk_track_resident and the `resident` consumers find it.
struct RowBands { int r0, r1, a0, a1; };

// its argument checks, in the order the entries report them, and the chunk plan: io.esz and io.chunk are set, no buffer is touched
static int row_band_begin(ctk_handle *h, StreamIO &io, int64_t steps, size_t plane, size_t esz, int64_t chunk_steps, int keep_resident, const char *name)
{
    if (!io.read && !io.host_in) return ctk_set_error(CTK_E_INVALID, "%s: null input", name);
    const bool sink = io.host_out_v || io.write_v;
    if (!sink && !keep_resident) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output and keep_resident = 0)", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", name, (long long)chunk_steps);
    HIPCHK(hipSetDevice(h->device));
    io.esz = esz;
    io.chunk = ctk_stream_chunk(chunk_steps, steps, plane);
    return CTK_OK;
}

// ... and the call itself after row_band_begin.  tables: uploads the family's device tables once the chunk buffers stand; launch:
// queues the kernels of chunk c on the handle's stream, the planes of its steps going to `out`.
static int row_band_produce(ctk_handle *h, StreamIO &io, int64_t steps, int ny, int nx, const RowBands &rb, int keep_resident, const char *name,
                            const std::function<int()> &tables, const std::function<int(const ProduceIn &c, char *out)> &launch)
{
    const size_t row = (size_t)nx * io.esz, plane = (size_t)ny * row;
    const double t_call = now_ms();
    CTKCHK(stream_setup(h, (size_t)io.chunk * plane, 0, io.read != nullptr));
    if (keep_resident) { h->an_slab.drop(); h->an_pct_n = -1; }
    CTKCHK(produce_out_setup(h, io, h->an_slab.buf, steps, plane, keep_resident));
    CTKCHK(tables());
    const size_t in_off = (size_t)rb.r0 * row, in_w = (size_t)(rb.r1 - rb.r0) * row, out_off = (size_t)rb.a0 * row, out_w = (size_t)(rb.a1 - rb.a0) * row;
    // the rows of `out` that nothing is downloaded into are zeroed by a helper thread while the chunks travel (other bytes than the
    // copies write; at 1 degree, one hemisphere, that is three quarters of the array)
    struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } zero;
    if (io.host_out_v) zero.t = std::thread(zero_other_rows, io.host_out_v, steps, plane, out_off, out_w);
    // the chunks (stream_produce): io.host_in is the whole (steps, ny, nx) array (rows [r0, r1) of every plane travel), io.read a
    // reader of whole planes.  The results go to io.host_out_v (rows [a0, a1) of every plane) / io.write_v (whole planes) chunk by
    // chunk and (keep) into an_slab.
    Producer p;
    p.in_bytes = (size_t)io.chunk * plane; p.out_step = plane;
    p.upload = [&](const ProduceIn &c) -> int {
        if (in_w == plane) return upload_steps(h, io, c, plane);
        // (an empty band: a reversal table without an active row.  ctk_lwa_* never has one: lwa_check wants a row in every domain.)
        const char *src = c.src ? c.src : (const char *)io.host_in + (size_t)c.c0 * plane;
        if (in_w) HIPCHK(hipMemcpy2DAsync(c.dev + in_off, plane, src + in_off, plane, in_w, (size_t)c.nt, hipMemcpyHostToDevice, h->copy_stream));      // row s of the copy: rows [r0, r1) of step c0 + s
        return CTK_OK;
    };
    p.launch = [&](const ProduceIn &c, ProduceOut &o) -> int {
        o.t0 = c.c0; o.nt = c.nt;
        o.dev = produce_out_dev(h, io, h->an_slab.buf, c, plane, keep_resident);
        return launch(c, o.dev);
    };
    if (out_w != plane)
        p.download = [&](const ProduceOut &o, char *dst) -> int {
            if (out_w) HIPCHK(hipMemcpy2D(dst + out_off, plane, o.dev + out_off, plane, out_w, (size_t)o.nt, hipMemcpyDeviceToHost));
            return CTK_OK;
        };
    const int rc = stream_produce(h, io, steps, name, p);
    if (zero.t.joinable()) zero.t.join();
    CTKCHK(stream_produce_end(h, io, rc, t_call));
    if (keep_resident) h->an_slab.keep(steps, ny, nx, io.esz == 8);
    return CTK_OK;
}

// The windowed producer (pass 2 of ctk_anom_stream_*, ctk_filter_*): a kernel whose outputs read up to `halo` steps in front of their
// chunk.  The chunks pass through two windows [halo steps kept from the chunk before | chunk] in io_in -- io.chunk >= halo, and the
// caller's stream_setup gave each window (io.chunk + halo) * plane bytes --: a chunk is uploaded behind the halo and its last `halo`
// steps are copied in front of the next one on the device, so the reader is never asked for a step twice.
//   done_at(end, from)  the outputs, counted on from `from`, that are complete once the steps below `end` are there (end == steps: all)
//   place(b, o0)        where the outputs from o0 on of the chunk in buffer b go
//   launch              queues their kernel on the handle's stream: plane 0 of `window` is step xbase, its steps [xlo, xhi) may be
//                       read, the outputs [o0, o1) go to `out`
static int window_produce(ctk_handle *h, StreamIO &io, int64_t steps, int64_t halo, size_t plane, const char *name,
                          const std::function<int64_t(int64_t end, int64_t from)> &done_at, const std::function<char *(int b, int64_t o0)> &place,
                          const std::function<int(const char *window, int64_t xbase, int64_t xlo, int64_t xhi, int64_t o0, int64_t o1, char *out)> &launch)
{
    int64_t o_done = 0;
    Producer p;
    p.in_bytes = (size_t)(io.chunk + halo) * plane; p.out_step = plane;
    p.upload = [&](const ProduceIn &c) -> int {
        const char *src = c.src ? c.src : (const char *)io.host_in + (size_t)c.c0 * plane;
        HIPCHK(hipMemcpyAsync(c.dev + (size_t)halo * plane, src, (size_t)c.nt * plane, hipMemcpyHostToDevice, h->copy_stream));
        return CTK_OK;
    };
    p.launch = [&](const ProduceIn &c, ProduceOut &o) -> int {
        // steps [c0 - halo, c0 + nt) are in the window now (the first chunk has nothing in front of it)
        const int64_t xlo = c.c0 == 0 ? 0 : c.c0 - halo, o0 = o_done, o1 = done_at(c.c0 + c.nt, o_done);
        if (o1 > o0) {
            o.t0 = o0; o.nt = o1 - o0; o.dev = place(c.b, o0);
            CTKCHK(launch(c.dev, c.c0 - halo, xlo, c.c0 + c.nt, o0, o1, o.dev));
        }
        // the last `halo` steps in front of the next chunk (a chunk that is not the last has nt == chunk >= halo steps: they lie in its body)
        if (c.c0 + c.nt < steps && halo > 0)
            HIPCHK(hipMemcpyAsync((char *)h->io_in.p + (size_t)(c.b ^ 1) * p.in_bytes, c.dev + (size_t)c.nt * plane, (size_t)halo * plane, hipMemcpyDeviceToDevice, h->stream));
        o_done = o1;
        return CTK_OK;
    };
    return stream_produce(h, io, steps, name, p);
}

// output phase: k_relabel writes chunk k+1 into one device buffer while chunk k leaves the other
static int stream_out(ctk_handle *h, int persistence, const int32_t *chunk_vals)
{
    if (h->rle_out) return CTK_OK;                                               // (array sink: the result leaves as run tables after the pass)
    StreamIO &io = *h->sio;
    const int64_t T = h->T;
    const size_t plane = (size_t)h->ny * h->nx * 4, cbytes = (size_t)io.chunk * plane;
    CTKCHK(stream_setup(h, 0, cbytes, io.write != nullptr));
    const double t_out = now_ms();
    if (io.host_out) {                                                           // huge pages where the allocation allows (first-touch faults)
        const uintptr_t a0 = ((uintptr_t)io.host_out + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1);
        const uintptr_t a1 = ((uintptr_t)io.host_out + (size_t)T * plane) & ~(((uintptr_t)2 << 20) - 1);
        if (a1 > a0) (void)madvise((void *)a0, a1 - a0, MADV_HUGEPAGE);
        if (!h->bounce) h->bounce.reset(new (std::nothrow) BouncePool());
    }
    struct Pending { int64_t t0 = -1, nt = 0; int b = 0; } pend;
    auto drain = [&](const Pending &p) -> int {                                 // chunk p leaves the device
        if (p.t0 < 0) return CTK_OK;
        int32_t *dev = (int32_t *)((char *)h->io_out.p + (size_t)p.b * cbytes);
        HIPCHK(hipEventSynchronize(h->ev_rel[p.b]));
        if (io.write) {
            HIPCHK(hipMemcpyAsync(h->pin_out[p.b], dev, (size_t)p.nt * plane, hipMemcpyDeviceToHost, h->copy_stream));
            HIPCHK(hipEventRecord(h->ev_d2h[p.b], h->copy_stream));
            HIPCHK(hipEventSynchronize(h->ev_d2h[p.b]));
            const double w0 = now_ms();
            const int rc = io.write(io.write_user, p.t0, p.nt, (const int32_t *)h->pin_out[p.b]);
            io.ms_write += now_ms() - w0;
            if (rc) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream: the writer returned %d for timesteps [%lld, %lld)", rc, (long long)p.t0, (long long)(p.t0 + p.nt));
        } else {
            char *dst = (char *)io.host_out + (size_t)p.t0 * plane;
            if (!h->bounce || !bounce_copy(*h->bounce, h->device, dev, dst, (size_t)p.nt * plane, false))
                HIPCHK(hipMemcpy(dst, dev, (size_t)p.nt * plane, hipMemcpyDeviceToHost));
        }
        return CTK_OK;
    };
    int k = 0;
    for (int64_t t0 = 0; t0 < T; t0 += io.chunk, k++) {
        const int b = k & 1;
        const int64_t nt = std::min<int64_t>(io.chunk, T - t0);
        int32_t *dev = (int32_t *)((char *)h->io_out.p + (size_t)b * cbytes);
        // buffer b was drained two chunks ago (drain is synchronous): relabel chunk k into it, then drain chunk k-1 meanwhile
        CTKCHK(launch_relabel(h, persistence, dev, true, chunk_vals, t0, nt));
        HIPCHK(hipEventRecord(h->ev_rel[b], h->stream));
        CTKCHK(drain(pend));
        pend.t0 = t0; pend.nt = nt; pend.b = b;
    }
    CTKCHK(drain(pend));
    io.ms_out += now_ms() - t_out;
    return CTK_OK;
}

static int track_stream_impl(ctk_handle *h, StreamIO &io, bool f64, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                             double overlap, int persistence, int twosided, int64_t *n_tracked, int64_t chunk_steps,
                             const int64_t *starts = nullptr, int64_t nseg = 0, bool seg_entry = false /* an entry with segment arguments */)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (T < 0 || ny < 1 || nx < 1 || chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream: bad shape");
    if (!seg_entry && !h->seg_starts.empty())
        return ctk_set_error(CTK_E_INVALID, "ctk_track_stream: segments are set on this handle (ctk_set_segments); the streaming entries take them as an argument (ctk_track_stream_seg_*)");
    // segment starts of THIS call: kept in the handle while it runs, so that every pass through track_dev_impl -- the dense re-run
    // below, the route through the time-shard path, the host resolver -- builds and sees the same edge table
    struct SegCall { ctk_handle *h; ~SegCall() { h->seg_call.clear(); } } seg_call{h};
    if (seg_entry) {
        CTKCHK(segment_args_check(h, "ctk_track_stream_seg", starts, nseg, std::max<int64_t>(T, 1)));
        if (nseg > 1) h->seg_call.assign(starts, starts + nseg);         // (one segment: the unsegmented call)
    }
    if (T > 0 && ((!io.host_in && !io.read) || (!io.host_out && !io.write))) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream: no source or no sink");
    HIPCHK(hipSetDevice(h->device));
    io.esz = f64 ? 8 : 4;
    const size_t plane = (size_t)ny * nx * io.esz;
    io.chunk = ctk_stream_chunk(chunk_steps, std::max<int64_t>(T, 1), plane);
    const double t0 = now_ms();
    h->sio = &io;
    // an array as the sink: the result needs no chunks -- the run tables of the whole slab are resident when the pass is over
    // (deliver_runs); a writer callback gets dense chunks in pinned buffers as before
    h->rle_out = T > 0 && io.host_out && runs_wanted(h, ny, nx);
    h->stats[CTK_S_RLE_OUT] = 0;
    int rc = track_dev_impl(h, nullptr, f64, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, nullptr, n_tracked);
    if (rc == CTK_OK && h->rle_out) {
        const double o0 = now_ms();
        const size_t nb = (size_t)T * ny * nx * 4;
        const uintptr_t a0 = ((uintptr_t)io.host_out + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1), a1 = ((uintptr_t)io.host_out + nb) & ~(((uintptr_t)2 << 20) - 1);
        if (a1 > a0) (void)madvise((void *)a0, a1 - a0, MADV_HUGEPAGE);
        int wrote0 = 0;
        rc = deliver_runs(h, persistence, io.host_out, &wrote0);
        if (rc == CTK_OK && n_tracked) *n_tracked = h->last_alive + (wrote0 ? 1 : 0) - 1;      // len(np.unique(flag)) - 1, contrack.py:793
        io.ms_out += now_ms() - o0;
        if (rc == CTK_RLE_UNAVAILABLE) {                       // the slab streams through once more, the result leaves in dense chunks
            h->rle_out = false;
            h->stats[CTK_S_RLE_OUT] = 0;
            rc = track_dev_impl(h, nullptr, f64, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, nullptr, n_tracked);
        }
    }
    h->sio = nullptr;
    h->rle_out = false;
    stream_ms_set(h, io);
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_D2H] = io.ms_out; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return rc;
}

extern "C" int ctk_track_stream_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                                    double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = anom; io.host_out = flag;
    return track_stream_impl(h, io, false, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps);
}
extern "C" int ctk_track_stream_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                                    double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = anom; io.host_out = flag;
    return track_stream_impl(h, io, true, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps);
}
extern "C" int ctk_track_stream_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const double *thr,
                                   int cmp_op, const float *wrow, double overlap, int persistence, int twosided, ctk_write_chunk_fn writer,
                                   void *writer_user, int64_t *n_tracked, int64_t chunk_steps)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    StreamIO io;
    io.read = reader; io.read_user = reader_user; io.write = writer; io.write_user = writer_user;
    return track_stream_impl(h, io, elem_bytes == 8, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps);
}
// ... with segment breaks as an argument of the call (include/contrack_hip.h)
extern "C" int ctk_track_stream_seg_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                                        double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps,
                                        const int64_t *starts, int64_t nseg)
{
    StreamIO io;
    io.host_in = anom; io.host_out = flag;
    return track_stream_impl(h, io, false, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps, starts, nseg, true);
}
extern "C" int ctk_track_stream_seg_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                                        double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked, int64_t chunk_steps,
                                        const int64_t *starts, int64_t nseg)
{
    StreamIO io;
    io.host_in = anom; io.host_out = flag;
    return track_stream_impl(h, io, true, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps, starts, nseg, true);
}
extern "C" int ctk_track_stream_seg_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const double *thr,
                                       int cmp_op, const float *wrow, double overlap, int persistence, int twosided, ctk_write_chunk_fn writer,
                                       void *writer_user, int64_t *n_tracked, int64_t chunk_steps, const int64_t *starts, int64_t nseg)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_track_stream_seg_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    StreamIO io;
    io.read = reader; io.read_user = reader_user; io.write = writer; io.write_user = writer_user;
    return track_stream_impl(h, io, elem_bytes == 8, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, n_tracked, chunk_steps, starts, nseg, true);
}
extern "C" int ctk_stream_times(ctk_handle *h, double *ms4)
{
    if (!h || !ms4) return ctk_set_error(CTK_E_INVALID, "null argument");
    for (int i = 0; i < 4; i++) ms4[i] = h->stream_ms[i];
    return CTK_OK;
}

// frees the device copies the host-array entries keep between calls (slab + result: twice the slab size) and the bounce lanes
extern "C" int ctk_release_io(ctk_handle *h)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    for (DevBuf *b : {&h->io_in, &h->io_out, &h->an_raw, &h->fl_out, &h->gr_tab, &h->lw_tab, &h->lw_ref}) b->release();
    h->an_slab.release(); h->an_pct_n = -1;
    h->lv_slab.release();
    h->io_gen++; h->lc_flag = nullptr; h->lc_field = nullptr;          // (the exact rows of a lifecycle call read those slabs)
    h->bounce.reset();
    h->rle.reset();
    stream_teardown(h);
    return CTK_OK;
}

extern "C" int ctk_track_f32_dev(ctk_handle *h, const float *anom_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                                 const float *wrow, double overlap, int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked)
{
    return track_dev_impl(h, anom_dev, false, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag_dev, n_tracked);
}
extern "C" int ctk_track_f64_dev(ctk_handle *h, const double *anom_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                                 const float *wrow, double overlap, int persistence, int twosided, int32_t *flag_dev, int64_t *n_tracked)
{
    return track_dev_impl(h, anom_dev, true, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag_dev, n_tracked);
}
extern "C" int ctk_track_f32(ctk_handle *h, const float *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                             double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked)
{
    return track_host_impl(h, anom, false, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag, n_tracked);
}
extern "C" int ctk_track_f64(ctk_handle *h, const double *anom, int64_t T, int ny, int nx, const double *thr, int cmp_op, const float *wrow,
                             double overlap, int persistence, int twosided, int32_t *flag, int64_t *n_tracked)
{
    return track_host_impl(h, anom, true, T, ny, nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag, n_tracked);
}

// ------------------------------------------------------------------------------------------------
// debug / staged parity
// ------------------------------------------------------------------------------------------------
extern "C" int ctk_debug_mask(ctk_handle *h, uint8_t *mask)
{
    if (!h || !mask) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state < ST_LABELLED) return ctk_set_error(CTK_E_STATE, "no labelled shard");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->T * h->ny * (int64_t)h->nx;
    if (n == 0) return CTK_OK;
    CTKCHK(ensure(h, h->dbg, (size_t)n));
    k_expand_mask<<<(int)std::min<int64_t>((n + 255) / 256, 1 << 20), 256, 0, h->stream>>>(P<uint64_t>(h->mask), h->T * h->ny, h->nx, h->W, P<uint8_t>(h->dbg));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mask, h->dbg.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_debug_label2d(ctk_handle *h, int before_seam, int32_t *lab)
{
    if (!h || !lab) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->state < ST_LABELLED) return ctk_set_error(CTK_E_STATE, "no labelled shard");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = h->T * h->ny * (int64_t)h->nx;
    if (n == 0) return CTK_OK;
    CTKCHK(ensure(h, h->dbg, (size_t)n * 4));
    k_run_values<<<(int)h->T, 256, 0, h->stream>>>(P<uint32_t>(h->run_base), P<uint32_t>(h->run_comp), CPX(h), nullptr, nullptr, 0, 0,
                                                   P<uint32_t>(h->d_mrep), 0, before_seam ? 1 : 2, P<int32_t>(h->run_val));
    HIPCHK(hipGetLastError());
    const int64_t tb = h->t_begin;
    h->t_begin = 0;
    int rc = launch_relabel(h, 0, P<int32_t>(h->dbg), false);
    h->t_begin = tb;
    CTKCHK(rc);
    HIPCHK(hipMemcpyAsync(lab, h->dbg.p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

// ------------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------------
// run_lifecycle reductions (contrack.py:798-906): one row per (time step, flag id)
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(ctk_life_row) == sizeof(CtkLifeRowDev), "row layouts must agree");

static_assert(CTK_LIFE_SW == LB_SW && CTK_LIFE_WAVES == LB_THREADS / 64, "ctk_forms.h restates the strip shape of ctk_lifecycle.hip");

// One pass of the reductions over the T time steps of a slab in device memory: the whole slab of a resident call, one chunk of a
// streamed one (ctk_life_stream.hip).  life_launch queues the strip kernels and the copy of their counters, life_settle waits for
// them, redoes the time steps they gave up and -- once -- everything, if the row table was too small.
struct LifeRun {
    const int32_t *flag = nullptr; const void *field = nullptr;
    bool f64 = false; int64_t T = 0; int ny = 0, nx = 0;
    int32_t wshift = 0, limb_bits = 0;
    int64_t t_base = 0;                            // lc_rounds[t_base + t] counts the rounds of this pass's time step t
    CtkLifePlan plan = {0, 0, 0, 0, 0};
    size_t cap = 0;                                // rows the table holds
    unsigned long long cnt[2] = {0, 0};            // rows written | time steps (work items) given up
    int64_t given_up = 0, fb_launches = 0; int attempts = 0;
};

// the row weights of a call: limbs and float32 values to the device
static int life_weights(ctk_handle *h, const float *wrow, int ny, int nx, int32_t *wshift, int32_t *limb_bits)
{
    std::vector<int64_t> wlo(ny), whi(ny);
    CTKCHK(ctk_weights_to_limbs(wrow, ny, (int64_t)ny * nx, wlo.data(), whi.data(), wshift, limb_bits));
    CTKCHK(ensure(h, h->lc_wlo, (size_t)ny * 8));
    CTKCHK(ensure(h, h->lc_whi, (size_t)ny * 8));
    CTKCHK(ensure(h, h->lc_w, (size_t)ny * 4));
    CTKCHK(ensure(h, h->lc_cnt, 16));
    HIPCHK(hipMemcpyAsync(h->lc_wlo.p, wlo.data(), (size_t)ny * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->lc_whi.p, whi.data(), (size_t)ny * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->lc_w.p, wrow, (size_t)ny * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));          // wlo / whi are stack-lifetime vectors
    return CTK_OK;
}

// Banded form (every byte read once, T x chunks workgroups); the time steps it gives up (more ids than its tables hold) are
// redone by k_lifecycle in life_settle, which splits further by residue classes of the ids.
static int life_launch(ctk_handle *h, LifeRun &r)
{
    const int64_t T = r.T;
    const int ny = r.ny, nx = r.nx, nxw = (nx + 31) / 32;
    const CtkLifePlan &plan = r.plan;
    const int rw = plan.rw, nsx = plan.nsx, nby = plan.nby, nb = nsx * nby;
    const size_t gkey_bytes = (size_t)T * LB_GH * 4, gacc_bytes = (size_t)T * LB_GH * sizeof(CtkLifeAcc);
    const size_t occ_bytes = (size_t)T * LB_KS * nxw * 4, cp_bytes = (size_t)T * LB_KS * nx * 8;
    if ((uint64_t)T * (uint64_t)nb > 0x7fffffffull) return ctk_set_error(CTK_E_RANGE, "ctk_lifecycle: %lld time steps x %d chunks beyond one launch", (long long)T, nb);
    CTKCHK(ensure(h, h->lc_cross, (size_t)T * (LB_KS + 1) * 4));
    CTKCHK(ensure(h, h->lc_gtab, gkey_bytes + gacc_bytes));
    CTKCHK(ensure(h, h->lc_occ, occ_bytes));
    CTKCHK(ensure(h, h->lc_cp, cp_bytes));
    int32_t *gkey = P<int32_t>(h->lc_gtab);
    CtkLifeAcc *gacc = (CtkLifeAcc *)((char *)h->lc_gtab.p + gkey_bytes);
    r.attempts++;                                     // (what follows describes the attempt whose rows are returned)
    r.given_up = 0; r.fb_launches = 0;
    std::fill(h->lc_rounds.begin() + r.t_base, h->lc_rounds.begin() + r.t_base + T, (uint8_t)0);
    CTKCHK(ensure(h, h->lc_rows, r.cap * sizeof(CtkLifeRowDev)));
    r.cap = h->lc_rows.cap / sizeof(CtkLifeRowDev);
    const size_t cap = r.cap;
    CTKCHK(ensure(h, h->lc_ovf, (size_t)T));
    HIPCHK(hipMemsetAsync(h->lc_cnt.p, 0, 16, h->stream));
    HIPCHK(hipMemsetAsync(h->lc_ovf.p, 0, (size_t)T, h->stream));
    HIPCHK(hipMemsetAsync(h->lc_gtab.p, 0, gkey_bytes + gacc_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->lc_occ.p, 0, occ_bytes, h->stream));
    HIPCHK(hipMemsetAsync(h->lc_cp.p, 0, cp_bytes, h->stream));
    k_life_seam<<<(unsigned)T, 64, 0, h->stream>>>(r.flag, ny, nx, P<int32_t>(h->lc_cross), P<unsigned char>(h->lc_ovf));
    {
        const bool vec = plan.vec != 0;
        const unsigned grid = (unsigned)(T * nb);
#define CTK_LIFE_STRIPS(VT, VEC)                                                                                                                       \
    k_life_strips<VT, VEC><<<grid, LB_THREADS, 0, h->stream>>>(r.flag, (const VT *)r.field, ny, nx, nxw, nsx, nby, rw, P<int64_t>(h->lc_wlo),          \
                                                               P<int64_t>(h->lc_whi), P<float>(h->lc_w), P<int32_t>(h->lc_cross), gkey, gacc,         \
                                                               P<unsigned>(h->lc_occ), P<double>(h->lc_cp), P<unsigned char>(h->lc_ovf))
        if (r.f64) { if (vec) CTK_LIFE_STRIPS(double, true); else CTK_LIFE_STRIPS(double, false); }
        else { if (vec) CTK_LIFE_STRIPS(float, true); else CTK_LIFE_STRIPS(float, false); }
#undef CTK_LIFE_STRIPS
    }
    k_life_finish<<<(unsigned)T, LB_GH, 0, h->stream>>>(nx, nxw, P<int32_t>(h->lc_cross), gkey, gacc, P<unsigned>(h->lc_occ), P<double>(h->lc_cp), r.wshift,
                                                        r.limb_bits, P<CtkLifeRowDev>(h->lc_rows), cap, P<unsigned long long>(h->lc_cnt),
                                                        P<unsigned char>(h->lc_ovf));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(r.cnt, h->lc_cnt.p, 16, hipMemcpyDeviceToHost, h->stream));
    return CTK_OK;
}

static int life_settle(ctk_handle *h, LifeRun &r)
{
    const int64_t T = r.T;
    const int ny = r.ny, nx = r.nx, nxw = (nx + 31) / 32, ks = r.plan.ks;
    auto launch = [&](const int32_t *work, unsigned items) -> int {
        if (r.f64)
            k_lifecycle<double><<<items, LC_THREADS, (size_t)ks * nxw * 4, h->stream>>>(r.flag, (const double *)r.field, ny, nx, nxw, ks, P<int64_t>(h->lc_wlo),
                                                                                        P<int64_t>(h->lc_whi), P<float>(h->lc_w), r.wshift, r.limb_bits,
                                                                                        P<CtkLifeRowDev>(h->lc_rows), r.cap, P<unsigned long long>(h->lc_cnt), work,
                                                                                        P<unsigned char>(h->lc_ovf));
        else
            k_lifecycle<float><<<items, LC_THREADS, (size_t)ks * nxw * 4, h->stream>>>(r.flag, (const float *)r.field, ny, nx, nxw, ks, P<int64_t>(h->lc_wlo),
                                                                                       P<int64_t>(h->lc_whi), P<float>(h->lc_w), r.wshift, r.limb_bits,
                                                                                       P<CtkLifeRowDev>(h->lc_rows), r.cap, P<unsigned long long>(h->lc_cnt), work,
                                                                                       P<unsigned char>(h->lc_ovf));
        HIPCHK(hipGetLastError());
        return CTK_OK;
    };
    unsigned long long *cnt = r.cnt;
    for (;;) {
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<int32_t> work;
        if (cnt[1]) {
            std::vector<unsigned char> ov((size_t)T);
            HIPCHK(hipMemcpy(ov.data(), h->lc_ovf.p, (size_t)T, hipMemcpyDeviceToHost));
            for (int64_t t = 0; t < T; ++t) if (ov[(size_t)t]) { work.push_back((int32_t)t); work.push_back(1); work.push_back(0); }
            r.given_up = (int64_t)(work.size() / 3);
        }
        while (!work.empty()) {
            const size_t items = work.size() / 3;
            if (work[1] > (1 << 24)) return ctk_set_error(CTK_E_RANGE, "ctk_lifecycle: a time step's flag ids cannot be split into passes that fit");
            CTKCHK(ensure(h, h->lc_work, work.size() * 4));
            CTKCHK(ensure(h, h->lc_ovf, std::max<size_t>(items, (size_t)T)));
            HIPCHK(hipMemcpy(h->lc_work.p, work.data(), work.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemsetAsync(h->lc_ovf.p, 0, items, h->stream));
            unsigned long long zero = 0;
            HIPCHK(hipMemcpyAsync(P<unsigned long long>(h->lc_cnt) + 1, &zero, 8, hipMemcpyHostToDevice, h->stream));
            CTKCHK(launch(P<int32_t>(h->lc_work), (unsigned)items));
            r.fb_launches++;
            for (size_t i = 0; i < items; ++i) {          // (the items of one time step follow each other)
                if (i && work[3 * i] == work[3 * (i - 1)]) continue;
                uint8_t &rd = h->lc_rounds[(size_t)(r.t_base + work[3 * i])];
                if (rd < 255) rd++;
            }
            HIPCHK(hipMemcpyAsync(cnt, h->lc_cnt.p, 16, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            std::vector<int32_t> next;
            if (cnt[1]) {
                std::vector<unsigned char> ov(items);
                HIPCHK(hipMemcpy(ov.data(), h->lc_ovf.p, items, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < items; ++i)
                    if (ov[i]) for (int j = 0; j < 2; ++j) { next.push_back(work[3 * i]); next.push_back(work[3 * i + 1] * 2); next.push_back(work[3 * i + 2] + j * work[3 * i + 1]); }
            }
            work.swap(next);
        }
        if (cnt[0] <= r.cap) break;
        if (r.attempts == 2) return ctk_set_error(CTK_E_INTERNAL, "ctk_lifecycle: row count changed between passes");
        r.cap = (size_t)cnt[0];
        CTKCHK(life_launch(h, r));
    }
    return CTK_OK;
}

// rows leave the device in arbitrary order; the reference's frame is sorted by (Flag, Date) (contrack.py:906).
// Two stable counting sorts (by t, then by label) when the label range is small, else a comparison sort of keys.
// land[0..n) with t in [0, T) -> out; returns the order taken (0 counting sorts, 1 comparison sort)
static int life_sort(ctk_handle *h, const ctk_life_row *land, size_t n, int64_t T, std::vector<ctk_life_row> &out)
{
    h->lc_tmp.resize(n);
    out.resize(n);
    int32_t lmin = INT32_MAX, lmax = INT32_MIN;
    for (size_t i = 0; i < n; ++i) { lmin = std::min(lmin, land[i].label); lmax = std::max(lmax, land[i].label); }
    const uint64_t lrange = n ? (uint64_t)((int64_t)lmax - (int64_t)lmin) + 1 : 0;
    const int order = (!n || lrange <= 8 * (uint64_t)n + 65536) ? 0 : 1;
    if (!order) {
        std::vector<uint32_t> &cnt = h->lc_cnt_host;
        cnt.assign((size_t)T + 1, 0);
        for (size_t i = 0; i < n; ++i) cnt[(size_t)land[i].t + 1]++;
        for (int64_t t = 0; t < T; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
        for (size_t i = 0; i < n; ++i) h->lc_tmp[cnt[(size_t)land[i].t]++] = land[i];                  // by t
        cnt.assign((size_t)lrange + 1, 0);
        for (size_t i = 0; i < n; ++i) cnt[(size_t)((int64_t)h->lc_tmp[i].label - lmin) + 1]++;
        for (uint64_t k = 0; k < lrange; ++k) cnt[(size_t)k + 1] += cnt[(size_t)k];
        for (size_t i = 0; i < n; ++i) out[cnt[(size_t)((int64_t)h->lc_tmp[i].label - lmin)]++] = h->lc_tmp[i];   // by label, stable
    } else {
        std::vector<std::pair<uint64_t, uint32_t>> &keys = h->lc_keys;
        keys.resize(n);
        for (size_t i = 0; i < n; ++i)
            keys[i] = {((uint64_t)((uint32_t)land[i].label ^ 0x80000000u) << 32) | (uint32_t)land[i].t, (uint32_t)i};
        std::sort(keys.begin(), keys.end());
        for (size_t i = 0; i < n; ++i) out[i] = land[keys[i].second];
    }
    return order;
}

// the rows of a settled pass: from the device into the pinned landing area
static int life_land(ctk_handle *h, size_t n, ctk_life_row **land)
{
    CTKCHK(ensure_host(h, h->h_cand, std::max<size_t>(n, 1) * sizeof(ctk_life_row), true));     // pinned landing area
    *land = (ctk_life_row *)h->h_cand.p;
    if (n) HIPCHK(hipMemcpy(*land, h->lc_rows.p, n * sizeof(ctk_life_row), hipMemcpyDeviceToHost));
    return CTK_OK;
}

static int life_check_shape(int64_t T, int ny, int nx)
{
    if (ny > 65535 || nx > 65535 || T > 4000000) return ctk_set_error(CTK_E_RANGE, "ctk_lifecycle: grid %d x %d x %lld beyond the supported size", ny, nx, (long long)T);
    return CTK_OK;
}

// a call begins: nothing of the last one is left to ask for
static void life_reset(ctk_handle *h, int64_t T)
{
    h->lc_host.clear();
    h->lc_path_T = -1;
    h->lc_plan = CtkLifePlan{0, 0, 0, 0, 0};
    h->lc_given_up = 0; h->lc_fb_launches = 0; h->lc_attempts = 0; h->lc_sort = 0;
    h->lc_rounds.assign((size_t)T, 0);
    h->lc_streamed = false;
    h->lx_idx.clear(); h->lx_rec.clear();
}

// own: where the slabs live (ctk_handle::lc_own); the host-array entry passes 1 or 2 after its uploads
static int lifecycle_dev_impl(ctk_handle *h, const int32_t *flag_dev, const void *field_dev, bool f64, int64_t T, int ny, int nx, const float *wrow,
                              int64_t *nrows, int own = 0)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (T < 0 || ny < 1 || nx < 1 || !wrow || (T > 0 && (!flag_dev || !field_dev)))
        return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle: bad shape or null pointer");
    CTKCHK(life_check_shape(T, ny, nx));
    HIPCHK(hipSetDevice(h->device));
    life_reset(h, T);
    if (nrows) *nrows = 0;
    if (T == 0) { h->lc_path_T = 0; return CTK_OK; }
    LifeRun r;
    r.flag = flag_dev; r.field = field_dev; r.f64 = f64; r.T = T; r.ny = ny; r.nx = nx;
    CTKCHK(life_weights(h, wrow, ny, nx, &r.wshift, &r.limb_bits));
    r.plan = ctk_life_plan(T, ny, nx, f64, (uintptr_t)flag_dev, (uintptr_t)field_dev);
    h->lc_plan = r.plan;
    r.cap = std::max<size_t>(h->lc_rows.cap / sizeof(CtkLifeRowDev), (size_t)T * 16 + 1024);
    h->lc_flag = flag_dev; h->lc_field = field_dev; h->lc_f64 = f64; h->lc_T = T; h->lc_ny = ny; h->lc_nx = nx;
    h->lc_own = own; h->lc_io_gen = h->io_gen; h->lc_an_gen = h->an_slab.gen;
    int rc = life_launch(h, r);
    if (rc == CTK_OK) rc = life_settle(h, r);
    h->lc_attempts = r.attempts; h->lc_given_up = r.given_up; h->lc_fb_launches = r.fb_launches;
    CTKCHK(rc);
    const size_t n = (size_t)r.cnt[0];
    ctk_life_row *land = nullptr;
    CTKCHK(life_land(h, n, &land));
    h->lc_sort = life_sort(h, land, n, T, h->lc_host);
    if (nrows) *nrows = (int64_t)n;
    h->lc_path_T = T;
    return CTK_OK;
}

// test hook, GPU-free: ctk_life_plan for slabs whose device addresses are flag_align / field_align bytes past a 32-byte boundary
extern "C" int ctk_debug_lifecycle_plan(int64_t T, int ny, int nx, int f64, int64_t flag_align, int64_t field_align, int64_t *out5)
{
    if (!out5 || T < 1 || ny < 1 || nx < 1 || flag_align < 0 || field_align < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_lifecycle_plan: bad arguments");
    const CtkLifePlan p = ctk_life_plan(T, ny, nx, f64 != 0, (uintptr_t)flag_align, (uintptr_t)field_align);
    out5[0] = p.rw; out5[1] = p.nsx; out5[2] = p.nby; out5[3] = p.vec; out5[4] = p.ks;
    return CTK_OK;
}

// test hook: the path of the last ctk_lifecycle_* call on this handle
extern "C" int ctk_debug_lifecycle_path(ctk_handle *h, int64_t *out8, uint8_t *steps, int64_t T)
{
    if (!h || !out8 || (T > 0 && !steps)) return ctk_set_error(CTK_E_INVALID, "ctk_debug_lifecycle_path: null argument");
    if (h->lc_path_T < 0) return ctk_set_error(CTK_E_STATE, "ctk_debug_lifecycle_path needs a finished ctk_lifecycle_* call first");
    if (T != h->lc_path_T) return ctk_set_error(CTK_E_INVALID, "ctk_debug_lifecycle_path: %lld time steps asked for, the last call had %lld", (long long)T, (long long)h->lc_path_T);
    out8[0] = h->lc_plan.rw; out8[1] = h->lc_plan.nsx; out8[2] = h->lc_plan.nby; out8[3] = h->lc_plan.vec;
    out8[4] = h->lc_given_up; out8[5] = h->lc_fb_launches; out8[6] = h->lc_attempts; out8[7] = h->lc_sort;
    if (T > 0) memcpy(steps, h->lc_rounds.data(), (size_t)T);
    return CTK_OK;
}

static int lifecycle_host_impl(ctk_handle *h, const int32_t *flag, const void *field, bool f64, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    if (T < 0 || ny < 1 || nx < 1 || (T > 0 && !flag)) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle: bad shape or null pointer");
    // field == NULL: the anomaly slab that ctk_anom_* left resident (no second trip over PCIe for it)
    if (T > 0 && !field && !h->an_slab.find(T, ny, nx, f64))
        return ctk_set_error(CTK_E_STATE, "ctk_lifecycle: field = NULL needs a resident anomaly slab of this shape and type (ctk_anom_* with keep_resident)");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)T * ny * nx, esz = f64 ? 8 : 4;
    void *f_dev = nullptr, *v_dev = nullptr;
    if (n) {
        CTKCHK(claim_io(h, h->io_out, n * 4));                     // the flag slab (the tracker's own result buffer, if it ran here)
        f_dev = h->io_out.p;
        HIPCHK(hipMemcpy(f_dev, flag, n * 4, hipMemcpyHostToDevice));
        if (field) {
            CTKCHK(claim_io(h, h->io_in, n * esz));
            v_dev = h->io_in.p;
            HIPCHK(hipMemcpy(v_dev, field, n * esz, hipMemcpyHostToDevice));
        } else v_dev = h->an_slab.buf.p;
    }
    return lifecycle_dev_impl(h, (const int32_t *)f_dev, v_dev, f64, T, ny, nx, wrow, nrows, field ? 1 : 2);
}

extern "C" int ctk_lifecycle_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *field_dev, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows)
{
    return lifecycle_dev_impl(h, flag_dev, field_dev, false, T, ny, nx, wrow, nrows);
}
extern "C" int ctk_lifecycle_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *field_dev, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows)
{
    return lifecycle_dev_impl(h, flag_dev, field_dev, true, T, ny, nx, wrow, nrows);
}
extern "C" int ctk_lifecycle_f32(ctk_handle *h, const int32_t *flag, const float *field, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows)
{
    return lifecycle_host_impl(h, flag, field, false, T, ny, nx, wrow, nrows);
}
extern "C" int ctk_lifecycle_f64(ctk_handle *h, const int32_t *flag, const double *field, int64_t T, int ny, int nx, const float *wrow, int64_t *nrows)
{
    return lifecycle_host_impl(h, flag, field, true, T, ny, nx, wrow, nrows);
}
static int life_exact_keys(ctk_handle *h, const int32_t *flag_dev, const void *field_dev, bool f64, int ny, int nx, const std::vector<CtkLifeKey> &keys,
                           ctk_life_exact *out);
// the listed rows (indices into the sorted rows of the last ctk_lifecycle_* call) re-evaluated in the reference's own summation orders
extern "C" int ctk_lifecycle_exact(ctk_handle *h, const int64_t *row_idx, int64_t n, ctk_life_exact *out)
{
    if (!h || n < 0 || (n > 0 && (!row_idx || !out))) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_exact: bad arguments");
    if (n == 0) return CTK_OK;
    if (h->lc_streamed) return ctk_set_error(CTK_E_STATE, "ctk_lifecycle_exact: the last call was streamed, its slabs are gone (ctk_lifecycle_stream_exact holds the rows it picked)");
    if (h->lc_own && (h->lc_io_gen != h->io_gen || (h->lc_own == 2 && h->lc_an_gen != h->an_slab.gen)))
        return ctk_set_error(CTK_E_STATE, "ctk_lifecycle_exact: a later call on this handle overwrote or released the slabs of the last ctk_lifecycle_* call; run it again first");
    if (!h->lc_flag || !h->lc_field) return ctk_set_error(CTK_E_STATE, "ctk_lifecycle_exact needs a ctk_lifecycle_* call first");
    HIPCHK(hipSetDevice(h->device));
    std::vector<CtkLifeKey> keys((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (row_idx[i] < 0 || (size_t)row_idx[i] >= h->lc_host.size()) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_exact: row %lld out of range", (long long)row_idx[i]);
        const ctk_life_row &r = h->lc_host[(size_t)row_idx[i]];
        keys[(size_t)i] = CtkLifeKey{r.t, r.label, r.shift, r.pad};
    }
    return life_exact_keys(h, h->lc_flag, h->lc_field, h->lc_f64, h->lc_ny, h->lc_nx, keys, out);
}

// keys[i]: (t, label, shift, row extent) of a row of the slab at flag_dev / field_dev, t counted from the slab's first plane
static int life_exact_keys(ctk_handle *h, const int32_t *flag_dev, const void *field_dev, bool f64, int ny, int nx, const std::vector<CtkLifeKey> &keys,
                           ctk_life_exact *out)
{
    static_assert(sizeof(ctk_life_exact) == sizeof(CtkLifeExact), "row layouts must agree");
    const int64_t n = (int64_t)keys.size();
    hipStream_t s = h->stream;
    CTKCHK(ensure(h, h->lc_ekeys, (size_t)n * sizeof(CtkLifeKey)));
    CTKCHK(ensure(h, h->lc_offs, (size_t)n * 16));                           // pixel offsets, row-table offsets
    CTKCHK(ensure(h, h->lc_out, (size_t)(n + 1) * sizeof(CtkLifeExact) + (size_t)n * 4));      // the rows | the kernel's failure word | the pixel counts
    // row tables: three words per row of every contour's row extent (the keys know the extents)
    std::vector<uint64_t> offs((size_t)2 * n);
    uint64_t rtotal = 0;
    int max_rows = 1;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t pad = (uint32_t)keys[(size_t)i].pad;
        const int ya = (int)(pad & 0xffffu), yb = std::min(ny - 1, (int)(pad >> 16));
        if (yb < ya) return ctk_set_error(CTK_E_INTERNAL, "ctk_lifecycle_exact: row %lld of the list has no row extent", (long long)i);
        offs[(size_t)(n + i)] = rtotal; rtotal += 3 * (uint64_t)(yb - ya + 1);
        max_rows = std::max(max_rows, yb - ya + 1);
    }
    CTKCHK(ensure(h, h->lc_sp, (size_t)std::max<uint64_t>(rtotal, 1) * 4));
    HIPCHK(hipMemcpyAsync(h->lc_ekeys.p, keys.data(), (size_t)n * sizeof(CtkLifeKey), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(P<uint64_t>(h->lc_offs) + n, offs.data() + n, (size_t)n * 8, hipMemcpyHostToDevice, s));
    uint32_t *d_fail = reinterpret_cast<uint32_t *>(P<CtkLifeExact>(h->lc_out) + n);
    uint32_t *d_counts = d_fail + sizeof(CtkLifeExact) / 4;
    const dim3 rgrid((unsigned)n, (unsigned)((max_rows + 3) / 4));           // (x: the listed row, y: four rows of its row extent)
    k_life_rows<<<rgrid, 256, 0, s>>>(flag_dev, P<CtkLifeKey>(h->lc_ekeys), P<uint64_t>(h->lc_offs) + n, ny, nx, P<uint32_t>(h->lc_sp));
    k_life_rowscan<<<(unsigned)n, 256, 0, s>>>(P<CtkLifeKey>(h->lc_ekeys), P<uint64_t>(h->lc_offs) + n, ny, P<uint32_t>(h->lc_sp), d_counts);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> counts((size_t)n);
    HIPCHK(hipMemcpyAsync(counts.data(), d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t total = 0;
    uint32_t max_count = 0;
    for (int64_t i = 0; i < n; ++i) { offs[(size_t)i] = total; total += counts[(size_t)i]; max_count = std::max(max_count, counts[(size_t)i]); }
    const int lx_threads = max_count > 8192 ? 1024 : 256;      // (large contours: four groups of the pairwise sums, four feeder waves)
    const size_t px = (size_t)std::max<uint64_t>(total, 1) * 8;
    CTKCHK(ensure(h, h->lc_sw, 5 * px));                                      // sw | sp | sq | sqy | sqx
    HIPCHK(hipMemcpyAsync(h->lc_offs.p, offs.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_fail, 0, 4, s));
    double *d_sw = P<double>(h->lc_sw);
    const size_t st = px / 8;
    if (f64)
        k_life_lists<double><<<rgrid, 256, 0, s>>>(flag_dev, (const double *)field_dev, P<float>(h->lc_w), P<CtkLifeKey>(h->lc_ekeys), P<uint64_t>(h->lc_offs), P<uint64_t>(h->lc_offs) + n,
                                                   ny, nx, d_sw, d_sw + st, d_sw + 2 * st, d_sw + 3 * st, d_sw + 4 * st, P<uint32_t>(h->lc_sp));
    else
        k_life_lists<float><<<rgrid, 256, 0, s>>>(flag_dev, (const float *)field_dev, P<float>(h->lc_w), P<CtkLifeKey>(h->lc_ekeys), P<uint64_t>(h->lc_offs), P<uint64_t>(h->lc_offs) + n,
                                                  ny, nx, d_sw, d_sw + st, d_sw + 2 * st, d_sw + 3 * st, d_sw + 4 * st, P<uint32_t>(h->lc_sp));
#define CTK_LX_LAUNCH(G)                                                                                                                                   \
    k_life_exact<G><<<(unsigned)n, 256 * G, 0, s>>>(P<uint64_t>(h->lc_offs), d_counts, d_sw, d_sw + st, d_sw + 2 * st, d_sw + 3 * st, d_sw + 4 * st,         \
                                                    P<CtkLifeExact>(h->lc_out), d_fail)
    if (lx_threads == 1024) CTK_LX_LAUNCH(4); else CTK_LX_LAUNCH(1);
#undef CTK_LX_LAUNCH
    HIPCHK(hipGetLastError());
    uint32_t failed = 0;
    HIPCHK(hipMemcpyAsync(out, h->lc_out.p, (size_t)n * sizeof(CtkLifeExact), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&failed, d_fail, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (failed) return ctk_set_error(CTK_E_INTERNAL, "ctk_lifecycle_exact: a wait between the waves of k_life_exact expired");
    return CTK_OK;
}

extern "C" int ctk_lifecycle_rows(ctk_handle *h, ctk_life_row *rows, int64_t cap)
{
    if (!h || (cap > 0 && !rows)) return ctk_set_error(CTK_E_INVALID, "null argument");
    if ((size_t)cap < h->lc_host.size()) return ctk_set_error(CTK_E_INVALID, "ctk_lifecycle_rows: room for %lld rows, %zu held", (long long)cap, h->lc_host.size());
    if (!h->lc_host.empty()) memcpy(rows, h->lc_host.data(), h->lc_host.size() * sizeof(ctk_life_row));
    return CTK_OK;
}

#include "ctk_sharded.hip"
#include "ctk_anom.hip"
#include "ctk_anom_seg.hip"
#include "ctk_freq.hip"
#include "ctk_spell.hip"
#include "ctk_life_stream.hip"
#include "ctk_pctl.hip"
#include "ctk_pfield.hip"
#include "ctk_std.hip"
#include "ctk_level.hip"
#include "ctk_filter.hip"
#include "ctk_reversal.hip"
#include "ctk_lwa.hip"
#include "ctk_subset.hip"
#include "ctk_composite.hip"
#include "ctk_blockstat.hip"
#include "ctk_centred.hip"
#include "ctk_band.hip"

// device-memory helpers for a ctypes host
// ------------------------------------------------------------------------------------------------
extern "C" int ctk_dev_malloc(ctk_handle *h, void **p, size_t nbytes)
{
    if (!h || !p) return ctk_set_error(CTK_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = hipMalloc(p, nbytes ? nbytes : 8);
    if (e != hipSuccess) { *p = nullptr; return ctk_set_error(CTK_E_NOMEM, "hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e)); }
    return CTK_OK;
}
// Result buffers for the host-array entries without first-touch page faults: pinned, CPU-cacheable host memory owned by the caller
// (ctk_host_alloc / ctk_host_free) or a caller array registered once (ctk_host_register / ctk_host_unregister).  ctk_track_f32 /
// _f64 / ctk_track_resident recognise such a `flag` pointer and copy the result into it with ONE DMA (no bounce buffers).
extern "C" int ctk_host_alloc(ctk_handle *h, void **p, size_t nbytes)
{
    if (!h || !p) return ctk_set_error(CTK_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = hipHostMalloc(p, nbytes ? nbytes : 8, hipHostMallocNonCoherent);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return ctk_set_error(CTK_E_NOMEM, "hipHostMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e)); }
    return CTK_OK;
}
extern "C" int ctk_host_free(ctk_handle *h, void *p)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (p) HIPCHK(hipHostFree(p));
    return CTK_OK;
}
extern "C" int ctk_host_register(ctk_handle *h, void *p, size_t nbytes)
{
    if (!h || !p || !nbytes) return ctk_set_error(CTK_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipError_t e = hipHostRegister(p, nbytes, hipHostRegisterDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); return ctk_set_error(CTK_E_NOMEM, "hipHostRegister(%zu bytes) failed: %s", nbytes, hipGetErrorString(e)); }
    return CTK_OK;
}
extern "C" int ctk_host_unregister(ctk_handle *h, void *p)
{
    if (!h || !p) return ctk_set_error(CTK_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipHostUnregister(p));
    return CTK_OK;
}
// is [p, p + n) pinned / registered host memory the device can write directly?
static bool host_is_pinned(const void *p, size_t n)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (at.type != hipMemoryTypeHost) return false;
    hipPointerAttribute_t at2;
    memset(&at2, 0, sizeof(at2));
    if (n > 1 && hipPointerGetAttributes(&at2, (const char *)p + n - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
    return n <= 1 || at2.type == hipMemoryTypeHost;
}

extern "C" int ctk_dev_free(ctk_handle *h, void *p)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (p) HIPCHK(hipFree(p));
    return CTK_OK;
}
extern "C" int ctk_memcpy_h2d(ctk_handle *h, void *dst_dev, const void *src, size_t nbytes)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(dst_dev, src, nbytes, hipMemcpyHostToDevice));
    return CTK_OK;
}
extern "C" int ctk_memcpy_d2h(ctk_handle *h, void *dst, const void *src_dev, size_t nbytes)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(dst, src_dev, nbytes, hipMemcpyDeviceToHost));
    return CTK_OK;
}
extern "C" int ctk_sync(ctk_handle *h)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipDeviceSynchronize());
    return CTK_OK;
}
extern "C" void *ctk_stream(ctk_handle *h) { return h ? (void *)h->stream : nullptr; }
extern "C" int ctk_device_of(ctk_handle *h) { return h ? h->device : -1; }

extern "C" int ctk_synth_fill_window(ctk_handle *h, float *anom_dev, int64_t t0, int64_t T, int ny, int nx, uint64_t seed);
extern "C" int ctk_synth_fill(ctk_handle *h, float *anom_dev, int64_t T, int ny, int nx, uint64_t seed)
{
    return ctk_synth_fill_window(h, anom_dev, 0, T, ny, nx, seed);
}

extern "C" int ctk_checksum_i32_dev(ctk_handle *h, const int32_t *p_dev, int64_t n, int64_t index0, uint64_t *out2)
{
    if (!h || !out2 || n < 0 || (n > 0 && !p_dev)) return ctk_set_error(CTK_E_INVALID, "ctk_checksum_i32_dev: null argument or negative size");
    HIPCHK(hipSetDevice(h->device));
    CTKCHK(ensure(h, h->dbg, 16));
    HIPCHK(hipMemsetAsync(h->dbg.p, 0, 16, h->stream));
    if (n > 0) {
        k_checksum_i32<<<(int)std::min<int64_t>((n + 255) / 256, 8192), 256, 0, h->stream>>>(p_dev, n, index0, (unsigned long long *)h->dbg.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out2, h->dbg.p, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_dev_memset(ctk_handle *h, void *p_dev, int byte, size_t nbytes)
{
    if (!h || (nbytes && !p_dev)) return ctk_set_error(CTK_E_INVALID, "ctk_dev_memset: null argument");
    HIPCHK(hipSetDevice(h->device));
    if (nbytes) HIPCHK(hipMemsetAsync(p_dev, byte, nbytes, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

/* measurement support: best-of-`reps` time of a plain 16-byte non-temporal store (mode 1: chunks in launch order, mode 2: one contiguous
 * eighth of the buffer per XCD) / load (mode 0) stream over [p_dev, p_dev + nbytes) */
extern "C" int ctk_debug_stream_ceiling(ctk_handle *h, void *p_dev, size_t nbytes, int mode, int reps, double *best_ms)
{
    if (!h || !p_dev || !best_ms || nbytes < 16 || (((uintptr_t)p_dev) & 15) || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_stream_ceiling: bad argument");
    HIPCHK(hipSetDevice(h->device));
    CTKCHK(ensure(h, h->dbg, 64));
    Event e0, e1;
    HIPCHK(e0.create());
    if (e1.create() != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed");
    const int64_t n16 = (int64_t)(nbytes / 16);
    const unsigned grid = (unsigned)((n16 + 2047) / 2048);
    double best = 1e30;
    hipError_t err = hipSuccess;
    for (int r = 0; r < reps + 1 && err == hipSuccess; r++) {          // (+ 1: the first launch is not counted)
        err = hipEventRecord(e0, h->stream);
        if (mode) k_stream_store<<<grid, 256, 0, h->stream>>>((i32x4 *)p_dev, n16, mode == 2 ? 1 : 0);
        else k_stream_load<<<grid, 256, 0, h->stream>>>((const i32x4 *)p_dev, n16, P<int32_t>(h->dbg));
        if (err == hipSuccess) err = hipEventRecord(e1, h->stream);
        if (err == hipSuccess) err = hipEventSynchronize(e1);
        float f = 0.f;
        if (err == hipSuccess) err = hipEventElapsedTime(&f, e0, e1);
        if (r > 0 && f < best) best = f;
    }
    if (err != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "ctk_debug_stream_ceiling: %s", hipGetErrorString(err));
    *best_ms = best;
    return CTK_OK;
}

extern "C" int ctk_check_flag_dev(ctk_handle *h, const float *anom_dev, const int32_t *flag_dev, int64_t T, int ny, int nx, const double *thr, int cmp_op,
                                  int persistence, int64_t max_id, uint64_t *out6)
{
    if (!h || !out6 || T < 0 || ny < 1 || nx < 1 || max_id < 0 || max_id > 0x7ffffffell || cmp_op < 0 || cmp_op > 3 || (T > 0 && (!anom_dev || !flag_dev || !thr)))
        return ctk_set_error(CTK_E_INVALID, "ctk_check_flag_dev: bad argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t tab = (size_t)(max_id + 1) * 4;
    DevBuf tab_buf, thr_buf;                                                    // (freed thresholds first)
    HIPCHK(thr_buf.alloc((size_t)std::max<int64_t>(T, 1) * 8));
    HIPCHK(tab_buf.alloc(2 * tab));
    void *const d_thr = thr_buf.p, *const d_tab = tab_buf.p;
    CTKCHK(ensure(h, h->dbg, 64));
    HIPCHK(hipMemsetAsync(h->dbg.p, 0, 48, s));
    if (T > 0) HIPCHK(hipMemcpyAsync(d_thr, thr, (size_t)T * 8, hipMemcpyHostToDevice, s));
    int32_t *tmin = (int32_t *)d_tab, *tmax = tmin + (max_id + 1);
    k_fill_minmax<<<(int)std::min<int64_t>((max_id + 256) / 256, 4096), 256, 0, s>>>(tmin, tmax, max_id + 1);
    const int64_t nrows = T * ny;
    if (nrows > 0) {
        const int g = (int)std::min<int64_t>((nrows + 3) / 4, 1 << 16);
        unsigned long long *o = (unsigned long long *)h->dbg.p;
        switch (cmp_op) {
        case 0: k_check_flag<0><<<g, 256, 0, s>>>(anom_dev, flag_dev, nrows, ny, nx, (const double *)d_thr, max_id, tmin, tmax, o); break;
        case 1: k_check_flag<1><<<g, 256, 0, s>>>(anom_dev, flag_dev, nrows, ny, nx, (const double *)d_thr, max_id, tmin, tmax, o); break;
        case 2: k_check_flag<2><<<g, 256, 0, s>>>(anom_dev, flag_dev, nrows, ny, nx, (const double *)d_thr, max_id, tmin, tmax, o); break;
        default: k_check_flag<3><<<g, 256, 0, s>>>(anom_dev, flag_dev, nrows, ny, nx, (const double *)d_thr, max_id, tmin, tmax, o); break;
        }
    }
    k_check_ids<<<(int)std::min<int64_t>((max_id + 256) / 256, 4096), 256, 0, s>>>(tmin, tmax, max_id, persistence, (unsigned long long *)h->dbg.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out6, h->dbg.p, 48, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CTK_OK;
}

extern "C" int ctk_synth_fill_window(ctk_handle *h, float *anom_dev, int64_t t0, int64_t T, int ny, int nx, uint64_t seed)
{
    if (!h || !anom_dev || t0 < 0) return ctk_set_error(CTK_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n = T * (int64_t)ny * nx;
    if (n > 0) {
        const int64_t blocks = std::min<int64_t>((n + 255) / 256, 1 << 20);      // grid-stride beyond 2^28 pixels
        k_synth<<<(int)blocks, 256, 0, h->stream>>>(anom_dev, T, ny, nx, seed, t0);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}
