// ctk_level.hip -- the first step of the reference README's third recipe on the device (included by ctk_api.hip):
//     "The PV fields are vertically averaged between 500-150 hPa"                                              README.rst:235-240
// on a (steps, nlev, ny, nx) field with one float64 weight per level (include/contrack_hip.h states the arithmetic; the reference
// has no function for this step, tests/level_util.py is its numpy statement):
//     out[s][p] = dtype( (sum over the selected levels l in rising order of w[l] * x[s][l][p]) / (sum of those w[l]) )
// in float64, the multiply and the add rounded separately.  A level of weight 0 is not selected: never read, never uploaded.
//
// k_level_mean: one thread per 16 bytes of adjacent pixels of one step (4 float32 / 2 float64) walks the selected levels.  A level
// plane is contiguous, so a wave reads 1 KB per plane with one nontemporal 16-byte load per lane (the input is read once); the result
// leaves with a plain 16-byte store (the next stage reads it).  Level indices and weights are the same for the whole grid: they
// lie in a small device table read through the constant address space (scalar loads).  The loads of CTK_LEVEL_UNROLL planes of a
// lane are issued before the first is used, the rest of the levels in batches of 4, 2 and 1: the kernel has almost no arithmetic,
// so loads in flight are all that keeps it busy.  The scalar form (a plane that does not start on a 16-byte boundary: odd sizes, an
// offset pointer) is the same loop with one pixel per thread.  A workgroup stays inside one step (ctk_level_plan, ctk_forms.h).
// The store is an eighth of the traffic or more, and what bounds the kernel is that write stream among the reads: without its store
// it runs at 0.96 of a plain load stream, with it at 0.67-0.72 of the stream charged for the store, whatever the arithmetic
// (profiles/NOTES.md).  Large launches give every XCD one contiguous eighth of the workgroups (xcd_chunk): 4-13 % on four boards.
//
// Host-array entries: only the selected levels cross PCIe.  Neighbouring selected levels travel as one strided copy per chunk (pitch
// nlev planes, width `len` planes, one row per step; ctk_level_runs), the device chunk is compact (nt, nsel, ny, nx).  Two input and
// two output chunks on the handle's copy stream, events and pinned buffers: chunk k + 1 travels in while the kernel reduces chunk k
// and chunk k - 1 leaves (stream_produce, ctk_api.hip).
#pragma once

typedef const __attribute__((address_space(4))) double ctk_const_f64;
typedef float ctk_f32x4 __attribute__((ext_vector_type(4)));
typedef double ctk_f64x2 __attribute__((ext_vector_type(2)));

// what a lane holds of one level plane: VEC 16 bytes (N pixels), else one pixel
template <typename VT, bool VEC> struct LevelLane {
    typedef VT type;
    static constexpr int N = 1;
    static __device__ __forceinline__ type load(const VT *a) { return *a; }
    static __device__ __forceinline__ double get(const type &v, int) { return (double)v; }
    static __device__ __forceinline__ void set(type &v, int, VT r) { v = r; }
};
template <> struct LevelLane<float, true> {
    typedef ctk_f32x4 type;
    static constexpr int N = 4;
    static __device__ __forceinline__ type load(const float *a) { return __builtin_nontemporal_load((const type *)a); }
    static __device__ __forceinline__ double get(const type &v, int i) { return (double)v[i]; }
    static __device__ __forceinline__ void set(type &v, int i, float r) { v[i] = r; }
};
template <> struct LevelLane<double, true> {
    typedef ctk_f64x2 type;
    static constexpr int N = 2;
    static __device__ __forceinline__ type load(const double *a) { return __builtin_nontemporal_load((const type *)a); }
    static __device__ __forceinline__ double get(const type &v, int i) { return v[i]; }
    static __device__ __forceinline__ void set(type &v, int i, double r) { v[i] = r; }
};

// levels k .. k + U - 1 of the table: all U loads first, then the sums in rising k (xs: the lane's pixels on level 0 of its step)
template <typename VT, bool VEC, bool SKIPNA, int U>
__device__ __forceinline__ void level_batch(const VT *__restrict__ xs, int64_t npix, ctk_const_f64 *w, ctk_const_i32 *lev, int k, double *acc, double *ws)
{
#pragma clang fp contract(off)
    typedef LevelLane<VT, VEC> L;
    typename L::type v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = L::load(xs + (int64_t)lev[k + u] * npix);
#pragma unroll
    for (int u = 0; u < U; u++) {
        const double wk = w[k + u];
#pragma unroll
        for (int i = 0; i < L::N; i++) {
            const double xv = L::get(v[u], i);
            const double prod = wk * xv;                                         // (a rounded multiply, then a rounded add)
            if (SKIPNA) {
                if (xv == xv) { acc[i] = acc[i] + prod; ws[i] = ws[i] + wk; }
            } else {
                acc[i] = acc[i] + prod;
            }
        }
    }
}

// x: (steps, nlev, npix); level lev[k] of every step has weight w[k], k < nsel; wsum: w[0] + w[1] + ... in that order.  Workgroup b of
// `blocks` = bps * steps takes part b % bps of the plane of step b / bps.
template <typename VT, bool VEC, bool SKIPNA>
__global__ __launch_bounds__(CTK_LEVEL_THREADS) void k_level_mean(const VT *__restrict__ x, int64_t nlev, int64_t npix, int64_t bps, int64_t blocks, int nsel,
                                                                  const double *__restrict__ w_ptr, const int32_t *__restrict__ lev_ptr, double wsum,
                                                                  VT *__restrict__ out, int xcd)
{
    typedef LevelLane<VT, VEC> L;
    ctk_const_f64 *w = (ctk_const_f64 *)w_ptr;
    ctk_const_i32 *lev = (ctk_const_i32 *)lev_ptr;
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b < blocks; b += gridDim.x) {       // (a permutation of the launch's workgroups)
        const int64_t s = b / bps;
        const int64_t p0 = ((b - s * bps) * CTK_LEVEL_THREADS + threadIdx.x) * L::N;      // first pixel of this lane (64-bit throughout)
        if (p0 >= npix) continue;
        const VT *xs = x + s * nlev * npix + p0;
        double acc[L::N], ws[L::N];
#pragma unroll
        for (int i = 0; i < L::N; i++) { acc[i] = 0.0; ws[i] = 0.0; }
        int k = 0;
        for (; k + CTK_LEVEL_UNROLL <= nsel; k += CTK_LEVEL_UNROLL) level_batch<VT, VEC, SKIPNA, CTK_LEVEL_UNROLL>(xs, npix, w, lev, k, acc, ws);
        if (nsel - k >= 4) { level_batch<VT, VEC, SKIPNA, 4>(xs, npix, w, lev, k, acc, ws); k += 4; }
        if (nsel - k >= 2) { level_batch<VT, VEC, SKIPNA, 2>(xs, npix, w, lev, k, acc, ws); k += 2; }
        if (nsel - k >= 1) level_batch<VT, VEC, SKIPNA, 1>(xs, npix, w, lev, k, acc, ws);
        typename L::type r;
#pragma unroll
        for (int i = 0; i < L::N; i++) L::set(r, i, (VT)(acc[i] / (SKIPNA ? ws[i] : wsum)));      // float64 divide, one rounding to VT
        *(typename L::type *)(out + s * npix + p0) = r;
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the selected levels of a call: indices, weights, their sum in rising order, the runs of neighbours
struct LevelSel {
    std::vector<int32_t> lev;
    std::vector<double> w;
    std::vector<CtkLevelRun> runs;
    double wsum = 0.0;
};

// checks the n weights (each finite and >= 0, one > 0, at most CTK_LEVEL_MAX_SEL selected) and lists the selected levels
static int level_select(const char *who, const double *weights, int64_t n, LevelSel &sel)
{
    for (int64_t l = 0; l < n; l++)
        if (!(weights[l] >= 0.0) || !std::isfinite(weights[l]))
            return ctk_set_error(CTK_E_INVALID, "%s: weights[%lld] = %g (each weight must be finite and >= 0)", who, (long long)l, weights[l]);
    sel.runs.resize((size_t)(n + 1) / 2 + 1);
    int64_t nsel = 0;
    const int64_t nr = ctk_level_runs(weights, n, sel.runs.data(), &nsel);
    sel.runs.resize((size_t)nr);
    if (nsel < 1) return ctk_set_error(CTK_E_INVALID, "%s: all %lld weights are zero", who, (long long)n);
    if (nsel > CTK_LEVEL_MAX_SEL) return ctk_set_error(CTK_E_INVALID, "%s: %lld selected levels (at most %d)", who, (long long)nsel, CTK_LEVEL_MAX_SEL);
    sel.wsum = 0.0;
    for (const CtkLevelRun &r : sel.runs)
        for (int64_t l = r.l0; l < r.l0 + r.len; l++) { sel.lev.push_back((int32_t)l); sel.w.push_back(weights[l]); sel.wsum = sel.wsum + weights[l]; }
    return CTK_OK;
}

// the device table of a call: nsel weights, then nsel level indices (`compact`: the chunk holds the selected levels only, level k at k)
static int level_table(ctk_handle *h, const LevelSel &sel, bool compact, const double **w_dev, const int32_t **lev_dev)
{
    const size_t K = sel.w.size();
    CTKCHK(ensure(h, h->lv_tab, K * 12));
    std::vector<int32_t> lev(sel.lev);
    if (compact) for (size_t k = 0; k < K; k++) lev[k] = (int32_t)k;
    HIPCHK(hipMemcpy(h->lv_tab.p, sel.w.data(), K * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)h->lv_tab.p + K * 8, lev.data(), K * 4, hipMemcpyHostToDevice));
    *w_dev = (const double *)h->lv_tab.p;
    *lev_dev = (const int32_t *)((const char *)h->lv_tab.p + K * 8);
    return CTK_OK;
}

// out[s] = the mean of step s of x (steps, nlev, npix) over the table's levels, on the handle's stream
template <typename VT>
static int launch_level(ctk_handle *h, const VT *x, int64_t nlev, int64_t npix, int64_t steps, int nsel, const double *w_dev, const int32_t *lev_dev, double wsum,
                        int skipna, VT *out)
{
    const bool aligned = (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    const CtkLevelPlan pl = ctk_level_plan((int)sizeof(VT), nsel, npix, steps, aligned, h->lv_knobs.cap());
    h->lv_knobs.launched(pl.vec, pl.grid);
    const int xcd = h->lv_knobs.xcd(pl.xcd);
#define CTK_LEVEL_LAUNCH(V, S) k_level_mean<VT, V, S><<<pl.grid, CTK_LEVEL_THREADS, 0, h->stream>>>(x, nlev, npix, pl.bps, pl.blocks, nsel, w_dev, lev_dev, wsum, out, xcd)
    if (pl.vec) { if (skipna) CTK_LEVEL_LAUNCH(true, true); else CTK_LEVEL_LAUNCH(true, false); }
    else        { if (skipna) CTK_LEVEL_LAUNCH(false, true); else CTK_LEVEL_LAUNCH(false, false); }
#undef CTK_LEVEL_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

static int level_check(const char *who, const void *h, const void *x, int64_t steps, int64_t nlev, int ny, int nx, const double *weights)
{
    if (!h || !x || !weights || steps < 1 || nlev < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments (null pointer or a size below 1)", who);
    return CTK_OK;
}

template <typename VT>
static int level_dev_impl(ctk_handle *h, const VT *x_dev, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, VT *out_dev, const char *who)
{
    CTKCHK(level_check(who, h, x_dev, steps, nlev, ny, nx, weights));
    if (!out_dev) return ctk_set_error(CTK_E_INVALID, "%s: null output", who);
    LevelSel sel;
    CTKCHK(level_select(who, weights, nlev, sel));
    HIPCHK(hipSetDevice(h->device));
    h->lv_slab.gen++;                                                  // (the slab is not touched; every ctk_level_mean_* call changes the number, the header says)
    const double *w_dev = nullptr;
    const int32_t *lev_dev = nullptr;
    CTKCHK(level_table(h, sel, false, &w_dev, &lev_dev));
    CTKCHK(launch_level<VT>(h, x_dev, nlev, (int64_t)ny * nx, steps, (int)sel.w.size(), w_dev, lev_dev, sel.wsum, skipna, out_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_level_mean_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out_dev)
{
    return level_dev_impl<float>(h, x_dev, steps, nlev, ny, nx, weights, skipna, out_dev, "ctk_level_mean_f32_dev");
}
extern "C" int ctk_level_mean_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out_dev)
{
    return level_dev_impl<double>(h, x_dev, steps, nlev, ny, nx, weights, skipna, out_dev, "ctk_level_mean_f64_dev");
}

// weights: one per level of the source -- nlev of them for an array (zeros are not selected), the nsel non-zero ones for a reader
template <typename VT>
static int level_stream_impl(ctk_handle *h, StreamIO &io, int64_t steps, int64_t nlev, int ny, int nx, const double *weights, int skipna, int64_t chunk_steps,
                             int keep_resident, const char *name)
{
    CTKCHK(level_check(name, h, io.read ? (const void *)h : io.host_in, steps, nlev, ny, nx, weights));
    const bool sink = io.host_out_v || io.write_v;
    if (!sink && !keep_resident) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output and keep_resident = 0)", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", name, (long long)chunk_steps);
    LevelSel sel;
    CTKCHK(level_select(name, weights, nlev, sel));
    const int64_t K = (int64_t)sel.w.size();
    if (io.read && K != nlev) return ctk_set_error(CTK_E_INVALID, "%s: a reader delivers the selected levels only, %lld of its %lld weights are zero", name, (long long)(nlev - K), (long long)nlev);
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    const size_t plane = (size_t)npix * sizeof(VT);
    io.esz = sizeof(VT);
    io.chunk = ctk_stream_chunk(chunk_steps, steps, (size_t)K * plane);
    const double t_call = now_ms();
    h->lv_slab.drop();
    CTKCHK(stream_setup(h, (size_t)io.chunk * (size_t)K * plane, 0, io.read != nullptr));
    CTKCHK(produce_out_setup(h, io, h->lv_slab.buf, steps, plane, keep_resident));
    const double *w_dev = nullptr;
    const int32_t *lev_dev = nullptr;
    CTKCHK(level_table(h, sel, true, &w_dev, &lev_dev));
    // the chunks (stream_produce): io.host_in is the whole (steps, nlev, ny, nx) array (the runs pick its selected levels), io.read a
    // reader of compact chunks (nt, nsel, ny, nx).  The means go to io.host_out_v / io.write_v chunk by chunk and (keep) into lv_slab.
    Producer p;
    p.in_bytes = (size_t)io.chunk * (size_t)K * plane; p.out_step = plane;
    p.upload = [&](const ProduceIn &c) -> int {
        if (c.src || K == nlev) return upload_steps(h, io, c, (size_t)K * plane);
        for (const CtkLevelRun &r : sel.runs)                                   // row s of the copy: the run's planes of step c0 + s
            HIPCHK(hipMemcpy2DAsync(c.dev + (size_t)r.k0 * plane, (size_t)K * plane, (const char *)io.host_in + ((size_t)c.c0 * (size_t)nlev + (size_t)r.l0) * plane,
                                    (size_t)nlev * plane, (size_t)r.len * plane, (size_t)c.nt, hipMemcpyHostToDevice, h->copy_stream));
        return CTK_OK;
    };
    p.launch = [&](const ProduceIn &c, ProduceOut &o) -> int {
        o.t0 = c.c0; o.nt = c.nt;
        o.dev = produce_out_dev(h, io, h->lv_slab.buf, c, plane, keep_resident);
        return launch_level<VT>(h, (const VT *)c.dev, K, npix, c.nt, (int)K, w_dev, lev_dev, sel.wsum, skipna, (VT *)o.dev);
    };
    CTKCHK(stream_produce_end(h, io, stream_produce(h, io, steps, name, p), t_call));
    if (keep_resident) h->lv_slab.keep(steps, ny, nx, sizeof(VT) == 8);
    return CTK_OK;
}

template <typename VT>
static int level_host(ctk_handle *h, const VT *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, VT *out, int64_t chunk_steps,
                      int keep_resident, const char *name)
{
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return level_stream_impl<VT>(h, io, steps, nlev, ny, nx, weights, skipna, chunk_steps, keep_resident, name);
}

// (not streamed: the streamed form with the chunk plan of chunk_steps = 0 -- never steps x nlev planes of HBM)
extern "C" int ctk_level_mean_f32(ctk_handle *h, const float *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out, int keep_resident)
{
    return level_host<float>(h, x, steps, nlev, ny, nx, weights, skipna, out, 0, keep_resident, "ctk_level_mean_f32");
}
extern "C" int ctk_level_mean_f64(ctk_handle *h, const double *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out, int keep_resident)
{
    return level_host<double>(h, x, steps, nlev, ny, nx, weights, skipna, out, 0, keep_resident, "ctk_level_mean_f64");
}
extern "C" int ctk_level_mean_stream_f32(ctk_handle *h, const float *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, float *out,
                                         int64_t chunk_steps, int keep_resident)
{
    return level_host<float>(h, x, steps, nlev, ny, nx, weights, skipna, out, chunk_steps, keep_resident, "ctk_level_mean_stream_f32");
}
extern "C" int ctk_level_mean_stream_f64(ctk_handle *h, const double *x, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna, double *out,
                                         int64_t chunk_steps, int keep_resident)
{
    return level_host<double>(h, x, steps, nlev, ny, nx, weights, skipna, out, chunk_steps, keep_resident, "ctk_level_mean_stream_f64");
}
extern "C" int ctk_level_mean_stream_cb(ctk_handle *h, int elem_bytes, int64_t steps, int nsel, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user,
                                        const double *weights_sel, int skipna, ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps, int keep_resident)
{
    StreamIO io;
    CTKCHK(stream_cb_io("ctk_level_mean_stream_cb", h, elem_bytes, reader, reader_user, writer, writer_user, io));
    if (elem_bytes == 8) return level_stream_impl<double>(h, io, steps, nsel, ny, nx, weights_sel, skipna, chunk_steps, keep_resident, "ctk_level_mean_stream_cb");
    return level_stream_impl<float>(h, io, steps, nsel, ny, nx, weights_sel, skipna, chunk_steps, keep_resident, "ctk_level_mean_stream_cb");
}

// shape of the mean kept in HBM by the last ctk_level_mean_* call with keep_resident (steps = -1: none)
extern "C" int ctk_resident_level_mean(ctk_handle *h, int64_t *steps, int *ny, int *nx, int *is_f64)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->lv_slab.report(steps, ny, nx, is_f64);
    return CTK_OK;
}

// WHICH mean is resident: changes with every ctk_level_mean_* call and with ctk_release_io (as ctk_resident_anom_generation)
extern "C" int ctk_resident_level_mean_generation(ctk_handle *h, uint64_t *generation)
{
    if (!h || !generation) return ctk_set_error(CTK_E_INVALID, "null argument");
    *generation = h->lv_slab.gen;
    return CTK_OK;
}

// ctk_anom_seg_* with x taken from the resident mean
extern "C" int ctk_anom_seg_resident(ctk_handle *h, const int32_t *group, int ngroups, int window, int smooth, const void *clim_in, void *anom_out, void *clim_out,
                                     int keep_resident, const int64_t *starts, int64_t nseg)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "ctk_anom_seg_resident: null handle");
    const ResidentSlab &m = h->lv_slab;
    if (!m.held()) return ctk_set_error(CTK_E_INVALID, "ctk_anom_seg_resident: no vertical mean is resident (ctk_level_mean_* with keep_resident)");
    if (!anom_out && !clim_out && !keep_resident) return ctk_set_error(CTK_E_INVALID, "ctk_anom_seg_resident: bad arguments");
    CTKCHK(anom_seg_args("ctk_anom_seg_resident", h, m.T, m.ny, m.nx, group, ngroups, window, smooth, starts, nseg));
    if (m.f64)
        return anom_seg_dev<double>(h, (const double *)m.buf.p, m.T, m.ny, m.nx, group, ngroups, window, smooth, (const double *)clim_in, (double *)anom_out,
                                    (double *)clim_out, keep_resident, starts, nseg);
    return anom_seg_dev<float>(h, (const float *)m.buf.p, m.T, m.ny, m.nx, group, ngroups, window, smooth, (const float *)clim_in, (float *)anom_out,
                               (float *)clim_out, keep_resident, starts, nseg);
}

// what ctk_level_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_level_plan(int elem_bytes, int64_t nsel, int64_t npix, int64_t steps, int aligned, int64_t *out7)
{
    if (!out7 || (elem_bytes != 4 && elem_bytes != 8) || nsel < 1 || npix < 1 || steps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_level_plan: bad arguments");
    const CtkLevelPlan p = ctk_level_plan(elem_bytes, nsel, npix, steps, aligned != 0);
    out7[0] = p.vec; out7[1] = p.vpt; out7[2] = p.unroll; out7[3] = p.bps; out7[4] = p.blocks; out7[5] = p.grid; out7[6] = p.xcd;
    return CTK_OK;
}

// test hook: out2 = { the form of the last k_level_mean launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups }
extern "C" int ctk_debug_level_form(ctk_handle *h, int64_t *out2)
{
    return knobs_form(h, &ctk_handle::lv_knobs, out2);
}

// test hook / experiments (tools/level_probe.py) for the following k_level_mean launches on this handle: the xcd_chunk mode (0 launch
// order, 1 eighths, n > 1 tiles of n workgroups; -1: the rule of ctk_level_plan) and a lower cap on the workgroups of a launch, so that
// a small case walks the stride loop (0: CTK_LEVEL_GRID_MAX)
extern "C" int ctk_debug_set_level(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    return knobs_set("ctk_debug_set_level", h, &ctk_handle::lv_knobs, xcd_mode, grid_max);
}

// measurement (tools/level_probe.py): k_level_mean alone between HIP events on slabs in device memory -- one launch that is not counted,
// then `reps` timed ones; ms2 = {best, mean}
extern "C" int ctk_debug_time_level_mean(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int nlev, int ny, int nx, const double *weights, int skipna,
                                         void *out_dev, int reps, double *ms2)
{
    CTKCHK(level_check("ctk_debug_time_level_mean", h, x_dev, steps, nlev, ny, nx, weights));
    if (!out_dev || !ms2 || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_level_mean: bad arguments");
    LevelSel sel;
    CTKCHK(level_select("ctk_debug_time_level_mean", weights, nlev, sel));
    HIPCHK(hipSetDevice(h->device));
    const double *w_dev = nullptr;
    const int32_t *lev_dev = nullptr;
    CTKCHK(level_table(h, sel, false, &w_dev, &lev_dev));
    return time_launches(h, "ctk_debug_time_level_mean", reps, ms2, [&]() {
        return is_f64 ? launch_level<double>(h, (const double *)x_dev, nlev, (int64_t)ny * nx, steps, (int)sel.w.size(), w_dev, lev_dev, sel.wsum, skipna, (double *)out_dev)
                      : launch_level<float>(h, (const float *)x_dev, nlev, (int64_t)ny * nx, steps, (int)sel.w.size(), w_dev, lev_dev, sel.wsum, skipna, (float *)out_dev);
    });
}
