// ctk_composite.hip -- the composite that follows the reference tutorial's frequency map (README.rst:156-164), on the device (included
// by ctk_api.hip): the sum of a field over the time steps at which a grid point is flagged, per group of time steps (month, season ...
// -- or one group), and how many there were:
//     sum[g][p] = x[t0][p] + x[t1][p] + ...  over the t in rising order with group[t] == g and flag[t][p] > above   (float64, from +0.0)
//     n[g][p]   = how many                                                                                          (uint32)
// (with skipna a NaN value is not selected; the mean sum / n is left to the caller).  The reference has no function for it,
// tests/composite_util.py is its numpy statement.
//
// k_composite: one lane owns a pixel for ALL time steps of a launch.  Float64 addition is not associative, so T is never split over
// workgroups and nothing is added atomically: a pixel's values meet its sum in time order, which is what makes the result
// reproducible bit for bit.  Parallelism comes from the plane and from a batch of time steps whose loads are in flight together
// (ctk_composite_plan, ctk_forms.h: 16 steps per batch for a 1-degree plane, 8 for a quarter-degree one, which fills the chip by itself).
//
// The flags are one nontemporal stream.  The field is read UNDER the lane's flag test: the load of a step is issued only by lanes
// whose flag passed, and a wave none of whose 64 pixels passed skips it altogether, so with blocked pixels a few per cent and
// spatially coherent most cache lines of the field are never asked for; the price is one dependent trip per batch.  Measured
// against the two alternatives in the same process (profiles/NOTES.md): reading both slabs unconditionally is faster on a 1-degree
// plane, which cannot fill the chip (0.31 against 0.42 ms for 2707 steps) and slower on a quarter-degree plane (0.58 against 0.34 ms
// for 480 steps); the kernel's time grows with the plane, so the conditional read is the one form.  A form with 16 bytes of flags --
// 4 pixels -- per lane lost at both sizes (a wave then spans 256 pixels and skips far fewer field loads) and is not built.
//
// The accumulators, 12 bytes per (group, pixel), live in HBM; a lane keeps the current group's pair in registers.  It loads the pair
// at its first selected step inside a run of equal group ids and stores it at the end of that run (or of the launch) only if it
// selected something: with dayofyear groups the id changes at every step, and touching the accumulators unconditionally would triple
// the traffic.  group[t] is the same for the whole grid: read through the constant address space it is a scalar load.  Launches on
// the handle's stream are ordered, and a launch continues from the stored accumulators: that is how chunks keep the time order.
#pragma once

// the lane's pair of the current group: in registers from the first selected step of a run of equal ids until the run's end
struct CompAcc {
    double s;
    uint32_t n;
    bool have;
    int64_t at;                                     // g * npix + p: where the pair of the current group lies
    __device__ __forceinline__ void flush(double *__restrict__ sum, uint32_t *__restrict__ cnt)
    {
        if (have) { sum[at] = s; cnt[at] = n; have = false; }
    }
    __device__ __forceinline__ void add(double v, const double *__restrict__ sum, const uint32_t *__restrict__ cnt)
    {
        if (!have) { s = sum[at]; n = cnt[at]; have = true; }
        s = s + v;                                   // (float32 came through a plain conversion: denormals kept)
        n++;
    }
};

// time steps t .. t + U - 1: all U flag loads first, then the field loads of the lanes whose flag passed, then the sums in rising t
template <typename VT, bool GROUPED, bool SKIPNA, int U>
__device__ __forceinline__ void comp_batch(const int32_t *__restrict__ fp, const VT *__restrict__ xp, int64_t npix, int64_t p, int64_t t, ctk_const_i32 *group,
                                           int32_t above, int &g, CompAcc &acc, double *__restrict__ sum, uint32_t *__restrict__ cnt)
{
    int32_t f[U];
    VT v[U];
#pragma unroll
    for (int u = 0; u < U; u++) f[u] = __builtin_nontemporal_load(fp + (t + u) * npix);
#pragma unroll
    for (int u = 0; u < U; u++)
        if (f[u] > above) v[u] = xp[(t + u) * npix];
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (GROUPED) {
            const int gt = group[t + u];
            if (gt != g) { acc.flush(sum, cnt); g = gt; acc.at = (int64_t)g * npix + p; }
        }
        if (f[u] > above) {
            const double xv = (double)v[u];
            if (!SKIPNA || xv == xv) acc.add(xv, sum, cnt);
        }
    }
}

// flag, x: (T, npix); workgroup b of `blocks` takes part b of the plane.  umax: the widest batch (a power of two, at most
// CTK_COMPOSITE_UNROLL_MAX); the rest of T goes in ever shorter batches.  (Left alone the compiler takes 106 SGPRs: CTK_SGPR_8WAVES,
// ctk_kernels.hip.)
template <typename VT, bool GROUPED, bool SKIPNA>
__global__ __launch_bounds__(CTK_COMPOSITE_THREADS) CTK_SGPR_8WAVES void k_composite(const int32_t *__restrict__ flag, const VT *__restrict__ x, int64_t T, int64_t npix,
                                                                     int64_t blocks, const int32_t *__restrict__ group_ptr, int32_t above, int umax,
                                                                     double *__restrict__ sum, uint32_t *__restrict__ cnt)
{
    ctk_const_i32 *group = (ctk_const_i32 *)group_ptr;
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t p = b * CTK_COMPOSITE_THREADS + threadIdx.x;                // this lane's pixel (64-bit throughout)
        if (p >= npix) continue;
        const int32_t *fp = flag + p;
        const VT *xp = x + p;
        CompAcc acc;
        acc.s = 0.0; acc.n = 0; acc.have = false;
        int g = GROUPED ? group[0] : 0;
        acc.at = (int64_t)g * npix + p;
        int64_t t = 0;
#define CTK_COMP_BATCH(U) comp_batch<VT, GROUPED, SKIPNA, U>(fp, xp, npix, p, t, group, above, g, acc, sum, cnt)
        for (; umax >= 16 && t + 16 <= T; t += 16) CTK_COMP_BATCH(16);
        for (; umax >= 8 && t + 8 <= T; t += 8) CTK_COMP_BATCH(8);
        for (; umax >= 4 && t + 4 <= T; t += 4) CTK_COMP_BATCH(4);
        for (; umax >= 2 && t + 2 <= T; t += 2) CTK_COMP_BATCH(2);
        for (; t < T; t++) CTK_COMP_BATCH(1);
#undef CTK_COMP_BATCH
        acc.flush(sum, cnt);
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// sum / n += k_composite(flag[0..T), x[0..T)) on the handle's stream; group_dev: T device ints (nullptr: one group)
template <typename VT>
static int launch_composite_t(ctk_handle *h, const int32_t *flag_dev, const VT *x_dev, int64_t T, int64_t npix, const int32_t *group_dev, int32_t above, int skipna,
                              double *sum_dev, uint32_t *n_dev)
{
    const CtkCompositePlan pl = ctk_composite_plan((int)sizeof(VT), npix, h->cp_unroll_dbg);
    h->cp_unroll = pl.unroll; h->cp_grid = pl.grid;
#define CTK_COMP_LAUNCH(G, S) \
    k_composite<VT, G, S><<<pl.grid, CTK_COMPOSITE_THREADS, 0, h->stream>>>(flag_dev, x_dev, T, npix, pl.blocks, group_dev, above, pl.unroll, sum_dev, n_dev)
    if (group_dev) { if (skipna) CTK_COMP_LAUNCH(true, true); else CTK_COMP_LAUNCH(true, false); }
    else           { if (skipna) CTK_COMP_LAUNCH(false, true); else CTK_COMP_LAUNCH(false, false); }
#undef CTK_COMP_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}
static int launch_composite(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, bool f64, int64_t T, int64_t npix, const int32_t *group_dev, int32_t above,
                            int skipna, double *sum_dev, uint32_t *n_dev)
{
    return f64 ? launch_composite_t<double>(h, flag_dev, (const double *)x_dev, T, npix, group_dev, above, skipna, sum_dev, n_dev)
               : launch_composite_t<float>(h, flag_dev, (const float *)x_dev, T, npix, group_dev, above, skipna, sum_dev, n_dev);
}

// x == NULL: the anomaly slab that ctk_anom_* left resident on this handle, if its shape and type are the call's
static int comp_resident(ctk_handle *h, const char *name, bool f64, int64_t T, int ny, int nx, const void **x_dev)
{
    *x_dev = h->an_slab.find(T, ny, nx, f64);
    if (!*x_dev)
        return ctk_set_error(CTK_E_STATE, "%s: no field given, which needs a resident anomaly slab of this shape and type (ctk_anom_* with keep_resident)", name);
    return CTK_OK;
}

// the accumulators of one call: +0.0 and 0 are all-zero bytes
static int comp_zero(ctk_handle *h, double *sum_dev, uint32_t *n_dev, int ngroups, int64_t npix)
{
    HIPCHK(hipMemsetAsync(sum_dev, 0, (size_t)ngroups * npix * 8, h->stream));
    HIPCHK(hipMemsetAsync(n_dev, 0, (size_t)ngroups * npix * 4, h->stream));
    return CTK_OK;
}

static int composite_dev_impl(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, bool f64, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                              int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate, const char *name)
{
    if (h && (!flag_dev || !sum_dev || !n_dev)) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, name, T, ny, nx, group, ngroups, &group_dev));
    if (!x_dev) CTKCHK(comp_resident(h, name, f64, T, ny, nx, &x_dev));
    const int64_t npix = (int64_t)ny * nx;
    if (!accumulate) CTKCHK(comp_zero(h, sum_dev, n_dev, ngroups, npix));
    CTKCHK(launch_composite(h, flag_dev, x_dev, f64, T, npix, group_dev, above, skipna, sum_dev, n_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_composite_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *x_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                                     int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate)
{
    return composite_dev_impl(h, flag_dev, x_dev, false, T, ny, nx, group, ngroups, above, skipna, sum_dev, n_dev, accumulate, "ctk_composite_f32_dev");
}
extern "C" int ctk_composite_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *x_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                                     int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate)
{
    return composite_dev_impl(h, flag_dev, x_dev, true, T, ny, nx, group, ngroups, above, skipna, sum_dev, n_dev, accumulate, "ctk_composite_f64_dev");
}

// host arrays or reader callbacks: the field is stream_in's first slab and the flags its second, two chunk-sized device buffers each
// (chunk k+1 is read and copied while k_composite reduces chunk k).  `resident`: the field is the handle's anomaly slab and the flags
// are the only slab that travels.  The accumulators stay in HBM until the last chunk.
static int comp_stream_impl(ctk_handle *h, StreamIO &io, bool f64, bool resident, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                            int skipna, double *sum, uint32_t *n, int64_t chunk_steps, const char *name)
{
    if (h && (!sum || !n)) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    if (h && chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps=%lld", name, (long long)chunk_steps);
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, name, T, ny, nx, group, ngroups, &group_dev));
    const void *res_dev = nullptr;
    if (resident) CTKCHK(comp_resident(h, name, f64, T, ny, nx, &res_dev));
    const int64_t npix = (int64_t)ny * nx;
    const size_t esz = f64 ? 8 : 4;
    io.esz = resident ? 4 : esz;
    io.esz2 = resident ? 0 : 4;
    io.chunk = ctk_stream_chunk(chunk_steps, T, (size_t)npix * esz);
    const size_t cells = (size_t)ngroups * npix;
    CTKCHK(ensure(h, h->cp_sum, cells * 8));
    CTKCHK(ensure(h, h->cp_n, cells * 4));
    double *sdev = P<double>(h->cp_sum);
    uint32_t *ndev = P<uint32_t>(h->cp_n);
    CTKCHK(comp_zero(h, sdev, ndev, ngroups, npix));
    const double t0 = now_ms();
    CTKCHK(stream_consume(h, io, f64, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        const int32_t *fl = resident ? (const int32_t *)chunk : (const int32_t *)io.dev2;
        const void *xv = resident ? (const void *)((const char *)res_dev + (size_t)c0 * npix * esz) : chunk;
        return launch_composite(h, fl, xv, f64, nt, npix, group_dev ? group_dev + c0 : nullptr, above, skipna, sdev, ndev);
    }));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(sum, sdev, cells * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n, ndev, cells * 4, hipMemcpyDeviceToHost));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

static int composite_host_impl(ctk_handle *h, const int32_t *flag, const void *x, bool f64, int64_t T, int ny, int nx, const int32_t *group, int ngroups,
                               int32_t above, int skipna, double *sum, uint32_t *n, int64_t chunk_steps, const char *name)
{
    if (h && !flag) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    StreamIO io;
    if (x) { io.host_in = x; io.host_in2 = flag; }
    else io.host_in = flag;
    return comp_stream_impl(h, io, f64, x == nullptr, T, ny, nx, group, ngroups, above, skipna, sum, n, chunk_steps, name);
}

extern "C" int ctk_composite_f32(ctk_handle *h, const int32_t *flag, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                                 int skipna, double *sum, uint32_t *n, int64_t chunk_steps)
{
    return composite_host_impl(h, flag, x, false, T, ny, nx, group, ngroups, above, skipna, sum, n, chunk_steps, "ctk_composite_f32");
}
extern "C" int ctk_composite_f64(ctk_handle *h, const int32_t *flag, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                                 int skipna, double *sum, uint32_t *n, int64_t chunk_steps)
{
    return composite_host_impl(h, flag, x, true, T, ny, nx, group, ngroups, above, skipna, sum, n, chunk_steps, "ctk_composite_f64");
}
extern "C" int ctk_composite_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                                ctk_read_chunk_fn field_reader, void *field_user, const int32_t *group, int ngroups, int32_t above, int skipna, double *sum,
                                uint32_t *n, int64_t chunk_steps)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_composite_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    if (h && !flag_reader) return ctk_set_error(CTK_E_INVALID, "ctk_composite_cb: null flag reader");
    StreamIO io;
    if (field_reader) { io.read = field_reader; io.read_user = field_user; io.read2 = flag_reader; io.read2_user = flag_user; }
    else { io.read = flag_reader; io.read_user = flag_user; }
    return comp_stream_impl(h, io, elem_bytes == 8, field_reader == nullptr, T, ny, nx, group, ngroups, above, skipna, sum, n, chunk_steps, "ctk_composite_cb");
}

// what ctk_composite_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_composite_plan(int elem_bytes, int64_t npix, int unroll, int64_t *out3)
{
    if (!out3 || (elem_bytes != 4 && elem_bytes != 8) || npix < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_composite_plan: bad arguments");
    const CtkCompositePlan p = ctk_composite_plan(elem_bytes, npix, unroll);
    out3[0] = p.unroll; out3[1] = p.blocks; out3[2] = p.grid;
    return CTK_OK;
}

// test hook for the following k_composite launches on this handle: the widest batch of time steps (-1: the rule)
extern "C" int ctk_debug_set_composite(ctk_handle *h, int unroll)
{
    if (!h || unroll < -1 || unroll == 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_composite: null handle or unroll not -1 / positive");
    h->cp_unroll_dbg = unroll;
    return CTK_OK;
}

// out2 = { the widest batch of the last k_composite launch on this handle (0: none yet), its workgroups }
extern "C" int ctk_debug_composite_launch(ctk_handle *h, int64_t *out2)
{
    if (!h || !out2) return ctk_set_error(CTK_E_INVALID, "ctk_debug_composite_launch: null argument");
    out2[0] = h->cp_unroll; out2[1] = h->cp_grid;
    return CTK_OK;
}

// k_composite alone between HIP events on the handle's stream (tools/composite_probe.py): one launch that starts from zeroed
// accumulators, then `reps` timed launches that continue from them; ms2 = {best, mean} per launch
extern "C" int ctk_debug_time_composite(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const int32_t *group,
                                        int ngroups, int32_t above, int skipna, double *sum_dev, uint32_t *n_dev, int reps, double *ms2)
{
    if (h && (!flag_dev || !x_dev || !sum_dev || !n_dev || !ms2 || reps < 1)) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_composite: null buffer or reps < 1");
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, "ctk_debug_time_composite", T, ny, nx, group, ngroups, &group_dev));
    if ((int64_t)(reps + 1) * T > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_composite: (reps + 1) * T counts overflow uint32");
    const int64_t npix = (int64_t)ny * nx;
    const bool f64 = is_f64 != 0;
    CTKCHK(comp_zero(h, sum_dev, n_dev, ngroups, npix));
    return time_launches(h, "ctk_debug_time_composite", reps, ms2,
                         [&]() { return launch_composite(h, flag_dev, x_dev, f64, T, npix, group_dev, above, skipna, sum_dev, n_dev); });
}
