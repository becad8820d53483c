// ctk_anom.hip -- SURVEY.md section 8(f) rows N2 / N3 on the device (included by ctk_api.hip):
//   N2  contrack.calc_clim / calc_anom (contrack/contrack.py:458-581): group means (day-of-year climatology), centred rolling
//       mean over the groups with the reference's fill, anomaly, centred rolling mean over time.  The anomaly slab can stay
//       resident in HBM for run_contrack (ctk_track_resident): the producer of the hot path's input no longer pays PCIe twice.
//   N3  the percentile threshold of README.rst:150-151: per grid point of a latitude band the q-quantile over time (exact
//       order statistics by radix selection, numpy's linear interpolation), then the mean over the band.
//       The entries (ctk_anom_*, over independent time segments, streamed through chunk-sized buffers) are in ctk_anom_seg.hip, which
//       launches k_clim_raw / k_clim_roll from here unchanged: ctk_anom_* is its host path with no segments and k_anom from here, the
//       segmented entries replace k_anom by a form that reads every input once per tile.
// The reference evaluates these with xarray, which cannot be installed in the build container: what is implemented is the
// numpy restatement in oracle/anom_port.py (PARITY UNPINNED, see its header); sums in float64, results rounded to the input's
// dtype where xarray keeps it.
#pragma once

// clim_raw[g][p] = mean over the timesteps of group g, NaNs skipped (contrack.py:483)
template <typename VT>
__global__ __launch_bounds__(256) void k_clim_raw(const VT *__restrict__ x, const int32_t *__restrict__ tlist, const int32_t *__restrict__ goff, int64_t npix,
                                                  VT *__restrict__ raw)
{
    const int g = (int)blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    double s = 0.0;
    int c = 0;
    for (int k = goff[g]; k < goff[g + 1]; k++) {
        const VT v = x[(int64_t)tlist[k] * npix + p];
        if (!an_isnan(v)) { s += (double)v; c++; }
    }
    raw[(int64_t)g * npix + p] = c ? (VT)(s / c) : (VT)__builtin_nanf("");
}

// centred rolling mean over the groups, NaN -> mean of the last `window` groups (contrack.py:487-489)
template <typename VT>
__global__ __launch_bounds__(256) void k_clim_roll(const VT *__restrict__ raw, int G, int window, int64_t npix, VT *__restrict__ clim)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    double fs = 0.0;
    int fc = 0;
    for (int g = max(0, G - window); g < G; g++) {
        const VT v = raw[(int64_t)g * npix + p];
        if (!an_isnan(v)) { fs += (double)v; fc++; }
    }
    const VT fill = fc ? (VT)(fs / fc) : (VT)__builtin_nanf("");
    for (int g = (int)blockIdx.y; g < G; g += (int)gridDim.y) {
        const int lo = g - window / 2, hi = g + (window - 1) / 2;
        VT r = fill;
        if (lo >= 0 && hi < G) {
            double s = 0.0;
            for (int j = lo; j <= hi; j++) s += (double)raw[(int64_t)j * npix + p];        // (a NaN makes the window NaN)
            const VT m = (VT)(s / window);
            if (!an_isnan(m)) r = m;
        }
        clim[(int64_t)g * npix + p] = r;
    }
}

// anomaly + centred rolling mean over time (contrack.py:566-570); NaN where the window leaves the axis or holds a NaN
template <typename VT>
__global__ __launch_bounds__(256) void k_anom(const VT *__restrict__ x, const VT *__restrict__ clim, const int32_t *__restrict__ group, int64_t T, int64_t npix,
                                              int smooth, int tseg, VT *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int64_t t0 = (int64_t)blockIdx.y * tseg, t1 = min(T, t0 + tseg);
    for (int64_t t = t0; t < t1; t++) {
        const int64_t lo = t - smooth / 2, hi = t + (smooth - 1) / 2;
        VT r = (VT)__builtin_nanf("");
        if (lo >= 0 && hi < T) {
            double s = 0.0;
            for (int64_t j = lo; j <= hi; j++) s += (double)(VT)((double)x[j * npix + p] - (double)clim[(int64_t)group[j] * npix + p]);
            r = (VT)(s / smooth);
        }
        out[t * npix + p] = r;
    }
}

// ---- N3: q-quantile over time per grid point of rows [y0, y1), exact: pf_select (ctk_select.h) on the pixel's whole column -------
template <typename VT, typename KT>
__global__ __launch_bounds__(CTK_PFIELD_DIRECT_THREADS) void k_quantile(const VT *__restrict__ x, int64_t T, int64_t npix, int64_t p0, int64_t nband, double q,
                                                                        double *__restrict__ out)
{
    constexpr int TILE = CTK_PFIELD_DIRECT_TILE, NT = CTK_PFIELD_DIRECT_THREADS;
    __shared__ PfSel<KT, TILE, NT> S;
    const int64_t pb = (int64_t)blockIdx.x * TILE + (int)threadIdx.x % TILE;
    const bool live = pb < nband;
    const VT *col = x + p0 + (live ? pb : 0);
    const double r = pf_select<VT, KT, TILE, NT>(S, [&](int j) { return col[(int64_t)j * npix]; }, (int)T, live, q);
    if ((int)threadIdx.x < TILE && live) out[pb] = r;
}

// mean of the non-NaN entries, fixed order (one workgroup, pairwise tree)
__global__ __launch_bounds__(1024) void k_nanmean(const double *__restrict__ v, int64_t n, double *__restrict__ out)
{
    __shared__ double ss[1024];
    __shared__ unsigned long long sc[1024];
    double s = 0.0;
    unsigned long long c = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) { const double a = v[i]; if (a == a) { s += a; c++; } }
    ss[threadIdx.x] = s; sc[threadIdx.x] = c;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) { ss[threadIdx.x] += ss[threadIdx.x + d]; sc[threadIdx.x] += sc[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sc[0] ? ss[0] / (double)sc[0] : __builtin_nan("");
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// ---- shared by the percentile entries (ctk_percentile_* below, ctk_pctl.hip, ctk_pfield.hip) and ctk_anom_* ------------------------
struct PctlArgs {
    int64_t T; int ny, nx, y0, y1; const int32_t *group; int ngroups, window; double q;
    int64_t npix() const { return (int64_t)ny * nx; }
    int64_t nband() const { return (int64_t)(y1 - y0) * nx; }                  // the band: rows [y0, y1) of every plane ...
    int64_t p0() const { return (int64_t)y0 * nx; }                            // ... from this element of the plane on
};

// what ctk_percentile_groups_* and ctk_percentile_field_* check alike
static int pctl_validate_common(const ctk_handle *h, const PctlArgs &a, const double *out, const char *name)
{
    if (!h || !out || !a.group) return ctk_set_error(CTK_E_INVALID, "%s: null argument", name);
    if (a.T < 1 || a.ny < 1 || a.nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad shape (T=%lld ny=%d nx=%d)", name, (long long)a.T, a.ny, a.nx);
    if (a.T > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: T=%lld timesteps (at most 2^31 - 1)", name, (long long)a.T);
    if (a.y0 < 0 || a.y1 > a.ny || a.y0 >= a.y1) return ctk_set_error(CTK_E_INVALID, "%s: rows [%d, %d) are not rows of a grid of %d", name, a.y0, a.y1, a.ny);
    if (a.ngroups < 1) return ctk_set_error(CTK_E_INVALID, "%s: ngroups=%d (at least 1)", name, a.ngroups);
    if (a.window < 1) return ctk_set_error(CTK_E_INVALID, "%s: window=%d (at least 1)", name, a.window);
    if (!(a.q >= 0.0 && a.q <= 1.0)) return ctk_set_error(CTK_E_INVALID, "%s: q=%g is not in [0, 1]", name, a.q);
    for (int64_t t = 0; t < a.T; t++)
        if (a.group[t] < 0 || a.group[t] >= a.ngroups) return ctk_set_error(CTK_E_INVALID, "%s: group[%lld] = %d is not in [0, %d)", name, (long long)t, a.group[t], a.ngroups);
    return CTK_OK;
}

// the slab an entry selects on: x_host uploaded into io_in on the handle's stream, or (x_host NULL) the resident anomaly slab
template <typename VT>
static int pctl_slab(ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, const char *who, const VT **x_dev)
{
    if (x_host) {
        const size_t bytes = (size_t)T * (size_t)ny * (size_t)nx * sizeof(VT);
        CTKCHK(claim_io(h, h->io_in, bytes));
        HIPCHK(hipMemcpyAsync(h->io_in.p, x_host, bytes, hipMemcpyHostToDevice, h->stream));
        *x_dev = (const VT *)h->io_in.p;
    } else {
        *x_dev = (const VT *)h->an_slab.find(T, ny, nx, sizeof(VT) == 8);
        if (!*x_dev) return ctk_set_error(CTK_E_STATE, "%s: no matching anomaly slab is resident", who);
    }
    return CTK_OK;
}

// counting sort of the timesteps by group (ids in [0, G), T < 2^31): slist[off[g] .. off[g + 1]) = the steps of group g, rising
static void steps_by_group(const int32_t *group, int64_t T, int G, int32_t *slist, int32_t *off)
{
    std::fill(off, off + G + 1, 0);
    for (int64_t t = 0; t < T; t++) off[group[t] + 1]++;
    for (int g = 0; g < G; g++) off[g + 1] += off[g];
    std::vector<int32_t> cur(off, off + G);
    for (int64_t t = 0; t < T; t++) slist[cur[(size_t)group[t]]++] = (int32_t)t;
}

// the scalar percentile's kernels on the handle's stream: qv[0 .. nband) the per-pixel quantiles, qv[nband] their mean
template <typename VT, typename KT>
static void launch_quantile(ctk_handle *h, const VT *x_dev, int64_t T, int64_t npix, int64_t p0, int64_t nband, double q, double *qv)
{
    k_quantile<VT, KT><<<(unsigned)((nband + CTK_PFIELD_DIRECT_TILE - 1) / CTK_PFIELD_DIRECT_TILE), CTK_PFIELD_DIRECT_THREADS, 0, h->stream>>>(x_dev, T, npix, p0, nband, q, qv);
    k_nanmean<<<1, 1024, 0, h->stream>>>(qv, nband, qv + nband);
}

// WHICH slab is resident: a number that changes whenever the resident slab is written (any ctk_anom_* call that produces
// anomalies) or dropped (ctk_release_io).  A caller that left a slab resident remembers the number and runs on the slab only
// while it is unchanged -- two class instances sharing one handle cannot take each other's anomalies for their own.
extern "C" int ctk_resident_anom_generation(ctk_handle *h, uint64_t *generation)
{
    if (!h || !generation) return ctk_set_error(CTK_E_INVALID, "null argument");
    *generation = h->an_slab.gen;
    return CTK_OK;
}

// shape of the anomaly slab kept in HBM by the last ctk_anom_* call with keep_resident (T = -1: none)
extern "C" int ctk_resident_anom(ctk_handle *h, int64_t *T, int *ny, int *nx, int *is_f64)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "null handle");
    h->an_slab.report(T, ny, nx, is_f64);
    return CTK_OK;
}

// run_contrack on the resident anomaly slab: no H2D; flag goes to the host
extern "C" int ctk_track_resident(ctk_handle *h, const double *thr, int cmp_op, const float *wrow, double overlap, int persistence, int twosided,
                                  int32_t *flag, int64_t *n_tracked)
{
    if (!h || !flag) return ctk_set_error(CTK_E_INVALID, "null argument");
    const ResidentSlab &a = h->an_slab;
    if (!a.held()) return ctk_set_error(CTK_E_STATE, "ctk_track_resident: no anomaly slab is resident (ctk_anom_* with keep_resident)");
    HIPCHK(hipSetDevice(h->device));
    return track_to_host(h, a.buf.p, a.f64, a.T, a.ny, a.nx, thr, cmp_op, wrow, overlap, persistence, twosided, flag, n_tracked, nullptr);
}

template <typename VT, typename KT>
static int percentile_impl(ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, int y0, int y1, double q, double *out)
{
    if (!h || !out || T < 1 || ny < 1 || nx < 1 || y0 < 0 || y1 > ny || y0 >= y1 || !(q >= 0.0 && q <= 1.0)) return ctk_set_error(CTK_E_INVALID, "ctk_percentile: bad arguments");
    if (T > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "ctk_percentile: T=%lld timesteps (at most 2^31 - 1)", (long long)T);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t npix = (int64_t)ny * nx, nband = (int64_t)(y1 - y0) * nx;
    const VT *x_dev;
    CTKCHK(pctl_slab(h, x_host, T, ny, nx, "ctk_percentile", &x_dev));
    h->an_pct_n = -1;
    CTKCHK(ensure(h, h->an_raw, ((size_t)nband + 8) * 8));
    double *qv = P<double>(h->an_raw);
    launch_quantile<VT, KT>(h, x_dev, T, npix, (int64_t)y0 * nx, nband, q, qv);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, qv + nband, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    h->an_pct_n = nband;
    return CTK_OK;
}
extern "C" int ctk_percentile_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, double q, double *out)
{
    return percentile_impl<float, uint32_t>(h, x, T, ny, nx, y0, y1, q, out);
}
extern "C" int ctk_percentile_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, double q, double *out)
{
    return percentile_impl<double, uint64_t>(h, x, T, ny, nx, y0, y1, q, out);
}

// test hook: the per-pixel quantiles of the last ctk_percentile_* call (band order, row-major), still in an_raw
extern "C" int ctk_debug_percentile_values(ctk_handle *h, double *out, int64_t n)
{
    if (!h || !out) return ctk_set_error(CTK_E_INVALID, "null argument");
    if (h->an_pct_n < 0) return ctk_set_error(CTK_E_STATE, "ctk_debug_percentile_values: no ctk_percentile_* result is held");
    if (n != h->an_pct_n) return ctk_set_error(CTK_E_INVALID, "ctk_debug_percentile_values: n = %lld, the last band had %lld pixels", (long long)n, (long long)h->an_pct_n);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(out, h->an_raw.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return CTK_OK;
}
