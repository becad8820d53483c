// ctk_pfield.hip -- the percentile threshold FIELD per calendar day on the device (included by ctk_api.hip): what
// ctk_set_threshold_field consumes.  For every group g (calendar day) and every grid point of rows [y0, y1) the exact q-quantile
// (np.nanquantile, method 'linear', in float64) over the timesteps whose group lies in the centred window of W groups around g,
// taken circularly over the G groups:
//     pool(g, y, x') = { x[t, y, x'] : group[t] in { (g + d) mod G : -(W / 2) <= d <= (W - 1) / 2 } }
//
// The host sorts the timesteps by group once (a step list and G + 1 offsets).  The members of a window are consecutive groups
// modulo G, so every pool is one circular slice of that list: positions [A_g, A_g + len_g) of the list repeated, with A_g and
// A_g + len_g rising with g.  One radix selection (pf_select, ctk_select.h: 8-bit digits of the order-preserving keys of an_key, most
// significant first, per-pixel histograms in LDS, several lanes per pixel) serves two forms (ctk_pfield_plan, ctk_forms.h):
//   k_pfield_direct  a workgroup takes 64 consecutive pixels of the band and ONE group and fetches every pass from global memory
//                    through the step list: sizeof(key) reads of the pool per (group, pixel).  Valid for pools of any length.
//   k_pfield_ring    a workgroup takes 32, 16 or 8 consecutive pixels for ALL groups and keeps their current pool in LDS as a
//                    ring of timesteps: going from g to g + 1 it loads the positions [A_g + len_g, A_{g+1} + len_{g+1}) over the
//                    slots of the positions that left.  The slab is read 1 + W / G times; the passes run on the LDS copy.
// The count of the pool comes out of the first digit's histogram; the number of values <= the selected key and the next larger key
// come out of the last digit's pass (the histogram, or the smallest key under a larger prefix, tracked in the same pass).
// W >= G: every group has the same pool -- one plane is selected and k_pfield_replicate copies it.  Pool counts are per pixel:
// uint32 behind the host check T < 2^31.  Every load of the slab is one element wide: the band may start at any row.
#pragma once

// blockIdx.x = plane + planes * tile: the workgroups of a tile's groups run together and share its columns in the cache
template <typename VT, typename KT>
__global__ __launch_bounds__(CTK_PFIELD_DIRECT_THREADS) void k_pfield_direct(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int T,
                                                                             const int32_t *__restrict__ slist, const int64_t *__restrict__ pa,
                                                                             const int32_t *__restrict__ plen, int planes, double q, double *__restrict__ out)
{
    constexpr int TILE = CTK_PFIELD_DIRECT_TILE, NT = CTK_PFIELD_DIRECT_THREADS;
    __shared__ PfSel<KT, TILE, NT> S;
    const int g = (int)(blockIdx.x % (unsigned)planes);
    const int64_t pb = (int64_t)(blockIdx.x / (unsigned)planes) * TILE + (int)threadIdx.x % TILE;
    const bool live = pb < nband;
    const int a = (int)(pa[g] % T), len = plen[g];
    const VT *col = x + p0 + (live ? pb : 0);
    const double r = pf_select<VT, KT, TILE, NT>(S, [&](int j) { int64_t i = (int64_t)a + j; if (i >= T) i -= T; return col[(int64_t)slist[i] * npix]; }, len, live, q);
    if ((int)threadIdx.x < TILE && live) out[(int64_t)g * nband + pb] = r;
}

template <typename VT, typename KT, int TILE>
__global__ __launch_bounds__(CTK_PFIELD_RING_THREADS) void k_pfield_ring(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int T,
                                                                         const int32_t *__restrict__ slist, const int64_t *__restrict__ pa,
                                                                         const int32_t *__restrict__ plen, int planes, double q, double *__restrict__ out)
{
    constexpr int NT = CTK_PFIELD_RING_THREADS, L = NT / TILE;
    constexpr int R = (int)ctk_pfield_ring_steps((int)sizeof(VT), TILE);
    __shared__ PfSel<KT, TILE, NT> S;
    __shared__ VT ring[(size_t)R * TILE];                                      // slot of list position p: p % R
    const int px = (int)threadIdx.x % TILE, lane = (int)threadIdx.x / TILE;
    const int64_t pb = (int64_t)blockIdx.x * TILE + px;
    const bool live = pb < nband;
    const VT *col = x + p0 + (live ? pb : 0);
    int64_t have = pa[0];                                                      // positions [A, have) are in the ring
    for (int g = 0; g < planes; g++) {
        const int64_t A = pa[g];
        const int len = plen[g];                                               // (<= R: ctk_pfield_plan)
        const int64_t B = A + len;
        if (live)
            for (int64_t pos = (have > A ? have : A) + lane; pos < B; pos += L) {
                int64_t i = pos;
                while (i >= T) i -= T;                                         // (pos < 3 T)
                ring[(size_t)(pos % R) * TILE + px] = col[(int64_t)slist[i] * npix];
            }
        have = B;
        __syncthreads();
        const int slot0 = (int)(A % R);
        const double r = pf_select<VT, KT, TILE, NT>(S, [&](int j) { int s = slot0 + j; if (s >= R) s -= R; return ring[(size_t)s * TILE + px]; }, len, live, q);
        if (lane == 0 && live) out[(int64_t)g * nband + pb] = r;
    }
}

// out[g][i] = out[0][i], 1 <= g < G
__global__ __launch_bounds__(256) void k_pfield_replicate(double *__restrict__ out, int64_t nband, int G)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nband) return;
    const double v = out[i];
    for (int g = 1 + (int)blockIdx.y; g < G; g += (int)gridDim.y) out[(int64_t)g * nband + i] = v;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
struct PfPrep {
    std::vector<int32_t> slist, plen;      // timesteps sorted by group; pool length per plane
    std::vector<int64_t> pa;               // pool start per plane, as a position of the list repeated (rising with the plane)
    int64_t max_pool = 0;
};

static int pfield_validate(const ctk_handle *h, const PctlArgs &a, const double *out, const char *name)
{
    CTKCHK(pctl_validate_common(h, a, out, name));
    const int64_t nband = a.nband(), tiles = (nband + CTK_PFIELD_MIN_TILE - 1) / CTK_PFIELD_MIN_TILE;
    if (tiles * (int64_t)a.ngroups > 0x7fffffffll)
        return ctk_set_error(CTK_E_INVALID, "%s: %d groups x a band of %lld values is too large", name, a.ngroups, (long long)nband);
    return CTK_OK;
}

static void pfield_prepare(const PctlArgs &a, PfPrep &p)
{
    const int G = a.ngroups, W = a.window;
    const int64_t T = a.T;
    std::vector<int32_t> off((size_t)G + 1);
    p.slist.resize((size_t)T);
    steps_by_group(a.group, T, G, p.slist.data(), off.data());
    if (W >= G) { p.pa.assign(1, 0); p.plen.assign(1, (int32_t)T); p.max_pool = T; return; }
    auto off2 = [&](int64_t u) { return off[(size_t)(u % G)] + T * (u / G); };
    p.pa.resize((size_t)G); p.plen.resize((size_t)G);
    p.max_pool = 0;
    for (int g = 0; g < G; g++) {
        const int64_t u = (int64_t)g - W / 2 + G;
        p.pa[(size_t)g] = off2(u);
        p.plen[(size_t)g] = (int32_t)(off2(u + W) - off2(u));
        p.max_pool = std::max<int64_t>(p.max_pool, p.plen[(size_t)g]);
    }
}

// the whole field on a slab in device memory, on the handle's stream; the G planes are left in device memory (h->pf_out)
template <typename VT, typename KT>
static int pfield_launch(ctk_handle *h, const VT *x_dev, const PctlArgs &a, const PfPrep &p, bool force_direct)
{
    hipStream_t s = h->stream;
    const int G = a.ngroups, T = (int)a.T;
    const int64_t npix = a.npix(), nband = a.nband(), p0 = a.p0();
    const CtkPfieldPlan f = ctk_pfield_plan((int)sizeof(KT), force_direct ? INT64_MAX : p.max_pool, G, a.window);
    const int planes = f.planes;
    CTKCHK(ensure(h, h->pf_out, (size_t)G * (size_t)nband * 8));
    CTKCHK(ensure(h, h->pf_idx, 8 + (size_t)planes * 12 + (size_t)T * 4));       // the read probe's sink, pa, plen, slist
    int64_t *pa = P<int64_t>(h->pf_idx) + 1;
    int32_t *plen = (int32_t *)(pa + planes), *slist = plen + planes;
    HIPCHK(hipMemcpyAsync(pa, p.pa.data(), (size_t)planes * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(plen, p.plen.data(), (size_t)planes * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(slist, p.slist.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
    double *out = P<double>(h->pf_out);
    const int64_t tiles = (nband + f.tile - 1) / f.tile;
    if (f.form == CTK_PFIELD_DIRECT)
        k_pfield_direct<VT, KT><<<(unsigned)(tiles * planes), CTK_PFIELD_DIRECT_THREADS, 0, s>>>(x_dev, npix, p0, nband, T, slist, pa, plen, planes, a.q, out);
    else if (f.tile == 32)
        k_pfield_ring<VT, KT, 32><<<(unsigned)tiles, CTK_PFIELD_RING_THREADS, 0, s>>>(x_dev, npix, p0, nband, T, slist, pa, plen, planes, a.q, out);
    else if (f.tile == 16)
        k_pfield_ring<VT, KT, 16><<<(unsigned)tiles, CTK_PFIELD_RING_THREADS, 0, s>>>(x_dev, npix, p0, nband, T, slist, pa, plen, planes, a.q, out);
    else
        k_pfield_ring<VT, KT, 8><<<(unsigned)tiles, CTK_PFIELD_RING_THREADS, 0, s>>>(x_dev, npix, p0, nband, T, slist, pa, plen, planes, a.q, out);
    if (planes < G) k_pfield_replicate<<<dim3((unsigned)((nband + 255) / 256), (unsigned)std::min(G - 1, 64)), 256, 0, s>>>(out, nband, G);
    HIPCHK(hipGetLastError());
    h->pf_form = f.form; h->pf_max_pool = p.max_pool;
    return CTK_OK;
}

template <typename VT, typename KT>
static int percentile_field_impl(ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                 double q, double *out)
{
    const PctlArgs a = {T, ny, nx, y0, y1, group, ngroups, window, q};
    CTKCHK(pfield_validate(h, a, out, "ctk_percentile_field"));
    HIPCHK(hipSetDevice(h->device));
    const VT *x_dev;
    CTKCHK(pctl_slab(h, x_host, T, ny, nx, "ctk_percentile_field", &x_dev));
    PfPrep prep;
    pfield_prepare(a, prep);
    CTKCHK((pfield_launch<VT, KT>(h, x_dev, a, prep, false)));
    HIPCHK(hipMemcpyAsync(out, h->pf_out.p, (size_t)ngroups * (size_t)a.nband() * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_percentile_field_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                        double q, double *out)
{
    return percentile_field_impl<float, uint32_t>(h, x, T, ny, nx, y0, y1, group, ngroups, window, q, out);
}
extern "C" int ctk_percentile_field_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                        double q, double *out)
{
    return percentile_field_impl<double, uint64_t>(h, x, T, ny, nx, y0, y1, group, ngroups, window, q, out);
}

// what ctk_pfield_plan decides (host only, no device): out4 = { form (CtkPfieldForm), cap in pool steps, pixel tile, ring bytes }
extern "C" int ctk_debug_percentile_field_plan(int keybytes, int64_t max_pool_steps, int ngroups, int window, int64_t *out4)
{
    if (!out4 || (keybytes != 4 && keybytes != 8) || max_pool_steps < 0 || ngroups < 1 || window < 1)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_percentile_field_plan: bad arguments");
    const CtkPfieldPlan f = ctk_pfield_plan(keybytes, max_pool_steps, ngroups, window);
    out4[0] = f.form; out4[1] = f.cap; out4[2] = f.tile; out4[3] = f.ring_bytes;
    return CTK_OK;
}

// test hook: out2 = { form of the last ctk_percentile_field_* call on this handle (-1: none), its longest pool in timesteps }
extern "C" int ctk_debug_percentile_field_form(ctk_handle *h, int64_t *out2)
{
    if (!h || !out2) return ctk_set_error(CTK_E_INVALID, "null argument");
    out2[0] = h->pf_form; out2[1] = h->pf_max_pool;
    return CTK_OK;
}

// measurement (tools/pfield_probe.py, profiles/NOTES.md) on a slab in device memory (is_f64: float64): ms4 = { the form
// ctk_pfield_plan chooses, the direct form forced on the same input (both: best of reps, host clock around the upload of the lists,
// every kernel and the synchronisation; the download of the field is outside), one plain 16-byte read stream over the band
// (k_pctl_read, best of reps, HIP events), the chosen form (CtkPfieldForm) }.  out / out_direct (either may be NULL): the two fields.
template <typename VT, typename KT>
static int time_pfield_impl(ctk_handle *h, const VT *x_dev, const PctlArgs &a, int reps, double *out, double *out_direct, double *ms4)
{
    hipStream_t s = h->stream;
    const int64_t npix = a.npix(), nband = a.nband(), p0 = a.p0();
    PfPrep prep;
    pfield_prepare(a, prep);
    for (int form = 0; form < 2; form++) {
        double best = 1e30;
        for (int r = 0; r <= reps; r++) {                                      // (the first call grows the buffers)
            const double t0 = now_ms();
            CTKCHK((pfield_launch<VT, KT>(h, x_dev, a, prep, form == 1)));
            HIPCHK(hipStreamSynchronize(s));
            if (r) best = std::min(best, now_ms() - t0);
        }
        ms4[form] = best;
        if (form == 0) ms4[3] = (double)h->pf_form;
        double *dst = form ? out_direct : out;
        if (dst) HIPCHK(hipMemcpy(dst, h->pf_out.p, (size_t)a.ngroups * (size_t)nband * 8, hipMemcpyDeviceToHost));
    }
    const int64_t chunk = CTK_PCTL_CHUNK;
    const unsigned chunks = (unsigned)((nband + chunk - 1) / chunk);
    if (chunks > 65535) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_percentile_field: a band of %lld values is too large for the read stream", (long long)nband);
    Event ev[2];
    int rc = CTK_OK;
    for (Event &e : ev)
        if (rc == CTK_OK && e.create() != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed");
    uint64_t *sink = P<uint64_t>(h->pf_idx);                                    // (8 bytes in front of the lists)
    double best = 1e30;
    for (int r = 0; r <= reps && rc == CTK_OK; r++) {
        float m = 0;
        if (hipEventRecord(ev[0], s) != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        k_pctl_read<VT, KT><<<dim3((unsigned)a.T, chunks), 256, 0, s>>>(x_dev, npix, p0, nband, chunk, sink);
        if (rc == CTK_OK && (hipEventRecord(ev[1], s) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess || hipGetLastError() != hipSuccess ||
                             hipEventElapsedTime(&m, ev[0], ev[1]) != hipSuccess))
            rc = ctk_set_error(CTK_E_NODEVICE, "ctk_debug_time_percentile_field: a timed launch failed");
        if (r) best = std::min(best, (double)m);
    }
    ms4[2] = best;
    (void)hipStreamSynchronize(s);
    return rc;
}

extern "C" int ctk_debug_time_percentile_field(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group,
                                               int ngroups, int window, double q, int reps, double *out, double *out_direct, double *ms4)
{
    const PctlArgs a = {T, ny, nx, y0, y1, group, ngroups, window, q};
    double dummy = 0;
    CTKCHK(pfield_validate(h, a, &dummy, "ctk_debug_time_percentile_field"));
    if (!x_dev || !ms4 || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_percentile_field: null buffer or reps < 1");
    HIPCHK(hipSetDevice(h->device));
    for (int i = 0; i < 4; i++) ms4[i] = 0;
    return is_f64 ? time_pfield_impl<double, uint64_t>(h, (const double *)x_dev, a, reps, out, out_direct, ms4)
                  : time_pfield_impl<float, uint32_t>(h, (const float *)x_dev, a, reps, out, out_direct, ms4);
}
