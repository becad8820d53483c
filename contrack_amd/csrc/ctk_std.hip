// ctk_std.hip -- the standard-deviation threshold FIELD per calendar day on the device (included by ctk_api.hip): the other half of
// the reference's open item (contrack/contrack.py:9-10, "take 90th percentile or std_dev from anom field for threshold").  For every
// group g and every grid point of rows [y0, y1) the two-pass statement of include/contrack_hip.h in float64 over the pool of
// ctk_pfield.hip -- the timesteps whose group lies in the centred, circular window of W groups around g -- TAKEN IN TIME ORDER:
//     s = 0; c = 0;  for t rising:  v = x[t];  (skipna and v is NaN) ? v = 0 : c += 1;  s = s + v
//     m = s / c
//     q = 0;         for t rising:  v = x[t];  skip if (skipna and v is NaN);  d = v - m;  q = q + d * d
//     std = c - ddof > 0 ? sqrt(q / (c - ddof)) : NaN
// A timestep feeds the W accumulators of the groups whose window holds its group, and every accumulator must see its values in
// time order.  k_std_field gives every accumulator ONE writer: a workgroup takes 32, 16 or 8 consecutive pixels of the band
// (ctk_std_plan, ctk_forms.h) for ALL planes; its 512 threads are `owners` = 512 / tile per pixel, and owner s of a pixel holds the
// planes h with h % owners == s.  Every thread walks time once per pass and at each step updates those of its own planes that lie in
// the window of group[t] (the host passes the window's first plane per step) -- no thread ever touches another's accumulator, so no
// atomic, no barrier and no lock-step assumption orders the additions: program order does.  The accumulators live in LDS as
// [plane][pixel] arrays (the lanes of an owner are the tile's consecutive pixels, adjacent owners hold adjacent planes: consecutive
// 8-byte words, no bank is asked twice), the one a thread touched last in its registers; the slab is read once per pass,
// CTK_STD_STAGE timesteps of the tile at a time into LDS (the only barriers), the next round's loads in flight while the current
// one is accumulated.  W >= G: every group has the same pool -- one plane is accumulated and k_std_replicate
// copies it.  Without skipna the count is the pool's length, which the host knows (plen).  Every load of the slab is one element
// wide: the band may start at any row.  Division and square root are the IEEE operators; the build has -ffp-contract=off.
#pragma once

// the planes of owner s among [a, b), ascending: h = a + ((s - a) mod owners), then every owners-th
#define CTK_STD_OWNED(a, b, body)                                                        \
    for (int h = (a) + (((s) - (a)) & (OWNERS - 1)); h < (b); h += OWNERS) { body }

// one pass over time of a thread (pixel px, owner s): PASS 0 adds the values and counts them, PASS 1 adds the squared distances from
// the mean.  The accumulator the thread touched last stays in registers (hc: its plane, -1 none): consecutive days feed the same
// plane of an owner W times in a row, so most additions never wait for LDS.  The thread is the accumulator's only reader and writer,
// and it writes the registers back before it takes up another plane: every accumulator still sees its values in time order.
template <typename VT, int TILE, bool SKIPNA, bool NARROW, int PASS>
__device__ __forceinline__ void std_pass(const VT *__restrict__ col, bool live, int64_t npix, int T, const int32_t *__restrict__ first, int planes, int W,
                                         double *acc_s, double *acc_q, uint32_t *acc_n, VT *stage, int px, int s)
{
    constexpr int OWNERS = CTK_STD_THREADS / TILE, R = CTK_STD_STAGE, E = R / OWNERS, U = 8;
    static_assert(R % OWNERS == 0 && E >= 1 && (OWNERS & (OWNERS - 1)) == 0 && R % U == 0, "a thread stages E whole steps of its own pixel");
    double *acc = PASS == 0 ? acc_s : acc_q;
    int hc = -1;
    double sc = 0.0, mc = 0.0;
    uint32_t nc = 0u;
#define CTK_STD_FLUSH() if (hc >= 0) { acc[hc * TILE + px] = sc; if (SKIPNA && PASS == 0) acc_n[hc * TILE + px] = nc; }
#define CTK_STD_UPDATE(val)                                                                                          \
    if (h != hc) {                                                                                                   \
        CTK_STD_FLUSH()                                                                                              \
        hc = h; sc = acc[h * TILE + px];                                                                             \
        if (PASS != 0) mc = acc_s[h * TILE + px]; else if (SKIPNA) nc = acc_n[h * TILE + px];                        \
    }                                                                                                                \
    if (PASS == 0) { sc += (val); nc++; } else { const double d = (val) - mc; sc += d * d; }
    VT r[E];
#pragma unroll
    for (int e = 0; e < E; e++) { const int t = e * OWNERS + s; r[e] = live && t < T ? col[(int64_t)t * npix] : (VT)0; }
    for (int64_t t0 = 0; t0 < T; t0 += R) {
        __syncthreads();                                                       // the round before has been consumed
#pragma unroll
        for (int e = 0; e < E; e++) stage[(e * OWNERS + s) * TILE + px] = r[e];
        __syncthreads();
        if (t0 + R < T) {
#pragma unroll
            for (int e = 0; e < E; e++) { const int64_t t = t0 + R + e * OWNERS + s; r[e] = live && t < T ? col[t * npix] : (VT)0; }
        }
        const int n = (int)min((int64_t)R, T - t0);
        if (!live) continue;
        for (int j0 = 0; j0 < n; j0 += U) {                                    // U steps' values and first planes are fetched together
            double v[U];
            int a[U];
#pragma unroll
            for (int u = 0; u < U; u++) { v[u] = (double)stage[(j0 + u) * TILE + px]; a[u] = first[t0 + j0 + u]; }     // (first is padded to whole rounds)
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (j0 + u >= n || (SKIPNA && v[u] != v[u])) continue;
                const int b = a[u] + W;                                        // the planes a[u] .. a[u] + W - 1 (mod planes); W <= planes: one wrap at most
                if (NARROW) {                                                  // W <= owners: at most one own plane before the wrap, at most plane s after it
                    { const int h = a[u] + ((s - a[u]) & (OWNERS - 1)); if (h < min(b, planes)) { CTK_STD_UPDATE(v[u]) } }
                    { const int h = s; if (h < b - planes) { CTK_STD_UPDATE(v[u]) } }
                } else {
                    CTK_STD_OWNED(a[u], min(b, planes), CTK_STD_UPDATE(v[u]))
                    CTK_STD_OWNED(0, b - planes, CTK_STD_UPDATE(v[u]))
                }
            }
        }
    }
    CTK_STD_FLUSH()
#undef CTK_STD_UPDATE
#undef CTK_STD_FLUSH
}

template <typename VT, int TILE, bool SKIPNA, bool NARROW>
__global__ __launch_bounds__(CTK_STD_THREADS) void k_std_field(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int T,
                                                               const int32_t *__restrict__ first, const int32_t *__restrict__ plen, int planes, int W,
                                                               int ddof, double *__restrict__ out_std, double *__restrict__ out_mean,
                                                               uint32_t *__restrict__ out_n)
{
    constexpr int OWNERS = CTK_STD_THREADS / TILE;
    extern __shared__ __align__(16) unsigned char std_lds[];
    double *acc_s = (double *)std_lds;                                         // [planes][TILE]: the sum, then the mean
    double *acc_q = acc_s + (size_t)planes * TILE;                             // [planes][TILE]
    uint32_t *acc_n = (uint32_t *)(acc_q + (size_t)planes * TILE);             // [planes][TILE] (SKIPNA)
    VT *stage = (VT *)((unsigned char *)(acc_q + (size_t)planes * TILE) + (SKIPNA ? (size_t)planes * TILE * 4 : 0));      // [CTK_STD_STAGE][TILE]
    const int px = (int)threadIdx.x % TILE, s = (int)threadIdx.x / TILE;
    const int64_t pb = (int64_t)blockIdx.x * TILE + px;
    const bool live = pb < nband;
    const VT *col = x + p0 + (live ? pb : 0);

    CTK_STD_OWNED(0, planes, { acc_s[h * TILE + px] = 0.0; acc_q[h * TILE + px] = 0.0; if (SKIPNA) acc_n[h * TILE + px] = 0u; })
    std_pass<VT, TILE, SKIPNA, NARROW, 0>(col, live, npix, T, first, planes, W, acc_s, acc_q, acc_n, stage, px, s);
    CTK_STD_OWNED(0, planes, { acc_s[h * TILE + px] = acc_s[h * TILE + px] / (double)(SKIPNA ? acc_n[h * TILE + px] : (uint32_t)plen[h]); })
    std_pass<VT, TILE, SKIPNA, NARROW, 1>(col, live, npix, T, first, planes, W, acc_s, acc_q, acc_n, stage, px, s);
    if (!live) return;                                                         // (no barrier below)
    CTK_STD_OWNED(0, planes, {
        const uint32_t c = SKIPNA ? acc_n[h * TILE + px] : (uint32_t)plen[h];
        const int64_t den = (int64_t)c - ddof;
        const int64_t o = (int64_t)h * nband + pb;
        out_std[o] = den > 0 ? sqrt(acc_q[h * TILE + px] / (double)den) : __builtin_nan("");
        if (out_mean) out_mean[o] = acc_s[h * TILE + px];
        if (out_n) out_n[o] = c;
    })
}
#undef CTK_STD_OWNED

// out[g][i] = out[0][i], 1 <= g < G
template <typename V>
__global__ __launch_bounds__(256) void k_std_replicate(V *__restrict__ out, int64_t nband, int G)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nband) return;
    const V v = out[i];
    for (int g = 1 + (int)blockIdx.y; g < G; g += (int)gridDim.y) out[(int64_t)g * nband + i] = v;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
struct StdArgs {
    PctlArgs a; int ddof, skipna;
};
struct StdPrep {
    std::vector<int32_t> first, plen;      // per timestep the first of the `window` planes it feeds (padded with 0 to whole staged rounds); pool length per plane
    int planes = 1, window = 1;            // what the kernel walks: (G, W), or (1, 1) when the window covers every group
    int64_t max_pool = 0;
};

static int std_validate(const ctk_handle *h, const StdArgs &sa, const double *out_std, const char *name)
{
    const PctlArgs &a = sa.a;
    CTKCHK(pctl_validate_common(h, a, out_std, name));
    if (sa.ddof < 0) return ctk_set_error(CTK_E_INVALID, "%s: ddof=%d (at least 0)", name, sa.ddof);
    const CtkStdPlan f = ctk_std_plan(a.ngroups, a.window, sa.skipna);
    if (!f.tile)
        return ctk_set_error(CTK_E_INVALID, "%s: %d groups with a window of %d: at most %lld groups fit %s", name, a.ngroups, a.window, (long long)f.max_groups,
                             sa.skipna ? "with counts (skipna)" : "without counts");
    const int64_t tiles = (a.nband() + CTK_STD_MIN_TILE - 1) / CTK_STD_MIN_TILE;
    if (tiles > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: a band of %lld values is too large", name, (long long)a.nband());
    return CTK_OK;
}

static size_t std_padded(int64_t T) { return (size_t)((T + CTK_STD_STAGE - 1) / CTK_STD_STAGE) * CTK_STD_STAGE; }

static void std_prepare(const PctlArgs &a, StdPrep &p)
{
    const int G = a.ngroups, W = a.window;
    const int64_t T = a.T;
    if (W >= G) {
        p.planes = 1; p.window = 1;
        p.first.assign(std_padded(T), 0);
        p.plen.assign(1, (int32_t)T);
        p.max_pool = T;
        return;
    }
    p.planes = G; p.window = W;
    p.first.assign(std_padded(T), 0);                                          // a step of group m feeds the planes m - (W - 1) / 2 .. + W - 1 (mod G)
    for (int64_t t = 0; t < T; t++) p.first[(size_t)t] = (a.group[t] - (W - 1) / 2 + G) % G;
    std::vector<int64_t> steps((size_t)G, 0);
    for (int64_t t = 0; t < T; t++) steps[(size_t)a.group[t]]++;
    p.plen.resize((size_t)G);
    p.max_pool = 0;
    for (int g = 0; g < G; g++) {
        int64_t n = 0;
        for (int d = -(W / 2); d <= (W - 1) / 2; d++) n += steps[(size_t)(((g + d) % G + G) % G)];
        p.plen[(size_t)g] = (int32_t)n;
        p.max_pool = std::max(p.max_pool, n);
    }
}

template <typename VT, int TILE, bool SKIPNA, bool NARROW>
static int std_launch_tile(ctk_handle *h, const VT *x_dev, const StdArgs &sa, const StdPrep &p, const CtkStdPlan &f, const int32_t *first, const int32_t *plen,
                           double *o_std, double *o_mean, uint32_t *o_n)
{
    const PctlArgs &a = sa.a;
    const int64_t nband = a.nband();
    // (a launch may ask for more than 64 KB of dynamic LDS only after this.  The attribute belongs to the function, that is to every
    // handle and host thread of the process: it is always set to the one constant ctk_std_plan never exceeds, so the order in which
    // two threads set it cannot matter)
    static_assert(CTK_STD_LDS_BYTES <= 0x7fffffff, "the attribute is an int");
    if (f.lds_bytes > CTK_STD_LDS_BYTES) return ctk_set_error(CTK_E_INTERNAL, "k_std_field: a plan of %lld bytes of LDS (at most %d)", (long long)f.lds_bytes, CTK_STD_LDS_BYTES);
    HIPCHK(hipFuncSetAttribute((const void *)k_std_field<VT, TILE, SKIPNA, NARROW>, hipFuncAttributeMaxDynamicSharedMemorySize, CTK_STD_LDS_BYTES));
    k_std_field<VT, TILE, SKIPNA, NARROW><<<(unsigned)((nband + TILE - 1) / TILE), CTK_STD_THREADS, (size_t)f.lds_bytes, h->stream>>>(
        x_dev, a.npix(), a.p0(), nband, (int)a.T, first, plen, p.planes, p.window, sa.ddof, o_std, o_mean, o_n);
    return CTK_OK;
}

// the whole field on a slab in device memory, on the handle's stream; the planes are left in device memory (h->sf_out: std, then the
// mean if want_mean, then the counts if want_n)
template <typename VT>
static int std_launch(ctk_handle *h, const VT *x_dev, const StdArgs &sa, const StdPrep &p, bool want_mean, bool want_n)
{
    hipStream_t s = h->stream;
    const PctlArgs &a = sa.a;
    const int G = a.ngroups;
    const int64_t nband = a.nband();
    const CtkStdPlan f = ctk_std_plan(G, a.window, sa.skipna);
    const size_t plane_vals = (size_t)G * (size_t)nband;
    CTKCHK(ensure(h, h->sf_out, plane_vals * (8 + (want_mean ? 8 : 0) + (want_n ? 4 : 0))));
    CTKCHK(ensure(h, h->sf_idx, (p.first.size() + (size_t)p.planes) * 4));
    int32_t *first = P<int32_t>(h->sf_idx), *plen = first + p.first.size();
    HIPCHK(hipMemcpyAsync(first, p.first.data(), p.first.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(plen, p.plen.data(), (size_t)p.planes * 4, hipMemcpyHostToDevice, s));
    double *o_std = P<double>(h->sf_out), *o_mean = want_mean ? o_std + plane_vals : nullptr;
    uint32_t *o_n = want_n ? (uint32_t *)(o_std + plane_vals * (want_mean ? 2 : 1)) : nullptr;
#define CTK_STD_LAUNCH2(TILE, SKIPNA)                                                                                                   \
    CTKCHK((p.window <= CTK_STD_THREADS / TILE ? std_launch_tile<VT, TILE, SKIPNA, true>(h, x_dev, sa, p, f, first, plen, o_std, o_mean, o_n)      \
                                               : std_launch_tile<VT, TILE, SKIPNA, false>(h, x_dev, sa, p, f, first, plen, o_std, o_mean, o_n)))
#define CTK_STD_LAUNCH(TILE) do { if (sa.skipna) CTK_STD_LAUNCH2(TILE, true); else CTK_STD_LAUNCH2(TILE, false); } while (0)
    if (f.tile == 32) CTK_STD_LAUNCH(32); else if (f.tile == 16) CTK_STD_LAUNCH(16); else CTK_STD_LAUNCH(8);
#undef CTK_STD_LAUNCH2
#undef CTK_STD_LAUNCH
    if (p.planes < G) {
        const dim3 grid((unsigned)((nband + 255) / 256), (unsigned)std::min(G - 1, 64));
        k_std_replicate<double><<<grid, 256, 0, s>>>(o_std, nband, G);
        if (o_mean) k_std_replicate<double><<<grid, 256, 0, s>>>(o_mean, nband, G);
        if (o_n) k_std_replicate<uint32_t><<<grid, 256, 0, s>>>(o_n, nband, G);
    }
    HIPCHK(hipGetLastError());
    h->sf_tile = f.tile; h->sf_max_pool = p.max_pool;
    return CTK_OK;
}

template <typename VT>
static int std_field_impl(ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                          int ddof, int skipna, double *out_std, double *out_mean, uint32_t *out_n)
{
    const StdArgs sa = {{T, ny, nx, y0, y1, group, ngroups, window, 0.5}, ddof, skipna != 0};
    CTKCHK(std_validate(h, sa, out_std, "ctk_std_field"));
    HIPCHK(hipSetDevice(h->device));
    const VT *x_dev;
    CTKCHK(pctl_slab(h, x_host, T, ny, nx, "ctk_std_field", &x_dev));
    StdPrep prep;
    std_prepare(sa.a, prep);
    CTKCHK((std_launch<VT>(h, x_dev, sa, prep, out_mean != nullptr, out_n != nullptr)));
    const size_t plane_vals = (size_t)ngroups * (size_t)sa.a.nband();
    const double *d_std = P<double>(h->sf_out);
    HIPCHK(hipMemcpyAsync(out_std, d_std, plane_vals * 8, hipMemcpyDeviceToHost, h->stream));
    if (out_mean) HIPCHK(hipMemcpyAsync(out_mean, d_std + plane_vals, plane_vals * 8, hipMemcpyDeviceToHost, h->stream));
    if (out_n) HIPCHK(hipMemcpyAsync(out_n, d_std + plane_vals * (out_mean ? 2 : 1), plane_vals * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_std_field_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                 int ddof, int skipna, double *out_std, double *out_mean, uint32_t *out_n)
{
    return std_field_impl<float>(h, x, T, ny, nx, y0, y1, group, ngroups, window, ddof, skipna, out_std, out_mean, out_n);
}
extern "C" int ctk_std_field_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                 int ddof, int skipna, double *out_std, double *out_mean, uint32_t *out_n)
{
    return std_field_impl<double>(h, x, T, ny, nx, y0, y1, group, ngroups, window, ddof, skipna, out_std, out_mean, out_n);
}

// what ctk_std_plan decides (host only, no device): out4 = { pixel tile (0: does not fit), planes, dynamic LDS bytes, largest ngroups }
extern "C" int ctk_debug_std_field_plan(int ngroups, int window, int skipna, int64_t *out4)
{
    if (!out4 || ngroups < 1 || window < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_std_field_plan: bad arguments");
    const CtkStdPlan f = ctk_std_plan(ngroups, window, skipna != 0);
    out4[0] = f.tile; out4[1] = f.planes; out4[2] = f.lds_bytes; out4[3] = f.max_groups;
    return CTK_OK;
}

// test hook: out2 = { pixel tile of the last ctk_std_field_* call on this handle (-1: none), its longest pool in timesteps }
extern "C" int ctk_debug_std_field_form(ctk_handle *h, int64_t *out2)
{
    if (!h || !out2) return ctk_set_error(CTK_E_INVALID, "null argument");
    out2[0] = h->sf_tile; out2[1] = h->sf_max_pool;
    return CTK_OK;
}

// measurement (tools/std_probe.py, profiles/NOTES.md) on a slab in device memory (is_f64: float64): ms2 = { ctk_std_field's device
// work per call (best of reps, host clock around the upload of the ids, every kernel and the synchronisation; the download of the
// field is outside), the pixel tile }.  out_std (may be NULL): the field.
extern "C" int ctk_debug_time_std_field(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group,
                                        int ngroups, int window, int ddof, int skipna, int reps, double *out_std, double *ms2)
{
    const StdArgs sa = {{T, ny, nx, y0, y1, group, ngroups, window, 0.5}, ddof, skipna != 0};
    double dummy = 0;
    CTKCHK(std_validate(h, sa, &dummy, "ctk_debug_time_std_field"));
    if (!x_dev || !ms2 || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_std_field: null buffer or reps < 1");
    HIPCHK(hipSetDevice(h->device));
    StdPrep prep;
    std_prepare(sa.a, prep);
    double best = 1e30;
    for (int r = 0; r <= reps; r++) {                                          // (the first call grows the buffers)
        const double t0 = now_ms();
        if (is_f64) CTKCHK((std_launch<double>(h, (const double *)x_dev, sa, prep, false, false)));
        else CTKCHK((std_launch<float>(h, (const float *)x_dev, sa, prep, false, false)));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (r) best = std::min(best, now_ms() - t0);
    }
    ms2[0] = best; ms2[1] = (double)h->sf_tile;
    if (out_std) HIPCHK(hipMemcpy(out_std, h->sf_out.p, (size_t)ngroups * (size_t)sa.a.nband() * 8, hipMemcpyDeviceToHost));
    return CTK_OK;
}
