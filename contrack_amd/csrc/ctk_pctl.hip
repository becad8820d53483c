// ctk_pctl.hip -- the percentile threshold per calendar day of the reference's tutorial on the device (included by ctk_api.hip):
//     "a variable PV intensity threshold defined as the 10th percentile of the PV anomaly distribution over 30-90N at each
//      calendar day"                                                         README.rst:235-240, consumed by contrack.py:648-661
// For every group g (calendar day) the exact q-quantile (np.nanquantile, method 'linear', in float64) of the POOL of all values of
// rows [y0, y1) on every timestep whose group lies in the centred window of W groups around g, taken circularly over the G groups:
//     pool(g) = { x[t, y, :] : y0 <= y < y1, group[t] in { (g + d) mod G : -(W / 2) <= d <= (W - 1) / 2 } }
//
// Radix selection on the order-preserving keys of an_key (ctk_select.h), for all groups at once.  Histograms are additive over days:
//   k_pctl_sweep   one read of the band per digit.  A workgroup takes CTK_PCTL_CHUNK values of ONE timestep, so its day d is
//                  uniform; it counts the digit in LDS and adds the nonzero bins to the histograms of its day in HBM.  From the second
//                  digit on a value counts only under a prefix one of the day's TARGETS (the groups whose window holds d) has
//                  selected: the distinct prefixes of the targets, sorted (k_pctl_lists), are searched in LDS -- neighbouring days
//                  mostly share them -- and the histograms are per (day, distinct prefix), not per target.
//   k_pctl_select  per group: sums the histograms of its window's days under its own prefix (64-bit), finds the bin that holds rank
//                  floor((n - 1) q) and extends the prefix.  After the last digit the prefix is the selected key; the number of
//                  values <= it and, where another key shares its upper digits, the next larger key come from the same histogram.
//   k_pctl_close   the closing sweep, for the groups whose next larger key lies under another prefix: per (day, distinct selected
//                  key s) the smallest key above s.  Workgroups of a day none of whose targets needs it return before reading.
//   k_pctl_finish  numpy's interpolation (an_np_quantile, shared with pf_select).
// The band is read once per sweep: ctk_pctl_form().sweeps times per call (4 for float32, 7 for float64), whatever G and W are.
// Window sums, ranks and n are 64-bit; the per-day counters are uint32 behind the host check ctk_pctl_day_fits.
#pragma once

typedef float ctk_f32x4 __attribute__((ext_vector_type(4)));
typedef double ctk_f64x2 __attribute__((ext_vector_type(2)));

// fn(v) for every value of base[0 .. len): 16-byte loads from the first aligned address on, four in flight per lane
template <typename F>
__device__ __forceinline__ void pctl_stream(const float *base, int64_t len, F fn)
{
    const int tid = (int)threadIdx.x;
    const int64_t mis = (int64_t)((16 - ((uintptr_t)base & 15)) & 15) / 4, head = mis < len ? mis : len;
    if (tid < head) fn(base[tid]);
    const ctk_f32x4 *v = (const ctk_f32x4 *)(base + head);
    const int64_t nv = (len - head) / 4;
    int64_t i = tid;
    for (; i + 768 < nv; i += 1024) {
        const ctk_f32x4 a = v[i], b = v[i + 256], c = v[i + 512], d = v[i + 768];
        fn(a.x); fn(a.y); fn(a.z); fn(a.w); fn(b.x); fn(b.y); fn(b.z); fn(b.w);
        fn(c.x); fn(c.y); fn(c.z); fn(c.w); fn(d.x); fn(d.y); fn(d.z); fn(d.w);
    }
    for (; i < nv; i += 256) { const ctk_f32x4 a = v[i]; fn(a.x); fn(a.y); fn(a.z); fn(a.w); }
    const int64_t done = head + nv * 4;
    if (done + tid < len) fn(base[done + tid]);
}
template <typename F>
__device__ __forceinline__ void pctl_stream(const double *base, int64_t len, F fn)
{
    const int tid = (int)threadIdx.x;
    const int64_t mis = ((uintptr_t)base & 15) ? 1 : 0, head = mis < len ? mis : len;
    if (tid < head) fn(base[tid]);
    const ctk_f64x2 *v = (const ctk_f64x2 *)(base + head);
    const int64_t nv = (len - head) / 2;
    int64_t i = tid;
    for (; i + 768 < nv; i += 1024) {
        const ctk_f64x2 a = v[i], b = v[i + 256], c = v[i + 512], d = v[i + 768];
        fn(a.x); fn(a.y); fn(b.x); fn(b.y); fn(c.x); fn(c.y); fn(d.x); fn(d.y);
    }
    for (; i < nv; i += 256) { const ctk_f64x2 a = v[i]; fn(a.x); fn(a.y); }
    const int64_t done = head + nv * 2;
    if (done + tid < len) fn(base[done + tid]);
}

// the window of group g: `cnt` members, member j is (start + j) mod G.  mirrored: the TARGETS of day g (the groups whose window holds it)
__device__ __forceinline__ void pctl_window(int g, int G, int W, bool mirrored, int *start, int *cnt)
{
    if (W >= G) { *start = 0; *cnt = G; return; }
    const int back = mirrored ? (W - 1) / 2 : W / 2;
    *start = ((g - back) % G + G) % G;
    *cnt = W;
}

// slot of prefix `want` among the sorted distinct prefixes of a day (it is there: the asking group is a target of the day)
__device__ __forceinline__ int pctl_slot(const uint64_t *__restrict__ dl, int nu, uint64_t want)
{
    int lo = 0, hi = nu - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (dl[mid] < want) lo = mid + 1; else hi = mid; }
    return lo;
}

// zero the histogram slots in use (slot u of day d, u < nu[d]; first: one slot per day)
__global__ __launch_bounds__(256) void k_pctl_zero(uint32_t *__restrict__ hist, const uint32_t *__restrict__ nu, int stride, int first)
{
    const int d = (int)blockIdx.x, u = (int)blockIdx.y;
    if ((uint32_t)u >= (first ? 1u : nu[d])) return;
    const int64_t s = (int64_t)d * stride + u;
    uint4 *p = (uint4 *)(hist + s * CTK_PCTL_BINS);
    for (int i = (int)threadIdx.x; i < CTK_PCTL_BINS / 4; i += 256) p[i] = make_uint4(0, 0, 0, 0);
}

template <typename VT, typename KT, bool FIRST>
__global__ __launch_bounds__(256) void k_pctl_sweep(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int64_t chunk, const int32_t *__restrict__ group,
                                                    int stride, int shift, int bits, const uint32_t *__restrict__ nu_day, const uint64_t *__restrict__ dl,
                                                    uint32_t *__restrict__ hist)
{
    constexpr int NS = FIRST ? 1 : CTK_PCTL_LDS_SLOTS;
    __shared__ uint32_t lh[NS][CTK_PCTL_BINS];
    __shared__ KT s_dl[FIRST ? 1 : CTK_PCTL_MAX_WINDOW];
    const int64_t t = blockIdx.x, c0 = (int64_t)blockIdx.y * chunk;
    const int d = group[t];
    const int nu = FIRST ? 1 : (int)nu_day[d], nl = min(nu, NS), nbins = 1 << bits;
    const int64_t slot0 = (int64_t)d * stride;
    if (!FIRST) for (int i = (int)threadIdx.x; i < nu; i += 256) s_dl[i] = (KT)dl[slot0 + i];
    for (int i = (int)threadIdx.x; i < nl * CTK_PCTL_BINS; i += 256) (&lh[0][0])[i] = 0;
    __syncthreads();
    const uint32_t dmask = (uint32_t)nbins - 1u;
    pctl_stream(x + t * npix + p0 + c0, min(chunk, nband - c0), [&](VT v) {
        if (an_isnan(v)) return;                                               // (np.nanquantile)
        const KT k = an_key(v);
        const uint32_t dig = (uint32_t)(k >> shift) & dmask;
        int u = 0;
        if constexpr (!FIRST) {
            const KT up = k >> (shift + bits);
            if (up < s_dl[0] || up > s_dl[nu - 1]) return;
            int lo = 0, hi = nu - 1;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_dl[mid] < up) lo = mid + 1; else hi = mid; }
            if (s_dl[lo] != up) return;
            u = lo;
        }
        if (u < NS) atomicAdd(&lh[u][dig], 1u);
        else atomicAdd(&hist[(slot0 + u) * CTK_PCTL_BINS + dig], 1u);
    });
    __syncthreads();
    for (int u = 0; u < nl; u++)
        for (int i = (int)threadIdx.x; i < nbins; i += 256) {
            const uint32_t c = lh[u][i];
            if (c) atomicAdd(&hist[(slot0 + u) * CTK_PCTL_BINS + i], c);
        }
}

// per group: window histogram under its prefix, the bin of its rank, the longer prefix; LAST: le, the next key where the histogram has it
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_pctl_select(int G, int W, int stride, int bits, double q, const uint32_t *__restrict__ nu_day, const uint64_t *__restrict__ dl,
                                                     const uint32_t *__restrict__ hist, uint64_t *__restrict__ n_of, uint64_t *__restrict__ krem, uint64_t *__restrict__ prefix,
                                                     uint64_t *__restrict__ le_of, uint64_t *__restrict__ next_of, uint32_t *__restrict__ need)
{
    __shared__ uint64_t s_cnt[CTK_PCTL_BINS];
    const int g = (int)blockIdx.x, nbins = 1 << bits;
    if (!FIRST && n_of[g] == 0) return;
    const uint64_t pre = FIRST ? 0 : prefix[g];
    uint64_t acc[CTK_PCTL_BINS / 256];
#pragma unroll
    for (int j = 0; j < CTK_PCTL_BINS / 256; j++) acc[j] = 0;
    int start, cnt;
    pctl_window(g, G, W, false, &start, &cnt);
    for (int m = 0; m < cnt; m++) {
        int d = start + m; if (d >= G) d -= G;
        const int64_t slot0 = (int64_t)d * stride;
        const int nu = FIRST ? 1 : (int)nu_day[d];
        const int u = nu > 1 ? pctl_slot(dl + slot0, nu, pre) : 0;
        const uint32_t *hh = hist + (slot0 + u) * CTK_PCTL_BINS;
#pragma unroll
        for (int j = 0; j < CTK_PCTL_BINS / 256; j++) { const int i = (int)threadIdx.x + 256 * j; if (i < nbins) acc[j] += hh[i]; }
    }
#pragma unroll
    for (int j = 0; j < CTK_PCTL_BINS / 256; j++) s_cnt[threadIdx.x + 256 * j] = acc[j];
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint64_t n = 0;
    if (FIRST) {
        for (int i = 0; i < nbins; i++) n += s_cnt[i];
        n_of[g] = n;
        prefix[g] = 0;
        need[g] = 0;
        if (n == 0) return;
    } else n = n_of[g];
    const uint64_t k0 = (uint64_t)floor(((double)n - 1.0) * q);
    const uint64_t k = FIRST ? k0 : krem[g];
    uint64_t cum = 0;
    int bin = 0;
    for (; bin < nbins - 1; bin++) { if (cum + s_cnt[bin] > k) break; cum += s_cnt[bin]; }
    const uint64_t sel = (pre << bits) | (uint64_t)bin;
    prefix[g] = sel;
    krem[g] = k - cum;
    if (LAST) {
        const uint64_t le = (k0 - (k - cum)) + s_cnt[bin];
        uint64_t nx = ~0ull;
        for (int b = bin + 1; b < nbins; b++) if (s_cnt[b]) { nx = (pre << bits) | (uint64_t)b; break; }
        le_of[g] = le;
        next_of[g] = nx;
        need[g] = (nx == ~0ull && le == k0 + 1 && k0 + 1 < n) ? 1u : 0u;
    }
}

// per day: the sorted distinct prefixes of its targets; mins (after the last digit): the closing sweep's minima start at 'none'
__global__ __launch_bounds__(256) void k_pctl_lists(int G, int W, int stride, const uint64_t *__restrict__ prefix, uint32_t *__restrict__ nu_day, uint64_t *__restrict__ dl,
                                                   uint64_t *__restrict__ mins)
{
    __shared__ uint64_t s_p[CTK_PCTL_MAX_WINDOW];
    __shared__ uint32_t s_first[CTK_PCTL_MAX_WINDOW];
    __shared__ uint32_t s_nu;
    const int d = (int)blockIdx.x;
    if (mins) for (int j = (int)threadIdx.x; j < stride; j += 256) mins[(int64_t)d * stride + j] = ~0ull;
    if (W >= G) {                                                              // every group pools every day: one prefix
        if (threadIdx.x == 0) { nu_day[d] = 1; dl[d] = prefix[0]; }
        return;
    }
    int start, cnt;
    pctl_window(d, G, W, true, &start, &cnt);
    if (threadIdx.x == 0) s_nu = 0;
    for (int j = (int)threadIdx.x; j < cnt; j += 256) s_p[j] = prefix[(start + j) % G];
    __syncthreads();
    for (int j = (int)threadIdx.x; j < cnt; j += 256) {
        uint32_t first = 1;
        for (int i = 0; i < j; i++) if (s_p[i] == s_p[j]) { first = 0; break; }
        s_first[j] = first;
    }
    __syncthreads();
    for (int j = (int)threadIdx.x; j < cnt; j += 256) {
        if (!s_first[j]) continue;
        int r = 0;
        for (int i = 0; i < cnt; i++) r += (s_first[i] && s_p[i] < s_p[j]) ? 1 : 0;
        dl[(int64_t)d * stride + r] = s_p[j];
        atomicAdd(&s_nu, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) nu_day[d] = s_nu;
}

// closing sweep: mins[day][i] = the smallest key of the day above its i-th distinct selected key and not above the (i+1)-th
// (k_pctl_finish takes the minimum over i' >= i)
template <typename VT, typename KT>
__global__ __launch_bounds__(256) void k_pctl_close(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int64_t chunk, const int32_t *__restrict__ group,
                                                    int G, int W, int stride, const uint32_t *__restrict__ nu_day, const uint64_t *__restrict__ dl,
                                                    const uint32_t *__restrict__ need, uint64_t *__restrict__ mins)
{
    __shared__ KT s_dl[CTK_PCTL_MAX_WINDOW], s_min[CTK_PCTL_MAX_WINDOW];
    __shared__ uint32_t s_any;
    const int64_t t = blockIdx.x, c0 = (int64_t)blockIdx.y * chunk;
    const int d = group[t];
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    int start, cnt;
    pctl_window(d, G, W, true, &start, &cnt);
    {
        uint32_t any = 0;
        for (int j = (int)threadIdx.x; j < cnt; j += 256) any |= need[(start + j) % G];
        if (any) s_any = 1;
    }
    __syncthreads();
    if (!s_any) return;
    const int nu = (int)nu_day[d];
    const int64_t slot0 = (int64_t)d * stride;
    for (int i = (int)threadIdx.x; i < nu; i += 256) { s_dl[i] = (KT)dl[slot0 + i]; s_min[i] = ~(KT)0; }
    __syncthreads();
    pctl_stream(x + t * npix + p0 + c0, min(chunk, nband - c0), [&](VT v) {
        if (an_isnan(v)) return;
        const KT k = an_key(v);
        if (k <= s_dl[0]) return;
        int lo = 0, hi = nu - 1;                                               // the last selected key below k
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_dl[mid] < k) lo = mid; else hi = mid - 1; }
        if (k < s_min[lo]) pctl_atomic_min(&s_min[lo], k);
    });
    __syncthreads();
    for (int i = (int)threadIdx.x; i < nu; i += 256)
        if (s_min[i] != ~(KT)0) pctl_atomic_min(&mins[slot0 + i], (uint64_t)s_min[i]);
}

template <typename VT, typename KT>
__global__ __launch_bounds__(256) void k_pctl_finish(int G, int W, int stride, double q, const uint32_t *__restrict__ nu_day, const uint64_t *__restrict__ dl,
                                                     const uint64_t *__restrict__ n_of, const uint64_t *__restrict__ prefix, const uint64_t *__restrict__ le_of,
                                                     const uint64_t *__restrict__ next_of, const uint32_t *__restrict__ need, const uint64_t *__restrict__ mins,
                                                     double *__restrict__ out)
{
    const int g = (int)(blockIdx.x * 256 + threadIdx.x);
    if (g >= G) return;
    const uint64_t n = n_of[g];
    if (n == 0) { out[g] = __builtin_nan(""); return; }
    const uint64_t sel = prefix[g];
    uint64_t nx = next_of[g];
    if (need[g]) {
        int start, cnt;
        pctl_window(g, G, W, false, &start, &cnt);
        for (int m = 0; m < cnt; m++) {
            int d = start + m; if (d >= G) d -= G;
            const int64_t slot0 = (int64_t)d * stride;
            const int nu = (int)nu_day[d];
            for (int i = nu > 1 ? pctl_slot(dl + slot0, nu, sel) : 0; i < nu; i++) { const uint64_t m2 = mins[slot0 + i]; if (m2 < nx) nx = m2; }
        }
    }
    const double a = (double)an_unkey((KT)sel);
    out[g] = an_np_quantile(n, q, a, nx == ~0ull ? a : (double)an_unkey((KT)nx), le_of[g]);
}

// a plain 16-byte read stream over the same band with the sweeps' grid: the floor a sweep is compared against
template <typename VT, typename KT>
__global__ __launch_bounds__(256) void k_pctl_read(const VT *__restrict__ x, int64_t npix, int64_t p0, int64_t nband, int64_t chunk, uint64_t *__restrict__ sink)
{
    const int64_t t = blockIdx.x, c0 = (int64_t)blockIdx.y * chunk;
    KT acc = 0;
    pctl_stream(x + t * npix + p0 + c0, min(chunk, nband - c0), [&](VT v) { acc ^= an_key(v); });
    if (acc == (KT)0x5a5a5a5a) sink[0] = (uint64_t)acc;                       // (keeps the loads alive)
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int pctl_validate(const ctk_handle *h, const PctlArgs &a, const double *out, const char *name)
{
    CTKCHK(pctl_validate_common(h, a, out, name));
    std::vector<int64_t> steps((size_t)a.ngroups, 0);
    for (int64_t t = 0; t < a.T; t++) steps[(size_t)a.group[t]]++;
    const int gmax = (int)(std::max_element(steps.begin(), steps.end()) - steps.begin());
    const int64_t nband = a.nband();
    switch (ctk_pctl_refusal(nband, a.ngroups, a.window, steps[(size_t)gmax])) {               // (the size rules: ctk_forms.h)
    case CTK_PCTL_REFUSE_WINDOW:
        return ctk_set_error(CTK_E_INVALID, "%s: a window of %d groups (below the %d groups) exceeds %d", name, a.window, a.ngroups, CTK_PCTL_MAX_WINDOW);
    case CTK_PCTL_REFUSE_SLOTS:
        return ctk_set_error(CTK_E_INVALID, "%s: %d groups x a window of %d need %lld histograms of 8 KB, more than the %lld (4 GB) this entry takes", name, a.ngroups,
                             a.window, (long long)a.ngroups * ctk_pctl_form(32, nband, a.ngroups, a.window).stride, (long long)CTK_PCTL_MAX_SLOTS);
    case CTK_PCTL_REFUSE_BAND: return ctk_set_error(CTK_E_INVALID, "%s: a band of %lld values is too large", name, (long long)nband);
    case CTK_PCTL_REFUSE_DAY:
        return ctk_set_error(CTK_E_INVALID, "%s: group %d has %lld timesteps of %lld band values: its uint32 counters would overflow (2^32)", name, gmax,
                             (long long)steps[(size_t)gmax], (long long)nband);
    default: break;
    }
    return CTK_OK;
}

// the whole selection on a slab in device memory, on the handle's stream; the G results are left in device memory (*out_dev).
// ev (measurement): events recorded before (ev[2 i]) and after (ev[2 i + 1]) band sweep i
template <typename VT, typename KT>
static int pctl_launch(ctk_handle *h, const VT *x_dev, const PctlArgs &a, const double **out_dev, const Event *ev = nullptr)
{
    hipStream_t s = h->stream;
    const int G = a.ngroups, W = a.window;
    const int64_t npix = a.npix(), nband = a.nband(), p0 = a.p0();
    const CtkPctlForm f = ctk_pctl_form((int)sizeof(KT) * 8, nband, G, W);
    const size_t slots = (size_t)G * (size_t)f.stride;
    CTKCHK(ensure(h, h->pc_hist, slots * CTK_PCTL_BINS * 4));
    // [n | krem | prefix | le | next | out] x G u64, the read probe's sink, [dl | mins] x slots u64, [nu | need] x G u32, group x T i32
    CTKCHK(ensure(h, h->pc_buf, ((size_t)6 * G + 1 + 2 * slots) * 8 + ((size_t)2 * G + (size_t)a.T) * 4));
    uint64_t *n_of = P<uint64_t>(h->pc_buf), *krem = n_of + G, *prefix = krem + G, *le_of = prefix + G, *next_of = le_of + G;
    double *out = (double *)(next_of + G);
    uint64_t *dl = (uint64_t *)(out + G) + 1, *mins = dl + slots;
    uint32_t *nu = (uint32_t *)(mins + slots), *need = nu + G;
    int32_t *grp = (int32_t *)(need + G);
    HIPCHK(hipMemcpyAsync(grp, a.group, (size_t)a.T * 4, hipMemcpyHostToDevice, s));
    uint32_t *hist = P<uint32_t>(h->pc_hist);
    const dim3 sweep_grid((unsigned)a.T, f.chunks), zero_grid((unsigned)G, (unsigned)f.stride);
    h->pc_sweeps = 0;
    h->pc_groups = G; h->pc_slots = slots;                                     // (ctk_debug_percentile_groups_state reads pc_buf by them)
    for (int l = 0; l < f.levels; l++) {
        const bool first = l == 0, last = l == f.levels - 1;
        k_pctl_zero<<<zero_grid, 256, 0, s>>>(hist, nu, f.stride, first ? 1 : 0);
        if (ev) HIPCHK(hipEventRecord(ev[2 * l], s));
        if (first) k_pctl_sweep<VT, KT, true><<<sweep_grid, 256, 0, s>>>(x_dev, npix, p0, nband, f.chunk, grp, f.stride, f.shift[l], f.bits[l], nu, dl, hist);
        else k_pctl_sweep<VT, KT, false><<<sweep_grid, 256, 0, s>>>(x_dev, npix, p0, nband, f.chunk, grp, f.stride, f.shift[l], f.bits[l], nu, dl, hist);
        h->pc_sweeps++;
        if (ev) HIPCHK(hipEventRecord(ev[2 * l + 1], s));
        if (first) k_pctl_select<true, false><<<G, 256, 0, s>>>(G, W, f.stride, f.bits[l], a.q, nu, dl, hist, n_of, krem, prefix, le_of, next_of, need);
        else if (!last) k_pctl_select<false, false><<<G, 256, 0, s>>>(G, W, f.stride, f.bits[l], a.q, nu, dl, hist, n_of, krem, prefix, le_of, next_of, need);
        else k_pctl_select<false, true><<<G, 256, 0, s>>>(G, W, f.stride, f.bits[l], a.q, nu, dl, hist, n_of, krem, prefix, le_of, next_of, need);
        k_pctl_lists<<<G, 256, 0, s>>>(G, W, f.stride, prefix, nu, dl, last ? mins : nullptr);
    }
    if (ev) HIPCHK(hipEventRecord(ev[2 * f.levels], s));
    k_pctl_close<VT, KT><<<sweep_grid, 256, 0, s>>>(x_dev, npix, p0, nband, f.chunk, grp, G, W, f.stride, nu, dl, need, mins);
    h->pc_sweeps++;
    if (ev) HIPCHK(hipEventRecord(ev[2 * f.levels + 1], s));
    k_pctl_finish<VT, KT><<<(unsigned)((G + 255) / 256), 256, 0, s>>>(G, W, f.stride, a.q, nu, dl, n_of, prefix, le_of, next_of, need, mins, out);
    HIPCHK(hipGetLastError());
    *out_dev = out;
    return CTK_OK;
}

template <typename VT, typename KT>
static int percentile_groups_impl(ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                  double q, double *out)
{
    const PctlArgs a = {T, ny, nx, y0, y1, group, ngroups, window, q};
    CTKCHK(pctl_validate(h, a, out, "ctk_percentile_groups"));
    HIPCHK(hipSetDevice(h->device));
    const VT *x_dev;
    CTKCHK(pctl_slab(h, x_host, T, ny, nx, "ctk_percentile_groups", &x_dev));
    const double *out_dev = nullptr;
    CTKCHK((pctl_launch<VT, KT>(h, x_dev, a, &out_dev)));
    HIPCHK(hipMemcpyAsync(out, out_dev, (size_t)ngroups * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_percentile_groups_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                         double q, double *out)
{
    return percentile_groups_impl<float, uint32_t>(h, x, T, ny, nx, y0, y1, group, ngroups, window, q, out);
}
extern "C" int ctk_percentile_groups_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups, int window,
                                         double q, double *out)
{
    return percentile_groups_impl<double, uint64_t>(h, x, T, ny, nx, y0, y1, group, ngroups, window, q, out);
}

// test hook: band sweeps (k_pctl_sweep and k_pctl_close launches) of the last ctk_percentile_groups_* call on this handle
extern "C" int ctk_debug_percentile_groups_sweeps(ctk_handle *h, int64_t *sweeps)
{
    if (!h || !sweeps) return ctk_set_error(CTK_E_INVALID, "null argument");
    *sweeps = h->pc_sweeps;
    return CTK_OK;
}

// test hook, no handle, no device: the plan of ctk_pctl_form and the refusal of ctk_pctl_refusal (ctk_forms.h) for keys of `keybits`
// bits, a band of nband values, ngroups, window and the most timesteps a group owns.  out22 = { levels, sweeps, stride, chunk, chunks,
// shift[8], bits[8] (0 beyond levels), refusal: 0 fine, 1 the window, 2 the histogram slots, 3 the band, 4 a day's counters }
extern "C" int ctk_debug_percentile_groups_plan(int keybits, int64_t nband, int ngroups, int window, int64_t max_steps_of_a_group, int64_t *out22)
{
    if (!out22 || (keybits != 32 && keybits != 64) || nband < 1 || ngroups < 1 || window < 1 || max_steps_of_a_group < 0)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_percentile_groups_plan: bad arguments");
    const CtkPctlForm f = ctk_pctl_form(keybits, nband, ngroups, window);
    out22[0] = f.levels; out22[1] = f.sweeps; out22[2] = f.stride; out22[3] = f.chunk; out22[4] = (nband + f.chunk - 1) / f.chunk;
    for (int l = 0; l < 8; l++) { out22[5 + l] = l < f.levels ? f.shift[l] : 0; out22[13 + l] = l < f.levels ? f.bits[l] : 0; }
    out22[21] = ctk_pctl_refusal(nband, ngroups, window, max_steps_of_a_group);
    return CTK_OK;
}

// test hook: what the last ctk_percentile_groups_* call on this handle left in pc_buf, per group: nu_day (the distinct selected keys of
// the day's targets, after the last k_pctl_lists), need (the closing sweep supplies the group's next larger key), n_of (its pool)
extern "C" int ctk_debug_percentile_groups_state(ctk_handle *h, int ngroups, uint32_t *nu_day, uint32_t *need, uint64_t *n_of)
{
    if (!h || !nu_day || !need || !n_of) return ctk_set_error(CTK_E_INVALID, "ctk_debug_percentile_groups_state: null argument");
    if (h->pc_groups < 1) return ctk_set_error(CTK_E_STATE, "ctk_debug_percentile_groups_state: no ctk_percentile_groups_* call has run on this handle");
    if (ngroups != h->pc_groups) return ctk_set_error(CTK_E_INVALID, "ctk_debug_percentile_groups_state: ngroups=%d, the last call had %d", ngroups, h->pc_groups);
    HIPCHK(hipSetDevice(h->device));
    const size_t G = (size_t)h->pc_groups;
    const uint64_t *n_dev = P<uint64_t>(h->pc_buf);                            // (the layout of pctl_launch)
    const uint32_t *nu_dev = (const uint32_t *)(n_dev + 6 * G + 1 + 2 * h->pc_slots);
    HIPCHK(hipMemcpyAsync(n_of, n_dev, G * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(nu_day, nu_dev, G * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(need, nu_dev + G, G * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

// measurement (tools/pctl_probe.py, profiles/NOTES.md) on a float32 slab in device memory: ms12 = { ctk_percentile_groups per call
// (best of reps, host clock around upload of the ids, every kernel, download, synchronisation), one plain 16-byte read stream over
// the band with the sweeps' grid (best of reps, HIP events), the scalar percentile's kernels (k_quantile + k_nanmean, once, HIP
// events), the band sweeps of one more call each (HIP events; [3 + i], i < sweeps), 0 beyond }; out: the G results
extern "C" int ctk_debug_time_percentile_groups(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, int y0, int y1, const int32_t *group, int ngroups,
                                                int window, double q, int reps, double *out, double *ms12)
{
    const PctlArgs a = {T, ny, nx, y0, y1, group, ngroups, window, q};
    CTKCHK(pctl_validate(h, a, out, "ctk_debug_time_percentile_groups"));
    if (!x_dev || !ms12 || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_percentile_groups: null buffer or reps < 1");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t npix = a.npix(), nband = a.nband(), p0 = a.p0();
    for (int i = 0; i < 12; i++) ms12[i] = 0;
    double best = 1e30;
    for (int r = 0; r <= reps; r++) {                                          // (the first call grows the buffers)
        const double t0 = now_ms();
        const double *out_dev = nullptr;
        CTKCHK((pctl_launch<float, uint32_t>(h, x_dev, a, &out_dev)));
        HIPCHK(hipMemcpyAsync(out, out_dev, (size_t)ngroups * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (r) best = std::min(best, now_ms() - t0);
    }
    ms12[0] = best;
    const CtkPctlForm f = ctk_pctl_form(32, nband, ngroups, window);
    Event ev[16];
    int rc = CTK_OK;
    for (Event &e : ev)
        if (rc == CTK_OK && e.create() != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventCreate failed");
    auto elapsed = [&](hipEvent_t e0, hipEvent_t e1, double *ms) {
        float m = 0;
        if (rc == CTK_OK && (hipEventSynchronize(e1) != hipSuccess || hipGetLastError() != hipSuccess || hipEventElapsedTime(&m, e0, e1) != hipSuccess))
            rc = ctk_set_error(CTK_E_NODEVICE, "ctk_debug_time_percentile_groups: a timed launch failed");
        *ms = m;
    };
    if (rc == CTK_OK) {                                                        // one more call, an event pair around every sweep
        const double *out_dev = nullptr;
        rc = pctl_launch<float, uint32_t>(h, x_dev, a, &out_dev, ev);
        for (int i = 0; i < f.sweeps && rc == CTK_OK; i++) elapsed(ev[2 * i], ev[2 * i + 1], &ms12[3 + i]);
    }
    uint64_t *sink = (uint64_t *)((double *)(P<uint64_t>(h->pc_buf) + 5 * (size_t)ngroups) + ngroups);
    best = 1e30;
    for (int r = 0; r <= reps && rc == CTK_OK; r++) {
        double m = 0;
        if (hipEventRecord(ev[0], s) != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        k_pctl_read<float, uint32_t><<<dim3((unsigned)T, f.chunks), 256, 0, s>>>(x_dev, npix, p0, nband, f.chunk, sink);
        if (rc == CTK_OK && hipEventRecord(ev[1], s) != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        elapsed(ev[0], ev[1], &m);
        if (r) best = std::min(best, m);
    }
    ms12[1] = best;
    if (rc == CTK_OK) rc = ensure(h, h->an_raw, ((size_t)nband + 8) * 8);
    if (rc == CTK_OK) {
        h->an_pct_n = -1;
        double *qv = P<double>(h->an_raw);
        if (hipEventRecord(ev[0], s) != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        launch_quantile<float, uint32_t>(h, x_dev, T, npix, p0, nband, q, qv);
        if (rc == CTK_OK && hipEventRecord(ev[1], s) != hipSuccess) rc = ctk_set_error(CTK_E_NODEVICE, "hipEventRecord failed");
        elapsed(ev[0], ev[1], &ms12[2]);
    }
    (void)hipStreamSynchronize(s);
    return rc;
}
