// ctk_filter.hip -- a weighted filter or a block mean along time (included by ctk_api.hip): the low-, high- and band-pass filters of
// the blocking literature (Lanczos weights, Duchon 1979) and the means over blocks of steps (6-hourly to daily, daily to pentads).
// include/contrack_hip.h states layout and arithmetic, tests/filter_util.py is their numpy statement.  Output q of a segment [S, E)
// has its K taps at the steps first .. first + K - 1, first = S + offset + q * stride; the taps that lie inside the segment are
// [k0, k1).  Per output and pixel, in float64, taps in rising order, the product rounded before it is added (k_band's rule):
//     weighted:  s = s + (w[i] * x[first + i])    result s, or s / (the sum of the used w[i]) where a tap is missing
//     box:       s = s + x[first + i]             result s / (the number of used taps)
//
// The host turns layout and segments into one CtkFilterTap {first, k0, k1} per output (filter_taps).  The kernels know nothing of
// segments, a tile may span a break; all they rely on is that first + k0 and first + k1 do not fall from one output to the next.
//
// k_filter_ring: one lane per pixel and tile of outputs.  The lane walks the steps from the first used tap of its tile to the last
// once and keeps the last K values of its pixel in a ring in LDS (slot k of lane l at ring[k * threads + l]: consecutive lanes,
// consecutive banks; a lane's ring is its own, so there is no barrier).  An output leaves when the step of its last used tap has
// arrived: the ring is re-added from that output's first used tap, which is the order of the statement.  x is read
// (tile * stride + K - stride) / (tile * stride) times instead of K times.
// k_filter_plain: every tap from memory, for a K whose ring does not fit in LDS and for stride >= K, where outputs share no tap
// (ctk_filter_plan, ctk_forms.h).
// Both take the slab as a window: plane 0 of `x` is step xbase; plane 0 of `out` is output o0.
//
// Weights and taps are the same for every lane of a workgroup (the tile is blockIdx.y, the tap a loop counter): they are read through
// the constant address space, which the compiler turns into scalar loads (s_load_dwordx2 / x4 in the ISA of both kernels) -- one per
// wave and tap, in the scalar cache, beside the vector memory pipe.  Staging the weights in LDS would cost the ring K * 8 bytes and
// every tap a second LDS read.
//
// Streamed (ctk_filter_f32 / _f64 / _stream_cb): the chunks pass through two windows [K - 1 steps kept from the chunk before | chunk];
// the last K - 1 steps of a window are copied in front of the next one on the device, so the reader is never asked for a step twice.
// An output leaves with the chunk that holds step first + K - 1 (whether that tap is used or not), the last chunk closes the gap.
#pragma once

struct CtkFilterTap { int64_t first; int32_t k0, k1; };
typedef const __attribute__((address_space(4))) CtkFilterTap ctk_const_tap;

// what an output becomes: s, ws the sums, n the taps that entered them, [k0, k1) the used taps
template <typename VT, bool BOX, bool SKIPNA>
__device__ __forceinline__ VT filter_result(double s, double ws, int n, int k0, int k1, int K, int edges_nan, ctk_const_f64 *w)
{
    const bool complete = k0 == 0 && k1 == K;
    if ((edges_nan && !complete) || n == 0) return (VT)__builtin_nan("");
    if (BOX) return (VT)(s / (double)n);
    if (complete && n == K) return (VT)s;
    if (!SKIPNA) for (int i = k0; i < k1; i++) ws = ws + w[i];                 // (an incomplete window: the used weights, in tap order)
    return (VT)(s / ws);
}

// `count` taps in rising order, tap t with weight w[t] and its value at v[t * step] (LDS or memory) -- the one place the sums are formed
template <typename VT, bool BOX, bool SKIPNA>
__device__ __forceinline__ void filter_taps_add(const VT *v, int64_t step, ctk_const_f64 *w, int count, double &s, double &ws, int &n)
{
#pragma unroll 4
    for (int t = 0; t < count; t++) {
        const double x = (double)v[t * step];
        if (SKIPNA && x != x) continue;
        if (BOX) s = s + x;
        else {
            const double wt = w[t], prod = wt * x;                               // (a rounded multiply, then a rounded add)
            s = s + prod;
            if (SKIPNA) ws = ws + wt;
        }
        n++;
    }
}

template <typename VT, bool BOX, bool SKIPNA>
__global__ __launch_bounds__(CTK_FILTER_THREADS) void k_filter_ring(const VT *__restrict__ x, int64_t xbase, const CtkFilterTap *__restrict__ tab_ptr,
                                                                    const double *__restrict__ w_ptr, int K, int edges_nan, int64_t npix, int64_t o0, int64_t o1,
                                                                    int64_t tile, VT *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char fl_ring_lds[];
    const int nth = (int)blockDim.x;
    VT *ring = (VT *)fl_ring_lds + threadIdx.x;
    ctk_const_f64 *w = (ctk_const_f64 *)w_ptr;
    ctk_const_tap *tab = (ctk_const_tap *)tab_ptr;
    const int64_t p = (int64_t)blockIdx.x * nth + threadIdx.x;
    if (p >= npix) return;                                                       // (no barrier below: a lane's ring is its own)
    const int64_t q0 = o0 + (int64_t)blockIdx.y * tile, q1 = min(o1, q0 + tile);
    if (q0 >= q1) return;
    // slot 0 holds the first used step of the tile, step j lies in slot (j - jlo) % K: an output's used taps are its last k1 - k0 steps
    const int64_t jlo = tab[q0].first + tab[q0].k0, jhi = tab[q1 - 1].first + tab[q1 - 1].k1;
    int64_t q = q0;
    int k0 = tab[q].k0, k1 = tab[q].k1;
    int64_t last = tab[q].first + k1 - 1;                                        // the step of output q's last used tap
    int slot = 0;
    for (int64_t j = jlo; j < jhi; j++) {
        ring[slot * nth] = x[(j - xbase) * npix + p];
        while (last == j) {
            int sl = slot - (k1 - 1 - k0);                                       // the slot of tap k0 (k1 - k0 <= K: one turn back at most)
            if (sl < 0) sl += K;
            double s = 0.0, ws = 0.0;
            int n = 0;
            const int run = min(k1 - k0, K - sl);                                // the taps up to the end of the ring, then those from slot 0 on
            filter_taps_add<VT, BOX, SKIPNA>(ring + sl * nth, nth, w + k0, run, s, ws, n);
            filter_taps_add<VT, BOX, SKIPNA>(ring, nth, w + k0 + run, k1 - k0 - run, s, ws, n);
            out[(q - o0) * npix + p] = filter_result<VT, BOX, SKIPNA>(s, ws, n, k0, k1, K, edges_nan, w);
            if (++q < q1) { k0 = tab[q].k0; k1 = tab[q].k1; last = tab[q].first + k1 - 1; }
            else last = -1;                                                      // (no step is negative)
        }
        slot = slot + 1 == K ? 0 : slot + 1;
    }
}

template <typename VT, bool BOX, bool SKIPNA>
__global__ __launch_bounds__(CTK_FILTER_THREADS) void k_filter_plain(const VT *__restrict__ x, int64_t xbase, const CtkFilterTap *__restrict__ tab_ptr,
                                                                     const double *__restrict__ w_ptr, int K, int edges_nan, int64_t npix, int64_t o0, int64_t o1,
                                                                     int64_t tile, VT *__restrict__ out)
{
    ctk_const_f64 *w = (ctk_const_f64 *)w_ptr;
    ctk_const_tap *tab = (ctk_const_tap *)tab_ptr;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int64_t q0 = o0 + (int64_t)blockIdx.y * tile, q1 = min(o1, q0 + tile);
    for (int64_t q = q0; q < q1; q++) {
        const int k0 = tab[q].k0, k1 = tab[q].k1;
        const VT *xs = x + (tab[q].first - xbase) * npix + p;
        double s = 0.0, ws = 0.0;
        int n = 0;
        filter_taps_add<VT, BOX, SKIPNA>(xs + (int64_t)k0 * npix, npix, w + k0, k1 - k0, s, ws, n);
        out[(q - o0) * npix + p] = filter_result<VT, BOX, SKIPNA>(s, ws, n, k0, k1, K, edges_nan, w);
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the layout (include/contrack_hip.h): one tap record per output, the outputs of the segments in order; out_starts (may be null):
// the first output of every segment.  The arguments have been checked (filter_layout_check).
static void filter_taps(int64_t T, int64_t K, int64_t stride, int64_t offset, const int64_t *starts, int64_t nseg, std::vector<CtkFilterTap> &taps, int64_t *out_starts)
{
    taps.clear();
    const int64_t one = 0;
    if (nseg < 1) { starts = &one; nseg = 1; }
    const int64_t c = offset + K / 2;                                            // label - S of q = 0
    for (int64_t k = 0; k < nseg; k++) {
        const int64_t S = starts[k], E = k + 1 < nseg ? starts[k + 1] : T;
        if (out_starts) out_starts[k] = (int64_t)taps.size();
        for (int64_t q = c >= 0 ? 0 : (-c + stride - 1) / stride; c + q * stride < E - S; q++) {
            const int64_t first = S + offset + q * stride;
            CtkFilterTap t;
            t.first = first; t.k0 = (int32_t)std::max<int64_t>(0, S - first); t.k1 = (int32_t)std::min<int64_t>(K, E - first);
            taps.push_back(t);
        }
    }
}

static int filter_layout_check(const char *who, int64_t T, int64_t K, int64_t stride, int64_t offset, const int64_t *starts, int64_t nseg)
{
    if (T < 1) return ctk_set_error(CTK_E_INVALID, "%s: T = %lld steps", who, (long long)T);
    if (K < 1 || K > CTK_FILTER_MAX_TAPS) return ctk_set_error(CTK_E_INVALID, "%s: K = %lld taps (1 .. %d)", who, (long long)K, CTK_FILTER_MAX_TAPS);
    if (stride < 1 || stride > ((int64_t)1 << 40)) return ctk_set_error(CTK_E_INVALID, "%s: stride = %lld (at least 1)", who, (long long)stride);
    if (offset < -((int64_t)1 << 40) || offset > ((int64_t)1 << 40)) return ctk_set_error(CTK_E_INVALID, "%s: offset = %lld", who, (long long)offset);
    return segment_starts_check(who, starts, nseg, T);
}

extern "C" int ctk_filter_layout(int64_t T, int K, int64_t stride, int64_t offset, const int64_t *starts, int64_t nseg, int64_t *first_out, int64_t *out_starts,
                                 int64_t *T_out)
{
    if (!T_out) return ctk_set_error(CTK_E_INVALID, "ctk_filter_layout: null T_out");
    CTKCHK(filter_layout_check("ctk_filter_layout", T, K, stride, offset, starts, nseg));
    std::vector<CtkFilterTap> taps;
    filter_taps(T, K, stride, offset, starts, nseg, taps, out_starts);
    if (first_out) for (size_t i = 0; i < taps.size(); i++) first_out[i] = taps[i].first;
    *T_out = (int64_t)taps.size();
    return CTK_OK;
}

// the arguments every entry shares, the handle last so that a mistake is named with a null handle too
struct FilterArgs {
    int64_t T; int ny, nx; const double *w; int K; int64_t stride, offset; int edges, skipna; const int64_t *starts; int64_t nseg;
};
static int filter_check(const char *who, const ctk_handle *h, const FilterArgs &a)
{
    if (a.ny < 1 || a.nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: a plane of %d x %d", who, a.ny, a.nx);
    CTKCHK(filter_layout_check(who, a.T, a.K, a.stride, a.offset, a.starts, a.nseg));
    if (a.edges != CTK_FILTER_EDGES_NAN && a.edges != CTK_FILTER_EDGES_RENORM) return ctk_set_error(CTK_E_INVALID, "%s: edges = %d", who, a.edges);
    if (a.w) {
        double sum = 0.0;
        bool neg = false;
        for (int i = 0; i < a.K; i++) {
            if (!std::isfinite(a.w[i])) return ctk_set_error(CTK_E_INVALID, "%s: w[%d] = %g (every weight must be finite)", who, i, a.w[i]);
            neg = neg || a.w[i] < 0.0;
            sum = sum + a.w[i];
        }
        if ((a.edges == CTK_FILTER_EDGES_RENORM || a.skipna) && (neg || !(sum > 0.0)))
            return ctk_set_error(CTK_E_INVALID, "%s: edges = renorm and skipna divide by the sum of the used weights: every weight must be >= 0 and their sum > 0", who);
    }
    if (!h) return ctk_set_error(CTK_E_INVALID, "%s: null handle", who);
    return CTK_OK;
}

// weights and taps of a call on the device
struct FilterTable {
    std::vector<CtkFilterTap> taps;
    const double *w_dev = nullptr;
    const CtkFilterTap *tab_dev = nullptr;
};
static int filter_table(ctk_handle *h, const FilterArgs &a, FilterTable &ft)
{
    filter_taps(a.T, a.K, a.stride, a.offset, a.starts, a.nseg, ft.taps, nullptr);
    const size_t wb = (((size_t)(a.w ? a.K : 1) * 8) + 15) & ~(size_t)15, tb = ft.taps.size() * sizeof(CtkFilterTap);
    CTKCHK(ensure(h, h->fl_tab, wb + tb));
    if (a.w) HIPCHK(hipMemcpy(h->fl_tab.p, a.w, (size_t)a.K * 8, hipMemcpyHostToDevice));
    if (tb) HIPCHK(hipMemcpy((char *)h->fl_tab.p + wb, ft.taps.data(), tb, hipMemcpyHostToDevice));
    ft.w_dev = (const double *)h->fl_tab.p;
    ft.tab_dev = (const CtkFilterTap *)((const char *)h->fl_tab.p + wb);
    return CTK_OK;
}

// outputs [o0, o1) on the handle's stream: plane 0 of x is step xbase and the steps [xlo, xhi) of it may be read; plane 0 of out is output o0
template <typename VT>
static int launch_filter(ctk_handle *h, const FilterArgs &a, const FilterTable &ft, const VT *x, int64_t xbase, int64_t xlo, int64_t xhi, int64_t o0, int64_t o1, VT *out)
{
    if (o1 <= o0) return CTK_OK;
    const CtkFilterTap &f = ft.taps[(size_t)o0], &l = ft.taps[(size_t)o1 - 1];
    if (f.first + f.k0 < xlo || l.first + l.k1 > xhi)                            // (used steps do not fall over the outputs: these two bound them all)
        return ctk_set_error(CTK_E_RANGE, "ctk_filter: outputs [%lld, %lld) use steps [%lld, %lld), the window holds [%lld, %lld)", (long long)o0, (long long)o1,
                             (long long)(f.first + f.k0), (long long)(l.first + l.k1), (long long)xlo, (long long)xhi);
    const int64_t npix = (int64_t)a.ny * a.nx;
    const CtkTimeFilterPlan pl = ctk_filter_plan((int)sizeof(VT), a.K, a.stride, o1 - o0, npix, h->fl_waves_dbg,
                                             h->fl_gy_dbg > 0 ? std::min<int64_t>(h->fl_gy_dbg, 65535) : 65535, h->fl_form_dbg);
    const int64_t last[8] = {pl.form, pl.threads, pl.tile, pl.gx, pl.gy, (int64_t)pl.lds, o0, o1};
    memcpy(h->fl_last, last, sizeof last);
    h->fl_launches++;
    const dim3 grid(pl.gx, pl.gy);
    const int en = a.edges == CTK_FILTER_EDGES_NAN;
#define CTK_FILTER_LAUNCH(B, S)                                                                                                                              \
    do {                                                                                                                                                     \
        if (pl.form == CTK_FILTER_RING)                                                                                                                      \
            k_filter_ring<VT, B, S><<<grid, pl.threads, pl.lds, h->stream>>>(x, xbase, ft.tab_dev, ft.w_dev, a.K, en, npix, o0, o1, pl.tile, out);          \
        else                                                                                                                                                 \
            k_filter_plain<VT, B, S><<<grid, pl.threads, 0, h->stream>>>(x, xbase, ft.tab_dev, ft.w_dev, a.K, en, npix, o0, o1, pl.tile, out);             \
    } while (0)
    if (!a.w) { if (a.skipna) CTK_FILTER_LAUNCH(true, true); else CTK_FILTER_LAUNCH(true, false); }
    else      { if (a.skipna) CTK_FILTER_LAUNCH(false, true); else CTK_FILTER_LAUNCH(false, false); }
#undef CTK_FILTER_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

template <typename VT>
static int filter_dev_impl(ctk_handle *h, const VT *x_dev, const FilterArgs &a, VT *out_dev, int64_t T_out, const char *who)
{
    CTKCHK(filter_check(who, h, a));
    if (!x_dev || !out_dev) return ctk_set_error(CTK_E_INVALID, "%s: null slab", who);
    HIPCHK(hipSetDevice(h->device));
    h->fl_launches = 0;
    FilterTable ft;
    CTKCHK(filter_table(h, a, ft));
    if ((int64_t)ft.taps.size() != T_out)
        return ctk_set_error(CTK_E_INVALID, "%s: T_out = %lld, the layout has %lld outputs (ctk_filter_layout)", who, (long long)T_out, (long long)ft.taps.size());
    CTKCHK(launch_filter<VT>(h, a, ft, x_dev, 0, 0, a.T, 0, T_out, out_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_filter_f32_dev(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges,
                                  int skipna, const int64_t *starts, int64_t nseg, float *out_dev, int64_t T_out)
{
    return filter_dev_impl<float>(h, x_dev, FilterArgs{T, ny, nx, w, K, stride, offset, edges, skipna, starts, nseg}, out_dev, T_out, "ctk_filter_f32_dev");
}
extern "C" int ctk_filter_f64_dev(ctk_handle *h, const double *x_dev, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges,
                                  int skipna, const int64_t *starts, int64_t nseg, double *out_dev, int64_t T_out)
{
    return filter_dev_impl<double>(h, x_dev, FilterArgs{T, ny, nx, w, K, stride, offset, edges, skipna, starts, nseg}, out_dev, T_out, "ctk_filter_f64_dev");
}

template <typename VT>
static int filter_stream_impl(ctk_handle *h, StreamIO &io, const FilterArgs &a, int64_t T_out, int64_t chunk_steps, int keep_resident, const char *name)
{
    CTKCHK(filter_check(name, h, a));
    const bool sink = io.host_out_v || io.write_v;
    if (!io.host_in && !io.read) return ctk_set_error(CTK_E_INVALID, "%s: null input", name);
    if (!sink && !keep_resident) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output and keep_resident = 0)", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", name, (long long)chunk_steps);
    HIPCHK(hipSetDevice(h->device));
    h->fl_launches = 0;
    const int64_t npix = (int64_t)a.ny * a.nx, K = a.K, halo = K - 1;
    const size_t plane = (size_t)npix * sizeof(VT);
    io.esz = sizeof(VT);
    io.chunk = ctk_stream_chunk(chunk_steps, a.T, plane, std::max<int64_t>(halo, 1));                     // (at least the halo: see below)
    const double t_call = now_ms();
    FilterTable ft;
    CTKCHK(filter_table(h, a, ft));
    const int64_t n_out = (int64_t)ft.taps.size();
    if (n_out != T_out)
        return ctk_set_error(CTK_E_INVALID, "%s: T_out = %lld, the layout has %lld outputs (ctk_filter_layout)", name, (long long)T_out, (long long)n_out);
    // an output leaves with the chunk that holds step first + K - 1; `first` rises by `stride` inside a segment, so a chunk gives
    // chunk / stride + 2 outputs or fewer -- and one more per segment that begins inside it, which is counted here rather than bounded
    auto done_at = [&](int64_t end, int64_t from) {                               // outputs complete once the steps below `end` are there
        if (end >= a.T) return n_out;
        int64_t o = from;
        while (o < n_out && ft.taps[(size_t)o].first + K - 1 < end) o++;
        return o;
    };
    int64_t most = 1;
    for (int64_t c0 = 0, o = 0; c0 < a.T; c0 += io.chunk) { const int64_t o1 = done_at(c0 + io.chunk, o); most = std::max(most, o1 - o); o = o1; }
    CTKCHK(stream_setup(h, (size_t)(io.chunk + halo) * plane, 0, io.read != nullptr));
    if (keep_resident) {
        CTKCHK(ensure(h, h->fl_out, (size_t)std::max<int64_t>(n_out, 1) * plane));
        if (io.write_v) CTKCHK(stream_setup(h, 0, (size_t)most * plane, true));
    } else {
        CTKCHK(stream_setup(h, 0, (size_t)most * plane, io.write_v != nullptr));
    }
    // (window_produce: an output that has not left yet has first + K - 1 >= c0, so its first tap is in the window of K - 1 kept steps)
    const int rc = window_produce(
        h, io, a.T, halo, plane, name, done_at,
        [&](int b, int64_t o0) { return keep_resident ? (char *)h->fl_out.p + (size_t)o0 * plane : (char *)h->io_out.p + (size_t)b * (size_t)most * plane; },
        [&](const char *win, int64_t xbase, int64_t xlo, int64_t xhi, int64_t o0, int64_t o1, char *out) {
            return launch_filter<VT>(h, a, ft, (const VT *)win, xbase, xlo, xhi, o0, o1, (VT *)out);
        });
    CTKCHK(stream_produce_end(h, io, rc, t_call));
    if (keep_resident) h->lv_slab.adopt(h->fl_out, n_out, a.ny, a.nx, sizeof(VT) == 8);     // (the result becomes the resident level mean)
    return CTK_OK;
}

extern "C" int ctk_filter_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna,
                              const int64_t *starts, int64_t nseg, float *out, int64_t T_out, int64_t chunk_steps, int keep_resident)
{
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return filter_stream_impl<float>(h, io, FilterArgs{T, ny, nx, w, K, stride, offset, edges, skipna, starts, nseg}, T_out, chunk_steps, keep_resident, "ctk_filter_f32");
}
extern "C" int ctk_filter_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna,
                              const int64_t *starts, int64_t nseg, double *out, int64_t T_out, int64_t chunk_steps, int keep_resident)
{
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return filter_stream_impl<double>(h, io, FilterArgs{T, ny, nx, w, K, stride, offset, edges, skipna, starts, nseg}, T_out, chunk_steps, keep_resident, "ctk_filter_f64");
}
extern "C" int ctk_filter_stream_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const double *w, int K,
                                    int64_t stride, int64_t offset, int edges, int skipna, const int64_t *starts, int64_t nseg, ctk_write_values_fn writer,
                                    void *writer_user, int64_t T_out, int64_t chunk_steps, int keep_resident)
{
    const FilterArgs a{T, ny, nx, w, K, stride, offset, edges, skipna, starts, nseg};
    CTKCHK(filter_check("ctk_filter_stream_cb", h, a));
    StreamIO io;
    CTKCHK(stream_cb_io("ctk_filter_stream_cb", h, elem_bytes, reader, reader_user, writer, writer_user, io));
    if (elem_bytes == 8) return filter_stream_impl<double>(h, io, a, T_out, chunk_steps, keep_resident, "ctk_filter_stream_cb");
    return filter_stream_impl<float>(h, io, a, T_out, chunk_steps, keep_resident, "ctk_filter_stream_cb");
}

// the input is the resident level mean: nothing is uploaded.  The result goes to fl_out, from there to `out` and / or into the slot.
template <typename VT>
static int filter_resident_impl(ctk_handle *h, const FilterArgs &a, VT *out, int64_t T_out, int keep_resident)
{
    const char *who = "ctk_filter_resident";
    HIPCHK(hipSetDevice(h->device));
    h->fl_launches = 0;
    const size_t plane = (size_t)a.ny * a.nx * sizeof(VT);
    FilterTable ft;
    CTKCHK(filter_table(h, a, ft));
    const int64_t n_out = (int64_t)ft.taps.size();
    if (n_out != T_out) return ctk_set_error(CTK_E_INVALID, "%s: T_out = %lld, the layout has %lld outputs (ctk_filter_layout)", who, (long long)T_out, (long long)n_out);
    CTKCHK(ensure(h, h->fl_out, (size_t)std::max<int64_t>(n_out, 1) * plane));
    CTKCHK(launch_filter<VT>(h, a, ft, (const VT *)h->lv_slab.buf.p, 0, 0, a.T, 0, n_out, (VT *)h->fl_out.p));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (out && n_out) CTKCHK(download(h, h->fl_out.p, out, (size_t)n_out * plane));
    if (keep_resident) h->lv_slab.adopt(h->fl_out, n_out, a.ny, a.nx, sizeof(VT) == 8);
    return CTK_OK;
}

extern "C" int ctk_filter_resident(ctk_handle *h, const double *w, int K, int64_t stride, int64_t offset, int edges, int skipna, const int64_t *starts, int64_t nseg,
                                   void *out, int64_t T_out, int keep_resident)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "ctk_filter_resident: null handle");
    const ResidentSlab &m = h->lv_slab;
    if (!m.held()) return ctk_set_error(CTK_E_INVALID, "ctk_filter_resident: no vertical mean is resident (ctk_level_mean_* or ctk_filter_* with keep_resident)");
    if (!out && !keep_resident) return ctk_set_error(CTK_E_INVALID, "ctk_filter_resident: nothing to produce (no output and keep_resident = 0)");
    const FilterArgs a{m.T, m.ny, m.nx, w, K, stride, offset, edges, skipna, starts, nseg};
    CTKCHK(filter_check("ctk_filter_resident", h, a));
    if (m.f64) return filter_resident_impl<double>(h, a, (double *)out, T_out, keep_resident);
    return filter_resident_impl<float>(h, a, (float *)out, T_out, keep_resident);
}

// ---- test hooks ------------------------------------------------------------------------------------------------------------------
// what ctk_filter_plan decides (host only: no handle, no GPU); waves_wanted / grid_y_max: 0 the rule's, forced: -1 the rule's form;
// out6 = {form, threads, lds, tile, gx, gy}
extern "C" int ctk_debug_filter_plan(int elem_bytes, int K, int64_t stride, int64_t nout, int64_t npix, int64_t waves_wanted, int64_t grid_y_max, int forced, int64_t *out6)
{
    if (!out6 || (elem_bytes != 4 && elem_bytes != 8) || K < 1 || stride < 1 || nout < 1 || npix < 1 || waves_wanted < 0 || grid_y_max < 0 || forced < -1 || forced > 1)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_filter_plan: bad arguments");
    const CtkTimeFilterPlan p = ctk_filter_plan(elem_bytes, K, stride, nout, npix, waves_wanted,
                                            grid_y_max > 0 ? std::min<int64_t>(grid_y_max, 65535) : 65535, forced);
    out6[0] = p.form; out6[1] = p.threads; out6[2] = (int64_t)p.lds; out6[3] = p.tile; out6[4] = p.gx; out6[5] = p.gy;
    return CTK_OK;
}

// for the following filter launches on this handle: ctk_filter_plan's waves_wanted, grid_y_max (0: the rule's) and forced form (-1: the rule's)
extern "C" int ctk_debug_set_filter(ctk_handle *h, int64_t waves_wanted, int64_t grid_y_max, int forced)
{
    if (!h || waves_wanted < 0 || grid_y_max < 0 || forced < -1 || forced > 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_filter: bad argument");
    h->fl_waves_dbg = waves_wanted; h->fl_gy_dbg = grid_y_max; h->fl_form_dbg = forced;
    return CTK_OK;
}

// out9 = {form, threads, tile, gx, gy, lds, o0, o1} of the last filter launch on this handle (form -1: none yet), then the number of
// launches the last ctk_filter_* call made
extern "C" int ctk_debug_filter_launch(ctk_handle *h, int64_t *out9)
{
    if (!h || !out9) return ctk_set_error(CTK_E_INVALID, "null argument");
    for (int i = 0; i < 8; i++) out9[i] = h->fl_last[i];
    out9[8] = h->fl_launches;
    return CTK_OK;
}

// measurement (tools/filter_probe.py): the filter kernel alone between HIP events on slabs in device memory, or (copy_bytes > 0)
// k_copy16 over that many bytes of the same two buffers; ms2 = {best, mean}
extern "C" int ctk_debug_time_filter(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const double *w, int K, int64_t stride, int64_t offset,
                                     int edges, int skipna, void *out_dev, int64_t T_out, int64_t copy_bytes, int reps, double *ms2)
{
    const FilterArgs a{T, ny, nx, w, K, stride, offset, edges, skipna, nullptr, 0};
    CTKCHK(filter_check("ctk_debug_time_filter", h, a));
    if (!x_dev || !out_dev || !ms2 || reps < 1 || copy_bytes < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_filter: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    if (copy_bytes > 0) return time_copy16(h, "ctk_debug_time_filter", LaunchKnobs(), x_dev, out_dev, copy_bytes, reps, ms2);
    FilterTable ft;
    CTKCHK(filter_table(h, a, ft));
    if ((int64_t)ft.taps.size() != T_out) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_filter: T_out = %lld, the layout has %lld outputs", (long long)T_out, (long long)ft.taps.size());
    return time_launches(h, "ctk_debug_time_filter", reps, ms2, [&]() {
        return is_f64 ? launch_filter<double>(h, a, ft, (const double *)x_dev, 0, 0, T, 0, T_out, (double *)out_dev)
                      : launch_filter<float>(h, a, ft, (const float *)x_dev, 0, 0, T, 0, T_out, (float *)out_dev);
    });
}
