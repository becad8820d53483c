// ctk_subset.hip -- the step between run_lifecycle and the consumers of `flag` on the device (included by ctk_api.hip): keep the
// tracks, or the (step, track) rows, a study picked from the life-cycle frame and clear the rest of the int32 flag slab
// (steps, ny, nx).  include/contrack_hip.h states it, tests/subset_util.py is its numpy statement.  A TABLE is `off` and `ids`:
// ids[off[t] .. off[t + 1]) are the ids wanted at step t, positive and strictly increasing; a by-id table has the one slice [0, K) for
// every step.  Per pixel, f its flag:
//     found = f > 0 and f in the step's slice ;  sel = invert ? (f > 0 and not found) : found
//     out = sel ? (mask ? 1 : f) : 0 ;  hits[entry that found it] += 1 ;  n_selected += sel
//
// k_subset: one lane per 16 bytes of adjacent pixels of one step, or per pixel where a plane does not start on a 16-byte boundary (a
// plane that is no multiple of 4 pixels, an offset pointer).  One read and at most one write of the slab; a lane writes only what it
// read, so the output may be the input.  A workgroup takes a part of a step -- CTK_SUBSET_TILES tiles of 256 lanes, loaded together
// -- per load of its table (ctk_subset_plan, ctk_forms.h, picks the form): the by-id forms load bitmap or ids once and stride over
// the parts, the row forms load the step's slice with every part.  The flags of a workgroup's next part are fetched before the
// current one is looked up, and a slice is fetched while its part's flags travel.  Background comes first: flags are 7-10 % of a tracked slab, and
// a lane whose values are all <= 0 looks nothing up.  Hits are counted in LDS beside the ids (uint32; flushed with one 64-bit atomic per
// non-zero counter when the slice goes, and before a counter could wrap) or, in the global-memory forms, with one atomic per found
// pixel.  n_selected: a 64-bit count per lane, one atomic per wave at the end into one of CTK_SUBSET_NSEL words the host sums.
#pragma once

#define CTK_SUBSET_NSEL 256             // words n_selected is counted in: a wave adds to the one of its number, the host sums them

typedef const __attribute__((address_space(4))) int64_t ctk_const_i64;      // a wave-uniform index into it is an s_load

struct SubsetDev {
    const int64_t *off;                // by id: unused; by row: off[s], off[s + 1] of step s of THIS launch
    const int32_t *ids;
    const uint32_t *bitmap;            // CTK_SUBSET_BITMAP: (max_id >> 5) + 1 words
    unsigned long long *hits;          // one per entry of ids, or null
    unsigned long long *nsel;          // CTK_SUBSET_NSEL counters whose sum is n_selected, or null
    int32_t max_id;
    uint32_t K;                        // by id: the ids
    int invert, mask;
};

// the entry of the sorted ids[0, n) that equals f, or n
template <typename P>
__device__ __forceinline__ uint32_t subset_find(P ids, uint32_t n, int32_t f)
{
    uint32_t lo = 0, len = n;
    while (len > 0) {
        const uint32_t half = len >> 1;
        if (ids[lo + half] < f) { lo += half + 1; len -= half + 1; }
        else len = half;
    }
    return lo < n && ids[lo] == f ? lo : n;
}

// flag, out: (steps, npix).  Part b of `blocks` = bps * steps covers lanes [part * TILES * 256, ...) of step b / bps; lane q of a plane
// owns pixels [q * N, q * N + N).
template <int FORM, bool VEC, bool HITS, bool WRITE>
__global__ __launch_bounds__(CTK_SUBSET_THREADS) void k_subset(const int32_t *flag, int64_t npix, int64_t bps, int64_t blocks, SubsetDev a, int32_t *out, int xcd)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    constexpr bool ROW = FORM == CTK_SUBSET_ROW_LDS || FORM == CTK_SUBSET_ROW_GLB;
    constexpr bool SEARCH_LDS = FORM == CTK_SUBSET_SEARCH_LDS || FORM == CTK_SUBSET_ROW_LDS;
    constexpr bool COUNT_LDS = SEARCH_LDS && HITS;
    constexpr int N = VEC ? 4 : 1, TILES = CTK_SUBSET_TILES;
    const uint32_t tid = threadIdx.x;
    const int64_t lanes = VEC ? npix / 4 : npix;                                  // lanes of one plane
    const int32_t *ids_s = (const int32_t *)sm;
    const int32_t *ids_g = a.ids;                                                 // the slice in use: [base, base + n) of the table
    int64_t base = 0;
    uint32_t n = ROW ? 0 : a.K;
    unsigned long long nsel = 0;
    uint32_t since = 0;                                                           // parts counted into the LDS counters since their last flush

    auto load_ids = [&]() {                                                       // ids_g[0, n) into LDS, the counters behind them zero
        for (uint32_t i = tid; i < n; i += CTK_SUBSET_THREADS) {
            sm[i] = (uint32_t)ids_g[i];
            if (COUNT_LDS) sm[n + i] = 0;
        }
    };
    auto flush = [&]() {                                                          // (between two barriers of the caller)
        for (uint32_t i = tid; i < n; i += CTK_SUBSET_THREADS) {
            const uint32_t c = sm[n + i];
            if (c) { atomicAdd(a.hits + base + i, (unsigned long long)c); sm[n + i] = 0; }
        }
    };
    auto look = [&](int32_t f) -> int32_t {
        if (f <= 0) return 0;
        bool found;
        if (FORM == CTK_SUBSET_BITMAP) found = f <= a.max_id && ((sm[(uint32_t)f >> 5] >> (f & 31)) & 1u);
        else {
            const uint32_t e = SEARCH_LDS ? subset_find(ids_s, n, f) : subset_find(ids_g, n, f);
            found = e < n;
            if (HITS && found) {
                if (SEARCH_LDS) atomicAdd(&sm[n + e], 1u);
                else atomicAdd(a.hits + base + e, 1ull);
            }
        }
        const bool sel = found != (a.invert != 0);
        nsel += sel;
        return sel ? (a.mask ? 1 : f) : 0;
    };

    if (!ROW) {
        if (FORM == CTK_SUBSET_BITMAP)
            for (uint32_t i = tid, w = ((uint32_t)a.max_id >> 5) + 1; i < w; i += CTK_SUBSET_THREADS) sm[i] = a.bitmap[i];
        if (FORM == CTK_SUBSET_SEARCH_LDS) load_ids();
        __syncthreads();
    }
    // the tiles of part b: all their loads are issued before the first is used (lanes past the plane: zeros)
    auto fetch = [&](int64_t b, i32x4 (&v)[TILES]) {
        const int64_t s = b / bps;
        const int64_t q0 = (b - s * bps) * (TILES * CTK_SUBSET_THREADS) + tid;
        const int32_t *fs = flag + s * npix;                                      // (64-bit throughout)
#pragma unroll
        for (int k = 0; k < TILES; k++) {
            const int64_t q = q0 + k * CTK_SUBSET_THREADS;
            v[k] = i32x4{0, 0, 0, 0};
            if (q < lanes) {
                if (VEC) v[k] = __builtin_nontemporal_load((const i32x4 *)(fs + q * 4));
                else v[k].x = fs[q];
            }
        }
    };
    i32x4 v[TILES], vn[TILES];
    int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd);                            // (a permutation of the launch's workgroups)
    if (b < blocks) fetch(b, v);
    bool first = true;
    for (; b < blocks; b += gridDim.x) {
        const int64_t s = b / bps;
        const int64_t q0 = (b - s * bps) * (TILES * CTK_SUBSET_THREADS) + tid;    // this thread's lane of the first tile
        // the next part's flags travel while this part's slice is loaded and its lanes are looked up (parts are disjoint: in place
        // nothing fetched here is written by this part)
        const bool more = b + gridDim.x < blocks;
        if (more) fetch(b + gridDim.x, vn);
        if (ROW) {
            ctk_const_i64 *off = (ctk_const_i64 *)a.off;                           // (the step is the workgroup's: scalar loads)
            base = off[s];
            n = (uint32_t)(off[s + 1] - base);
            ids_g = a.ids + base;
            if (FORM == CTK_SUBSET_ROW_LDS) {
                // (the part before this one has left the slice; a workgroup's first part has none before it, and its slice is
                // fetched while its flags travel)
                if (!first) __syncthreads();
                load_ids();
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < TILES; k++) {
            const int64_t q = q0 + k * CTK_SUBSET_THREADS;
            if (q >= lanes) continue;
            i32x4 r = {0, 0, 0, 0};
            if (v[k].x > 0 || (N == 4 && (v[k].y > 0 || v[k].z > 0 || v[k].w > 0))) {            // background first: most lanes stop here
                r.x = look(v[k].x);
                if (N == 4) { r.y = look(v[k].y); r.z = look(v[k].z); r.w = look(v[k].w); }
            }
            if (WRITE) {
                int32_t *os = out + s * npix;
                if (VEC) *(i32x4 *)(os + q * 4) = r;
                else os[q] = r.x;
            }
        }
        if (COUNT_LDS && (ROW || ++since == (1u << 19))) {                         // (2^19 parts of 2^12 pixels: a counter stays below 2^32)
            __syncthreads();
            flush();
            since = 0;
            if (!ROW) __syncthreads();
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < TILES; k++) v[k] = vn[k];
        }
        first = false;
    }
    if (COUNT_LDS && !ROW) {
        __syncthreads();
        flush();
    }
    if (a.nsel) {
        for (int o = 32; o > 0; o >>= 1) nsel += __shfl_down(nsel, o);
        // (a row launch has a workgroup per part: a quarter of a million waves adding to ONE word took longer than the slab)
        if ((tid & 63) == 0 && nsel) atomicAdd(a.nsel + ((blockIdx.x * (CTK_SUBSET_THREADS / 64) + (tid >> 6)) & (CTK_SUBSET_NSEL - 1)), nsel);
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the table of a call as the caller gave it (host pointers)
struct SubsetArgs {
    const int64_t *off; int64_t n_off;
    const int32_t *ids; int64_t n_ids;
    int invert, kind;
};
// ... and what the check found of it
struct SubsetShape { bool by_row; int64_t max_id, longest; };

static int subset_check(const char *who, const void *h, int64_t T, int ny, int nx, const SubsetArgs &a, SubsetShape &sh)
{
    if (!h || !a.off || (!a.ids && a.n_ids > 0)) return ctk_set_error(CTK_E_INVALID, "%s: null handle or table", who);
    if (T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad shape (T=%lld ny=%d nx=%d)", who, (long long)T, ny, nx);
    if ((int64_t)ny * nx > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: a plane of %lld pixels (at most 2^31 - 1)", who, (long long)ny * nx);
    if (a.kind != CTK_SUBSET_ID && a.kind != CTK_SUBSET_MASK) return ctk_set_error(CTK_E_INVALID, "%s: kind = %d (CTK_SUBSET_ID or CTK_SUBSET_MASK)", who, a.kind);
    if (a.n_off != 2 && a.n_off != T + 1) return ctk_set_error(CTK_E_INVALID, "%s: n_off = %lld (2: by id, or T + 1 = %lld: by row)", who, (long long)a.n_off, (long long)(T + 1));
    if (a.n_ids < 0 || a.off[0] != 0 || a.off[a.n_off - 1] != a.n_ids)
        return ctk_set_error(CTK_E_INVALID, "%s: off must run from 0 to n_ids = %lld (off[0] = %lld, off[%lld] = %lld)", who, (long long)a.n_ids, (long long)a.off[0],
                             (long long)(a.n_off - 1), (long long)a.off[a.n_off - 1]);
    sh.by_row = a.n_off != 2;
    sh.max_id = 0; sh.longest = 0;
    for (int64_t t = 0; t + 1 < a.n_off; t++) {
        const int64_t i0 = a.off[t], i1 = a.off[t + 1];
        if (i1 < i0 || i1 > a.n_ids) return ctk_set_error(CTK_E_INVALID, "%s: off[%lld] = %lld, off[%lld] = %lld: not non-decreasing within n_ids", who, (long long)t, (long long)i0, (long long)(t + 1), (long long)i1);
        for (int64_t i = i0; i < i1; i++) {
            if (a.ids[i] <= 0) return ctk_set_error(CTK_E_INVALID, "%s: ids[%lld] = %d (ids are > 0)", who, (long long)i, a.ids[i]);
            if (i > i0 && a.ids[i] <= a.ids[i - 1]) return ctk_set_error(CTK_E_INVALID, "%s: ids[%lld] = %d after %d: a slice must be strictly increasing", who, (long long)i, a.ids[i], a.ids[i - 1]);
        }
        sh.longest = std::max(sh.longest, i1 - i0);
        if (i1 > i0) sh.max_id = std::max<int64_t>(sh.max_id, a.ids[i1 - 1]);
    }
    return CTK_OK;
}

// a call's table on the device and its counters zeroed; want_hits: the call counts per entry
struct SubsetCall {
    SubsetShape sh;
    bool want_hits;
    int64_t n_ids;
    const int64_t *off_dev;
    SubsetDev d;
};
static int subset_table(ctk_handle *h, const SubsetArgs &a, const SubsetShape &sh, bool want_hits, bool want_nsel, SubsetCall &c)
{
    c.sh = sh; c.want_hits = want_hits; c.n_ids = a.n_ids;
    const bool bitmap = ctk_subset_plan(sh.by_row, sh.max_id, sh.longest, want_hits, 1, 1, false).form == CTK_SUBSET_BITMAP;
    const size_t words = bitmap ? (size_t)(sh.max_id >> 5) + 1 : 0;
    const size_t b_off = (size_t)a.n_off * 8, b_ids = (size_t)a.n_ids * 4;
    std::vector<char> host(b_off + b_ids + words * 4);
    memcpy(host.data(), a.off, b_off);
    if (b_ids) memcpy(host.data() + b_off, a.ids, b_ids);
    uint32_t *bm = (uint32_t *)(host.data() + b_off + b_ids);
    for (size_t w = 0; w < words; w++) bm[w] = 0;
    if (bitmap)
        for (int64_t i = 0; i < a.n_ids; i++) bm[(uint32_t)a.ids[i] >> 5] |= 1u << (a.ids[i] & 31);
    CTKCHK(ensure(h, h->sb_tab, host.size()));
    CTKCHK(ensure(h, h->sb_hits, (size_t)(a.n_ids + CTK_SUBSET_NSEL) * 8));
    HIPCHK(hipStreamSynchronize(h->stream));                                  // (a launch still reading the table of the call before)
    HIPCHK(hipMemcpy(h->sb_tab.p, host.data(), host.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(h->sb_hits.p, 0, (size_t)(a.n_ids + CTK_SUBSET_NSEL) * 8, h->stream));
    c.off_dev = (const int64_t *)h->sb_tab.p;
    c.d.off = c.off_dev;
    c.d.ids = (const int32_t *)((char *)h->sb_tab.p + b_off);
    c.d.bitmap = (const uint32_t *)((char *)h->sb_tab.p + b_off + b_ids);
    c.d.nsel = want_nsel ? P<unsigned long long>(h->sb_hits) : nullptr;
    c.d.hits = want_hits ? P<unsigned long long>(h->sb_hits) + CTK_SUBSET_NSEL : nullptr;
    c.d.max_id = (int32_t)sh.max_id;
    c.d.K = sh.by_row ? 0 : (uint32_t)a.n_ids;
    c.d.invert = a.invert != 0; c.d.mask = a.kind == CTK_SUBSET_MASK;
    return CTK_OK;
}

// the counters of a finished call to the host (hits, n_selected: null or where they go)
static int subset_counts(ctk_handle *h, const SubsetCall &c, uint64_t *hits, int64_t *n_selected)
{
    if (n_selected) {
        uint64_t part[CTK_SUBSET_NSEL];
        HIPCHK(hipMemcpy(part, h->sb_hits.p, sizeof part, hipMemcpyDeviceToHost));
        uint64_t sum = 0;
        for (uint64_t v : part) sum += v;
        *n_selected = (int64_t)sum;
    }
    if (hits && c.n_ids) HIPCHK(hipMemcpy(hits, (char *)h->sb_hits.p + CTK_SUBSET_NSEL * 8, (size_t)c.n_ids * 8, hipMemcpyDeviceToHost));
    return CTK_OK;
}

template <int FORM, bool VEC>
static void subset_launch_form(const CtkSubsetPlan &pl, hipStream_t st, bool hits, const int32_t *flag, int64_t npix, const SubsetDev &d, int32_t *out, int xcd)
{
#define CTK_SUBSET_LAUNCH(H, W) k_subset<FORM, VEC, H, W><<<pl.grid, CTK_SUBSET_THREADS, (size_t)pl.lds, st>>>(flag, npix, pl.bps, pl.blocks, d, out, xcd)
    if constexpr (FORM != CTK_SUBSET_BITMAP) {                                     // (the bitmap knows no entry: the rule never picks it with hits)
        if (hits) { if (out) CTK_SUBSET_LAUNCH(true, true); else CTK_SUBSET_LAUNCH(true, false); return; }
    }
    if (out) CTK_SUBSET_LAUNCH(false, true); else CTK_SUBSET_LAUNCH(false, false);
#undef CTK_SUBSET_LAUNCH
}

// out[s] = the selection of step s of flag (steps, ny * nx), the first of them step `step0` of the call's table, on the handle's
// stream; out null: counts only
static int launch_subset(ctk_handle *h, const int32_t *flag, int64_t npix, int64_t steps, const SubsetCall &c, int64_t step0, int32_t *out)
{
    const bool aligned = (((uintptr_t)flag | (uintptr_t)out) & 15) == 0;
    const CtkSubsetPlan pl = ctk_subset_plan(c.sh.by_row, c.sh.max_id, c.sh.longest, c.want_hits, npix, steps, aligned, h->sb_knobs.cap());
    h->sb_knobs.launched(pl.form, pl.grid); h->sb_vec = pl.vec;
    const int xcd = h->sb_knobs.xcd(pl.xcd);
    SubsetDev d = c.d;
    if (c.sh.by_row) d.off = c.off_dev + step0;
#define CTK_SUBSET_FORM(F) do { if (pl.vec) subset_launch_form<F, true>(pl, h->stream, c.want_hits, flag, npix, d, out, xcd); \
                                else subset_launch_form<F, false>(pl, h->stream, c.want_hits, flag, npix, d, out, xcd); } while (0)
    switch (pl.form) {
    case CTK_SUBSET_BITMAP: CTK_SUBSET_FORM(CTK_SUBSET_BITMAP); break;
    case CTK_SUBSET_SEARCH_LDS: CTK_SUBSET_FORM(CTK_SUBSET_SEARCH_LDS); break;
    case CTK_SUBSET_SEARCH_GLB: CTK_SUBSET_FORM(CTK_SUBSET_SEARCH_GLB); break;
    case CTK_SUBSET_ROW_LDS: CTK_SUBSET_FORM(CTK_SUBSET_ROW_LDS); break;
    default: CTK_SUBSET_FORM(CTK_SUBSET_ROW_GLB); break;
    }
#undef CTK_SUBSET_FORM
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

extern "C" int ctk_subset_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids,
                              int invert, int kind, int32_t *out_dev, uint64_t *hits, int64_t *n_selected)
{
    const char *who = "ctk_subset_dev";
    const SubsetArgs a = {off, n_off, ids, n_ids, invert, kind};
    SubsetShape sh;
    CTKCHK(subset_check(who, h, T, ny, nx, a, sh));
    if (!flag_dev) return ctk_set_error(CTK_E_INVALID, "%s: null flag", who);
    if (!out_dev && !hits && !n_selected) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output, no hits, no n_selected)", who);
    HIPCHK(hipSetDevice(h->device));
    SubsetCall c;
    CTKCHK(subset_table(h, a, sh, hits != nullptr, n_selected != nullptr, c));
    CTKCHK(launch_subset(h, flag_dev, (int64_t)ny * nx, T, c, 0, out_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return subset_counts(h, c, hits, n_selected);
}

// the int32 writer of a ctk_subset_cb call behind the writer of values stream_produce drains into
struct SubsetWriter { ctk_write_chunk_fn fn; void *user; };
static int subset_write(void *user, int64_t t0, int64_t nt, const void *src)
{
    const SubsetWriter *w = (const SubsetWriter *)user;
    return w->fn(w->user, t0, nt, (const int32_t *)src);
}

// host array or callbacks: the flag passes through two chunk-sized device buffers and the selection through two more
// (stream_produce); table and counters stay in HBM for the whole call
static int subset_stream_impl(ctk_handle *h, StreamIO &io, int64_t T, int ny, int nx, const SubsetArgs &a, uint64_t *hits, int64_t *n_selected, int64_t chunk_steps,
                              const char *name)
{
    SubsetShape sh;
    CTKCHK(subset_check(name, h, T, ny, nx, a, sh));
    if (!io.read && !io.host_in) return ctk_set_error(CTK_E_INVALID, "%s: null input", name);
    const bool sink = io.host_out_v || io.write_v;
    if (!sink && !hits && !n_selected) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output, no hits, no n_selected)", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", name, (long long)chunk_steps);
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    const size_t plane = (size_t)npix * 4;
    io.esz = 4;
    io.chunk = ctk_stream_chunk(chunk_steps, T, plane);
    const double t_call = now_ms();
    CTKCHK(stream_setup(h, (size_t)io.chunk * plane, 0, io.read != nullptr));
    if (sink) CTKCHK(stream_setup(h, 0, (size_t)io.chunk * plane, io.write_v != nullptr));
    SubsetCall c;
    CTKCHK(subset_table(h, a, sh, hits != nullptr, n_selected != nullptr, c));
    Producer p;
    p.in_bytes = (size_t)io.chunk * plane; p.out_step = plane;
    p.upload = [&](const ProduceIn &in) -> int { return upload_steps(h, io, in, plane); };
    p.launch = [&](const ProduceIn &in, ProduceOut &o) -> int {
        if (sink) { o.t0 = in.c0; o.nt = in.nt; o.dev = (char *)h->io_out.p + (size_t)in.b * (size_t)io.chunk * plane; }
        return launch_subset(h, (const int32_t *)in.dev, npix, in.nt, c, in.c0, (int32_t *)o.dev);
    };
    const int rc = stream_produce(h, io, T, name, p);
    CTKCHK(stream_produce_end(h, io, rc, t_call));
    return subset_counts(h, c, hits, n_selected);
}

extern "C" int ctk_subset(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids, int invert,
                          int kind, int32_t *out, uint64_t *hits, int64_t *n_selected, int64_t chunk_steps)
{
    const SubsetArgs a = {off, n_off, ids, n_ids, invert, kind};
    StreamIO io;
    io.host_in = flag; io.host_out_v = out;
    return subset_stream_impl(h, io, T, ny, nx, a, hits, n_selected, chunk_steps, "ctk_subset");
}

extern "C" int ctk_subset_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int64_t *off, int64_t n_off, const int32_t *ids,
                             int64_t n_ids, int invert, int kind, ctk_write_chunk_fn writer, void *writer_user, uint64_t *hits, int64_t *n_selected, int64_t chunk_steps)
{
    const SubsetArgs a = {off, n_off, ids, n_ids, invert, kind};
    SubsetWriter w = {writer, writer_user};
    StreamIO io;
    io.read = reader; io.read_user = reader_user;
    if (writer) { io.write_v = subset_write; io.write_user = &w; }
    return subset_stream_impl(h, io, T, ny, nx, a, hits, n_selected, chunk_steps, "ctk_subset_cb");
}

// what ctk_subset_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_subset_plan(int by_row, int64_t max_id, int64_t longest, int want_hits, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t grid_max,
                                     int64_t *out12)
{
    if (!out12 || max_id < 0 || max_id > 0x7fffffffll || longest < 0 || ny < 1 || nx < 1 || steps < 1 || ny * nx > 0x7fffffffll || grid_max < 0)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_subset_plan: bad arguments");
    const CtkSubsetPlan p = ctk_subset_plan(by_row != 0, max_id, longest, want_hits != 0, ny * nx, steps, aligned != 0, grid_max > 0 ? grid_max : CTK_LEVEL_GRID_MAX);
    out12[0] = p.form; out12[1] = p.vec; out12[2] = p.vpt; out12[3] = p.lds; out12[4] = p.bps; out12[5] = p.blocks; out12[6] = p.grid; out12[7] = p.xcd;
    out12[8] = CTK_SUBSET_BITMAP_BITS; out12[9] = CTK_SUBSET_LDS_IDS; out12[10] = CTK_SUBSET_TABLE_SHARE; out12[11] = CTK_SUBSET_TILES * CTK_SUBSET_THREADS;
    return CTK_OK;
}

// test hook: out3 = { the form of the last k_subset launch on this handle (CTK_SUBSET_BITMAP .. CTK_SUBSET_ROW_GLB of ctk_forms.h, -1
// none yet), 1 vector / 0 scalar, its workgroups }
extern "C" int ctk_debug_subset_form(ctk_handle *h, int64_t *out3)
{
    if (!h || !out3) return ctk_set_error(CTK_E_INVALID, "null argument");
    out3[0] = h->sb_knobs.form; out3[1] = h->sb_vec; out3[2] = h->sb_knobs.grid;
    return CTK_OK;
}

// test hook / experiments (tools/subset_probe.py) for the following k_subset launches on this handle: as ctk_debug_set_reversal
extern "C" int ctk_debug_set_subset(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    return knobs_set("ctk_debug_set_subset", h, &ctk_handle::sb_knobs, xcd_mode, grid_max);
}

// measurement (tools/subset_probe.py): k_subset alone between HIP events on slabs in device memory -- one launch that is not counted,
// then `reps` timed ones; ms2 = {best, mean}.  The counters go on counting over the launches and are not returned.  off == NULL: the
// plain copy kernel over the same two buffers instead (the whole slab rounded down to 16-byte words).
extern "C" int ctk_debug_time_subset(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids,
                                     int64_t n_ids, int invert, int kind, int32_t *out_dev, int want_hits, int want_n_selected, int reps, double *ms2)
{
    const char *who = "ctk_debug_time_subset";
    const SubsetArgs a = {off, n_off, ids, n_ids, invert, kind};
    if (!h || !flag_dev || !ms2 || reps < 1 || T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments", who);
    SubsetShape sh = {};
    if (off) CTKCHK(subset_check(who, h, T, ny, nx, a, sh));
    else if (!out_dev || (((uintptr_t)flag_dev | (uintptr_t)out_dev) & 15) != 0) return ctk_set_error(CTK_E_INVALID, "%s: the copy needs two 16-byte aligned buffers", who);
    if (off && !out_dev && !want_hits && !want_n_selected) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce", who);
    HIPCHK(hipSetDevice(h->device));
    SubsetCall c = {};
    if (off) CTKCHK(subset_table(h, a, sh, want_hits != 0, want_n_selected != 0, c));
    const int64_t npix = (int64_t)ny * nx;
    if (!off) return time_copy16(h, who, h->sb_knobs, flag_dev, out_dev, T * npix * 4, reps, ms2);
    return time_launches(h, who, reps, ms2, [&]() -> int { return launch_subset(h, flag_dev, npix, T, c, 0, out_dev); });
}
