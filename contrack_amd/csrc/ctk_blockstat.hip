// ctk_blockstat.hip -- what a blocking study selects on, per (step, track) row of the life-cycle frame, on the device (included by
// ctk_api.hip): the true peak of a field inside the block and where it sits, and the block's meridional and zonal extent, the latter
// taken around the date line.  include/contrack_hip.h states it, tests/blockstat_util.py is its numpy statement; the key is the ROW
// table of ctk_subset_* (off, ids), checked and uploaded by ctk_subset.hip's subset_check and subset_table.  For entry e = (t, id),
// P the pixels p = row * nx + col of step t with flag == id:
//     n = |P| ;  r0, r1 = the lowest and highest row ;  occ = the columns of P ;  nv = the values of P that are not NaN
//     max, max_p = the largest an_key among them and the lowest p that holds it ;  min, min_p = the smallest and the lowest p
// The column rule (west, width: the complement of the longest CIRCULAR run of unoccupied columns, the lowest start among equally
// long ones) is one of its own -- it is not the life cycle's `shift`, which copies the reference's non-circular
// np.argmax(np.diff(cols)).
//
// Everything is selection -- a count, integer extremes, a bit set, an extreme key with its first position -- so every accumulator is
// an integer that grows under ONE of add, max, or: rows and the lower extreme are kept complemented (~row, ~key), and all-zero bytes
// are the empty state of every one of them.  Nothing depends on the order of the pixels, the kernel form or the chunking.
//
// k_blockstat: k_subset's row geometry (ctk_blockstat_plan, ctk_forms.h).  A workgroup loads the step's slice of ids, binary-searches
// each pixel whose flag is > 0 and reads the field only where the id was found.  CTK_BLOCKSTAT_ROW_LDS keeps the slice's
// accumulators and column bit sets in LDS, updates them with LDS atomics and merges the touched entries into the records in HBM at
// the end of the part with the same operations; CTK_BLOCKSTAT_ROW_GLB does its atomics straight on HBM.  float32: value and first
// position travel in one 64-bit max on (key << 32) | ~p and one on ~((key << 32) | p) (p < 2^31, the table check's condition).
// float64: key and position do not fit one word, so the first launch keeps the extreme keys and a second one, MODE = BS_POS of the
// same kernel, reads again where the id was found and takes the lowest p whose key equals the entry's -- an entry lies in one step
// and so in one chunk, its keys are final when the chunk's first launch is.  k_blockstat_finish: one thread per entry walks its bit
// ring for the longest empty run and unpacks the words into a ctk_block_row.
#pragma once

#define BS_SHAPE 1                     // (= CTK_BLOCK_SHAPE)
#define BS_PEAKS 2                     // (= CTK_BLOCK_PEAKS)
#define BS_POS 4                       // the second launch of float64 peaks

typedef unsigned long long bs_u64;

// the accumulators of a call in HBM, one of each per entry of ids, and W words of column bits per entry; all start from zero bytes
struct BsDev {
    const int64_t *off;                // off[s], off[s + 1] of step s of THIS launch
    const int32_t *ids;
    bs_u64 *A;                         // float32: max of (key << 32) | ~p ;  float64: max of key
    bs_u64 *B;                         // float32: max of ~((key << 32) | p) ;  float64: max of ~key
    uint32_t *cnt, *nv;                // sums
    uint32_t *r0n, *r1p;               // max of ~row, max of row + 1
    uint32_t *pmaxn, *pminn;           // float64: max of ~p over the pixels that hold the entry's largest / smallest key
    uint32_t *bits;
    uint32_t W, nx;
};

// flag, x: (steps, npix).  Part b of `blocks` = bps * steps covers lanes [part * TILES * 256, ...) of step b / bps, as in k_subset.
template <int FORM, bool VEC, int MODE, typename VT>
__global__ __launch_bounds__(CTK_SUBSET_THREADS) void k_blockstat(const int32_t *__restrict__ flag, const VT *__restrict__ x, int64_t npix, int64_t bps,
                                                                  int64_t blocks, BsDev a, int xcd)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
    constexpr bool LDS = FORM == CTK_BLOCKSTAT_ROW_LDS;
    constexpr bool SHAPE = (MODE & BS_SHAPE) != 0, PEAKS = (MODE & BS_PEAKS) != 0, POS = MODE == BS_POS;
    constexpr bool F32 = sizeof(VT) == 4;
    constexpr int N = VEC ? 4 : 1, TILES = CTK_SUBSET_TILES;
    const uint32_t tid = threadIdx.x;
    const int64_t lanes = VEC ? npix / 4 : npix;                                  // lanes of one plane
    const uint32_t W = a.W, nx = a.nx;
    ctk_const_i64 *off = (ctk_const_i64 *)a.off;                                  // (the step is the workgroup's: scalar loads)
    bool used = false;                                                            // this workgroup has had a slice in LDS
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b < blocks; b += gridDim.x) {
        const int64_t s = b / bps;
        const int64_t base = off[s];
        const uint32_t n = (uint32_t)(off[s + 1] - base);
        if (n == 0) continue;                                                     // nothing is wanted at this step (the whole workgroup leaves)
        const int64_t q0 = (b - s * bps) * (TILES * CTK_SUBSET_THREADS) + tid;    // this thread's lane of the first tile
        const int32_t *fs = flag + s * npix;                                      // (64-bit throughout)
        i32x4 v[TILES];
#pragma unroll
        for (int k = 0; k < TILES; k++) {                                         // all loads of the part are issued before the first is used
            const int64_t q = q0 + k * CTK_SUBSET_THREADS;
            v[k] = i32x4{0, 0, 0, 0};
            if (q < lanes) {
                if (VEC) v[k] = __builtin_nontemporal_load((const i32x4 *)(fs + q * 4));
                else v[k].x = fs[q];
            }
        }
        // the slice's accumulators: in LDS [A | B | ids | cnt | nv | r0n | r1p | bits] (BS_POS: cnt and nv hold pmaxn and pminn), or in HBM
        bs_u64 *A = (bs_u64 *)sm, *B = A + n;
        uint32_t *sid = (uint32_t *)(B + n), *cnt = sid + n, *nv = cnt + n, *r0n = nv + n, *r1p = r0n + n, *bits = r1p + n;
        if (LDS) {
            if (used) __syncthreads();                                            // (the part before this one has left the slice)
            used = true;
            for (uint32_t i = tid; i < n; i += CTK_SUBSET_THREADS) {
                sid[i] = (uint32_t)a.ids[base + i];
                A[i] = POS ? a.A[base + i] : 0; B[i] = POS ? a.B[base + i] : 0;
                cnt[i] = 0; nv[i] = 0; r0n[i] = 0; r1p[i] = 0;
            }
            if (SHAPE)
                for (uint32_t i = tid; i < n * W; i += CTK_SUBSET_THREADS) bits[i] = 0;
            __syncthreads();
        } else {
            A = a.A + base; B = a.B + base;
            cnt = (POS ? a.pmaxn : a.cnt) + base; nv = (POS ? a.pminn : a.nv) + base; r0n = a.r0n + base; r1p = a.r1p + base;
            bits = a.bits + base * (int64_t)W;
        }
        const VT *xs = (PEAKS || POS) ? x + s * npix : nullptr;
        auto pixel = [&](int32_t f, uint32_t p, uint32_t row, uint32_t col) {
            if (f <= 0) return;
            const uint32_t e = LDS ? subset_find((const int32_t *)sid, n, f) : subset_find(a.ids + base, n, f);
            if (e >= n) return;
            if (!POS) {
                atomicAdd(&cnt[e], 1u);
                if (SHAPE) {
                    atomicMax(&r0n[e], ~row);
                    atomicMax(&r1p[e], row + 1);
                    atomicOr(&bits[e * W + (col >> 5)], 1u << (col & 31));
                }
            }
            if (PEAKS || POS) {
                const VT val = xs[p];                                             // (read only where the id was found)
                if (an_isnan(val)) return;
                if (PEAKS) {
                    atomicAdd(&nv[e], 1u);
                    if constexpr (F32) {
                        const bs_u64 hi = (bs_u64)an_key(val) << 32;
                        atomicMax(&A[e], hi | (uint32_t)~p);
                        atomicMax(&B[e], ~(hi | p));
                    } else {
                        const bs_u64 k = an_key(val);
                        atomicMax(&A[e], k);
                        atomicMax(&B[e], ~k);
                    }
                } else if constexpr (!F32) {                                      // BS_POS: the keys are final, A and B are only read
                    const bs_u64 k = an_key(val);
                    if (k == A[e]) atomicMax(&cnt[e], ~p);
                    if (~k == B[e]) atomicMax(&nv[e], ~p);
                }
            }
        };
#pragma unroll
        for (int k = 0; k < TILES; k++) {
            const int64_t q = q0 + k * CTK_SUBSET_THREADS;
            if (q >= lanes) continue;
            if (!(v[k].x > 0 || (N == 4 && (v[k].y > 0 || v[k].z > 0 || v[k].w > 0)))) continue;       // background first: most lanes stop here
            const uint32_t p = (uint32_t)(q * N);                                 // (a plane has fewer than 2^31 pixels)
            uint32_t row = p / nx, col = p - row * nx;
            pixel(v[k].x, p, row, col);
            if (N == 4) {
                if (++col == nx) { col = 0; row++; }
                pixel(v[k].y, p + 1, row, col);
                if (++col == nx) { col = 0; row++; }
                pixel(v[k].z, p + 2, row, col);
                if (++col == nx) { col = 0; row++; }
                pixel(v[k].w, p + 3, row, col);
            }
        }
        if (LDS) {                                                                // the touched entries meet the records in HBM
            __syncthreads();
            for (uint32_t i = tid; i < n; i += CTK_SUBSET_THREADS) {
                if (POS) {
                    if (cnt[i]) atomicMax(a.pmaxn + base + i, cnt[i]);
                    if (nv[i]) atomicMax(a.pminn + base + i, nv[i]);
                } else if (cnt[i]) {
                    atomicAdd(a.cnt + base + i, cnt[i]);
                    if (SHAPE) { atomicMax(a.r0n + base + i, r0n[i]); atomicMax(a.r1p + base + i, r1p[i]); }
                    if (PEAKS && nv[i]) { atomicAdd(a.nv + base + i, nv[i]); atomicMax(a.A + base + i, A[i]); atomicMax(a.B + base + i, B[i]); }
                }
            }
            if (SHAPE)
                for (uint32_t i = tid; i < n * W; i += CTK_SUBSET_THREADS) {
                    const uint32_t w = bits[i];
                    if (w) atomicOr(a.bits + base * (int64_t)W + i, w);
                }
        }
    }
}

// one thread per entry: the accumulators as the ctk_block_row the header states.  Walks the ring of nx column bits once, from the
// first occupied column round to itself, so every empty run is closed when the walk ends.
template <bool F64>
__global__ __launch_bounds__(256) void k_blockstat_finish(BsDev a, int64_t n_ids, int want, ctk_block_row *__restrict__ rows)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ids) return;
    ctk_block_row r;
    r.n = a.cnt[e]; r.nv = 0;
    r.r0 = r.r1 = r.west = -1; r.width = 0;
    r.max_p = r.min_p = -1;
    r.max = r.min = __longlong_as_double(0x7ff8000000000000ll);
    if (r.n && (want & BS_SHAPE)) {
        r.r0 = (int32_t)~a.r0n[e]; r.r1 = (int32_t)a.r1p[e] - 1;
        const uint32_t *bits = a.bits + e * (int64_t)a.W;
        const int32_t nx = (int32_t)a.nx;
        auto occ = [&](int32_t c) { return (bits[c >> 5] >> (c & 31)) & 1u; };
        int32_t c0 = 0;
        while (c0 < nx && !occ(c0)) c0++;                                         // (n > 0: there is one)
        int32_t best = 0, best_s = 0, run = 0, start = 0;
        for (int32_t i = 1; i <= nx && c0 < nx; i++) {
            int32_t c = c0 + i;
            if (c >= nx) c -= nx;
            if (!occ(c)) { if (!run) start = c; run++; }
            else if (run) {
                if (run > best || (run == best && start < best_s)) { best = run; best_s = start; }
                run = 0;
            }
        }
        r.west = best ? (best_s + best) % nx : 0;
        r.width = nx - best;
    }
    if (r.n && (want & BS_PEAKS) && a.nv[e]) {
        r.nv = a.nv[e];
        const bs_u64 A = a.A[e], B = ~a.B[e];
        if (F64) {
            r.max = an_unkey((uint64_t)A); r.min = an_unkey((uint64_t)B);
            r.max_p = (int64_t)(uint32_t)~a.pmaxn[e]; r.min_p = (int64_t)(uint32_t)~a.pminn[e];
        } else {
            r.max = (double)an_unkey((uint32_t)(A >> 32)); r.min = (double)an_unkey((uint32_t)(B >> 32));       // (a float32 widens exactly)
            r.max_p = (int64_t)(uint32_t)~(uint32_t)A; r.min_p = (int64_t)(uint32_t)B;
        }
    }
    rows[e] = r;
}

// the yardstick of tools/blockstat_probe.py: 16-byte loads over two buffers and nothing else (the sum is stored by no lane that
// loaded anything but ones: the loads stay, the store never happens on real data)
__global__ __launch_bounds__(256) void k_load16x2(const i32x4 *__restrict__ p0, int64_t n0, const i32x4 *__restrict__ p1, int64_t n1, int32_t *sink, int xcd)
{
    int32_t acc = 0;
    const int64_t n = n0 > n1 ? n0 : n1;
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b * 256 < n; b += gridDim.x) {
        const int64_t i = b * 256 + threadIdx.x;
        if (i < n0) { const i32x4 v = __builtin_nontemporal_load(p0 + i); acc |= v.x & v.y & v.z & v.w; }
        if (i < n1) { const i32x4 v = __builtin_nontemporal_load(p1 + i); acc |= v.x & v.y & v.z & v.w; }
    }
    if (acc == -1 && sink) sink[threadIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// a call: its checked table on the device (subset_table), the accumulators in bs_acc zeroed, the rows in bs_rows
struct BlockstatCall {
    SubsetCall tab;
    BsDev d;
    int want;
    bool f64;
    int nx;
    int64_t n_ids;
};

// everything the entries refuse, in one place: the table through subset_check, then what is this family's own
static int blockstat_check(const char *who, ctk_handle *h, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids, int want,
                           const void *rows, SubsetArgs &a, SubsetShape &sh)
{
    a = SubsetArgs{off, n_off, ids, n_ids, 0, CTK_SUBSET_ID};
    if (h && off && T >= 1 && n_off != T + 1)
        return ctk_set_error(CTK_E_INVALID, "%s: n_off = %lld (a row table: T + 1 = %lld; there is no by-id reading here)", who, (long long)n_off, (long long)(T + 1));
    CTKCHK(subset_check(who, h, T, ny, nx, a, sh));
    if (want == 0 || (want & ~(CTK_BLOCK_SHAPE | CTK_BLOCK_PEAKS)))
        return ctk_set_error(CTK_E_INVALID, "%s: want = %d (CTK_BLOCK_SHAPE | CTK_BLOCK_PEAKS, at least one)", who, want);
    if (!rows && n_ids > 0) return ctk_set_error(CTK_E_INVALID, "%s: null rows", who);
    return CTK_OK;
}

// x == NULL with peaks wanted: the resident anomaly slab of the call's shape and type (comp_resident's test), or the call is refused
static int blockstat_resident(const char *who, ctk_handle *h, bool f64, int64_t T, int ny, int nx, const void **x_dev)
{
    *x_dev = h->an_slab.find(T, ny, nx, f64);
    if (!*x_dev)
        return ctk_set_error(CTK_E_INVALID, "%s: peaks wanted and no field given, which needs a resident anomaly slab of this shape and type (ctk_anom_* with keep_resident)", who);
    return CTK_OK;
}

static int blockstat_begin(ctk_handle *h, const SubsetArgs &a, const SubsetShape &sh, int nx, int want, bool f64, BlockstatCall &c)
{
    c.want = want; c.f64 = f64; c.nx = nx; c.n_ids = a.n_ids;
    CTKCHK(subset_table(h, a, sh, false, false, c.tab));
    const size_t N = (size_t)a.n_ids, W = (want & CTK_BLOCK_SHAPE) ? ((size_t)nx + 31) / 32 : 0;
    const size_t bytes = N * (16 + 24 + 4 * W);
    CTKCHK(ensure(h, h->bs_acc, bytes));
    CTKCHK(ensure(h, h->bs_rows, N * sizeof(ctk_block_row)));
    HIPCHK(hipMemsetAsync(h->bs_acc.p, 0, bytes, h->stream));
    BsDev &d = c.d;
    d.off = c.tab.off_dev; d.ids = c.tab.d.ids;
    d.A = P<bs_u64>(h->bs_acc); d.B = d.A + N;
    d.cnt = (uint32_t *)(d.B + N); d.nv = d.cnt + N; d.r0n = d.nv + N; d.r1p = d.r0n + N; d.pmaxn = d.r1p + N; d.pminn = d.pmaxn + N; d.bits = d.pminn + N;
    d.W = (uint32_t)W; d.nx = (uint32_t)nx;
    return CTK_OK;
}

template <int FORM, bool VEC>
static void blockstat_launch_form(const CtkBlockstatPlan &pl, hipStream_t st, int mode, bool f64, const int32_t *flag, const void *x, int64_t npix, const BsDev &d, int xcd)
{
#define CTK_BS_LAUNCH(M, VT) k_blockstat<FORM, VEC, M, VT><<<pl.grid, CTK_SUBSET_THREADS, (size_t)pl.lds, st>>>(flag, (const VT *)x, npix, pl.bps, pl.blocks, d, xcd)
    switch (mode) {
    case BS_SHAPE: CTK_BS_LAUNCH(BS_SHAPE, float); break;
    case BS_PEAKS: if (f64) CTK_BS_LAUNCH(BS_PEAKS, double); else CTK_BS_LAUNCH(BS_PEAKS, float); break;
    case BS_SHAPE | BS_PEAKS: if (f64) CTK_BS_LAUNCH(BS_SHAPE | BS_PEAKS, double); else CTK_BS_LAUNCH(BS_SHAPE | BS_PEAKS, float); break;
    default: CTK_BS_LAUNCH(BS_POS, double); break;
    }
#undef CTK_BS_LAUNCH
}

// the steps [step0, step0 + steps) of the call's table from flag (steps, npix) and x (the same steps; null without peaks) into the
// accumulators, on the handle's stream
static int launch_blockstat(ctk_handle *h, const int32_t *flag, const void *x, int64_t npix, int64_t steps, const BlockstatCall &c, int64_t step0)
{
    const bool peaks = (c.want & CTK_BLOCK_PEAKS) != 0;
    const CtkBlockstatPlan pl = ctk_blockstat_plan((c.want & CTK_BLOCK_SHAPE) != 0, peaks, c.f64 ? 8 : 4, c.tab.sh.longest, c.nx, npix, steps,
                                                   ((uintptr_t)flag & 15) == 0, h->bs_knobs.cap());
    h->bs_knobs.launched(pl.form, pl.grid); h->bs_vec = pl.vec;
    const int xcd = h->bs_knobs.xcd(pl.xcd);
    BsDev d = c.d;
    d.off = c.tab.off_dev + step0;
    for (int pass = 0; pass < pl.passes; pass++) {
        const int mode = pass ? BS_POS : c.want;
        if (pl.form == CTK_BLOCKSTAT_ROW_LDS) {
            if (pl.vec) blockstat_launch_form<CTK_BLOCKSTAT_ROW_LDS, true>(pl, h->stream, mode, c.f64, flag, x, npix, d, xcd);
            else blockstat_launch_form<CTK_BLOCKSTAT_ROW_LDS, false>(pl, h->stream, mode, c.f64, flag, x, npix, d, xcd);
        } else {
            if (pl.vec) blockstat_launch_form<CTK_BLOCKSTAT_ROW_GLB, true>(pl, h->stream, mode, c.f64, flag, x, npix, d, xcd);
            else blockstat_launch_form<CTK_BLOCKSTAT_ROW_GLB, false>(pl, h->stream, mode, c.f64, flag, x, npix, d, xcd);
        }
        HIPCHK(hipGetLastError());
    }
    return CTK_OK;
}

// the records of a finished call as rows, copied out once
static int blockstat_end(ctk_handle *h, const BlockstatCall &c, ctk_block_row *rows)
{
    ctk_block_row *rdev = P<ctk_block_row>(h->bs_rows);
    const unsigned grid = (unsigned)((c.n_ids + 255) / 256);
    if (c.f64) k_blockstat_finish<true><<<grid, 256, 0, h->stream>>>(c.d, c.n_ids, c.want, rdev);
    else k_blockstat_finish<false><<<grid, 256, 0, h->stream>>>(c.d, c.n_ids, c.want, rdev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(rows, rdev, (size_t)c.n_ids * sizeof(ctk_block_row), hipMemcpyDeviceToHost));
    return CTK_OK;
}

static int blockstat_dev_impl(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, bool f64, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                              const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows, const char *who)
{
    SubsetArgs a;
    SubsetShape sh;
    CTKCHK(blockstat_check(who, h, T, ny, nx, off, n_off, ids, n_ids, want, rows, a, sh));
    if (!flag_dev) return ctk_set_error(CTK_E_INVALID, "%s: null flag", who);
    if ((want & CTK_BLOCK_PEAKS) && !x_dev) CTKCHK(blockstat_resident(who, h, f64, T, ny, nx, &x_dev));
    if (n_ids == 0) return CTK_OK;
    HIPCHK(hipSetDevice(h->device));
    BlockstatCall c;
    CTKCHK(blockstat_begin(h, a, sh, nx, want, f64, c));
    CTKCHK(launch_blockstat(h, flag_dev, (want & CTK_BLOCK_PEAKS) ? x_dev : nullptr, (int64_t)ny * nx, T, c, 0));
    return blockstat_end(h, c, rows);
}

extern "C" int ctk_blockstat_f32_dev(ctk_handle *h, const int32_t *flag_dev, const float *x_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                                     const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows)
{
    return blockstat_dev_impl(h, flag_dev, x_dev, false, T, ny, nx, off, n_off, ids, n_ids, want, rows, "ctk_blockstat_f32_dev");
}
extern "C" int ctk_blockstat_f64_dev(ctk_handle *h, const int32_t *flag_dev, const double *x_dev, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                                     const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows)
{
    return blockstat_dev_impl(h, flag_dev, x_dev, true, T, ny, nx, off, n_off, ids, n_ids, want, rows, "ctk_blockstat_f64_dev");
}

// host arrays or reader callbacks: the field is stream_consume's first slab and the flags its second, exactly as comp_stream_impl
// has them; `travels` false -- the field is resident or not wanted -- and the flags are the only slab on its way.  The records stay
// in HBM until the last chunk.
static int blockstat_stream_impl(ctk_handle *h, StreamIO &io, bool f64, bool have_field, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                                 const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps, const char *who)
{
    SubsetArgs a;
    SubsetShape sh;
    CTKCHK(blockstat_check(who, h, T, ny, nx, off, n_off, ids, n_ids, want, rows, a, sh));
    if (!io.read && !io.host_in) return ctk_set_error(CTK_E_INVALID, "%s: null flag", who);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", who, (long long)chunk_steps);
    const bool peaks = (want & CTK_BLOCK_PEAKS) != 0, travels = peaks && have_field;
    const void *res_dev = nullptr;
    if (peaks && !have_field) CTKCHK(blockstat_resident(who, h, f64, T, ny, nx, &res_dev));
    if (n_ids == 0) return CTK_OK;
    HIPCHK(hipSetDevice(h->device));
    const int64_t npix = (int64_t)ny * nx;
    const size_t esz = f64 ? 8 : 4;
    io.esz = travels ? esz : 4;
    io.esz2 = travels ? 4 : 0;
    io.chunk = ctk_stream_chunk(chunk_steps, T, (size_t)npix * io.esz);
    BlockstatCall c;
    CTKCHK(blockstat_begin(h, a, sh, nx, want, f64, c));
    const double t0 = now_ms();
    CTKCHK(stream_consume(h, io, f64, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        const int32_t *fl = travels ? (const int32_t *)io.dev2 : (const int32_t *)chunk;
        const void *xv = travels ? chunk : res_dev ? (const void *)((const char *)res_dev + (size_t)c0 * npix * esz) : nullptr;
        return launch_blockstat(h, fl, xv, npix, nt, c, c0);
    }));
    CTKCHK(blockstat_end(h, c, rows));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

static int blockstat_host_impl(ctk_handle *h, const int32_t *flag, const void *x, bool f64, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off,
                               const int32_t *ids, int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps, const char *who)
{
    StreamIO io;
    const bool travels = x && (want & CTK_BLOCK_PEAKS);
    if (travels) { io.host_in = x; io.host_in2 = flag; }
    else io.host_in = flag;
    if (h && !flag) return ctk_set_error(CTK_E_INVALID, "%s: null flag", who);
    return blockstat_stream_impl(h, io, f64, x != nullptr, T, ny, nx, off, n_off, ids, n_ids, want, rows, chunk_steps, who);
}

extern "C" int ctk_blockstat_f32(ctk_handle *h, const int32_t *flag, const float *x, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids,
                                 int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps)
{
    return blockstat_host_impl(h, flag, x, false, T, ny, nx, off, n_off, ids, n_ids, want, rows, chunk_steps, "ctk_blockstat_f32");
}
extern "C" int ctk_blockstat_f64(ctk_handle *h, const int32_t *flag, const double *x, int64_t T, int ny, int nx, const int64_t *off, int64_t n_off, const int32_t *ids,
                                 int64_t n_ids, int want, ctk_block_row *rows, int64_t chunk_steps)
{
    return blockstat_host_impl(h, flag, x, true, T, ny, nx, off, n_off, ids, n_ids, want, rows, chunk_steps, "ctk_blockstat_f64");
}
extern "C" int ctk_blockstat_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user,
                                ctk_read_chunk_fn field_reader, void *field_user, const int64_t *off, int64_t n_off, const int32_t *ids, int64_t n_ids, int want,
                                ctk_block_row *rows, int64_t chunk_steps)
{
    const char *who = "ctk_blockstat_cb";
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "%s: elem_bytes must be 4 (float32) or 8 (float64)", who);
    if (h && !flag_reader) return ctk_set_error(CTK_E_INVALID, "%s: null flag reader", who);
    StreamIO io;
    const bool travels = field_reader && (want & CTK_BLOCK_PEAKS);
    if (travels) { io.read = field_reader; io.read_user = field_user; io.read2 = flag_reader; io.read2_user = flag_user; }
    else { io.read = flag_reader; io.read_user = flag_user; }
    return blockstat_stream_impl(h, io, elem_bytes == 8, field_reader != nullptr, T, ny, nx, off, n_off, ids, n_ids, want, rows, chunk_steps, who);
}

// what ctk_blockstat_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_blockstat_plan(int want, int elem_bytes, int64_t longest, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t grid_max, int64_t *out14)
{
    if (!out14 || want == 0 || (want & ~(CTK_BLOCK_SHAPE | CTK_BLOCK_PEAKS)) || (elem_bytes != 4 && elem_bytes != 8) || longest < 0 || ny < 1 || nx < 1 || steps < 1 ||
        ny * nx > 0x7fffffffll || grid_max < 0)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_blockstat_plan: bad arguments");
    const CtkBlockstatPlan p = ctk_blockstat_plan((want & CTK_BLOCK_SHAPE) != 0, (want & CTK_BLOCK_PEAKS) != 0, elem_bytes, longest, nx, ny * nx, steps, aligned != 0,
                                                  grid_max > 0 ? grid_max : CTK_LEVEL_GRID_MAX);
    out14[0] = p.form; out14[1] = p.vec; out14[2] = p.vpt; out14[3] = p.lds; out14[4] = p.bps; out14[5] = p.blocks; out14[6] = p.grid; out14[7] = p.xcd;
    out14[8] = p.passes; out14[9] = p.words; out14[10] = p.entry; out14[11] = CTK_BLOCKSTAT_LDS_BYTES; out14[12] = CTK_BLOCKSTAT_LDS_BYTES / p.entry;
    out14[13] = CTK_SUBSET_TILES * CTK_SUBSET_THREADS;
    return CTK_OK;
}

// test hook / experiments for the following k_blockstat launches on this handle: as ctk_debug_set_level
extern "C" int ctk_debug_set_blockstat(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    return knobs_set("ctk_debug_set_blockstat", h, &ctk_handle::bs_knobs, xcd_mode, grid_max);
}

// test hook: out3 = { the form of the last k_blockstat launch on this handle (-1 none yet), 1 vector / 0 scalar, its workgroups }
extern "C" int ctk_debug_blockstat_form(ctk_handle *h, int64_t *out3)
{
    if (!h || !out3) return ctk_set_error(CTK_E_INVALID, "null argument");
    out3[0] = h->bs_knobs.form; out3[1] = h->bs_vec; out3[2] = h->bs_knobs.grid;
    return CTK_OK;
}

// measurement (tools/blockstat_probe.py): the launches of k_blockstat for the whole slab alone between HIP events on slabs in device
// memory -- one round that is not counted, then `reps` timed ones; ms2 = {best, mean}.  The records go on accumulating and are not
// returned.  off == NULL: k_load16x2, 16-byte loads over the flag slab and (x_dev given) the field slab, the yardstick.
extern "C" int ctk_debug_time_blockstat(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int is_f64, int64_t T, int ny, int nx, const int64_t *off,
                                        int64_t n_off, const int32_t *ids, int64_t n_ids, int want, int reps, double *ms2)
{
    const char *who = "ctk_debug_time_blockstat";
    if (!h || !flag_dev || !ms2 || reps < 1 || T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments", who);
    const int64_t npix = (int64_t)ny * nx;
    const bool f64 = is_f64 != 0;
    HIPCHK(hipSetDevice(h->device));
    if (!off) {
        if ((((uintptr_t)flag_dev | (uintptr_t)x_dev) & 15) != 0) return ctk_set_error(CTK_E_INVALID, "%s: the load stream needs 16-byte aligned buffers", who);
        const int64_t n0 = T * npix * 4 / 16, n1 = x_dev ? T * npix * (f64 ? 8 : 4) / 16 : 0;
        const unsigned grid = (unsigned)std::min<int64_t>(std::max<int64_t>((std::max(n0, n1) + 255) / 256, 1), CTK_LEVEL_GRID_MAX);
        const int xcd = h->bs_knobs.xcd(grid >= CTK_LEVEL_XCD_MIN ? 1 : 0);
        return time_launches(h, who, reps, ms2, [&]() -> int {
            k_load16x2<<<grid, 256, 0, h->stream>>>((const i32x4 *)flag_dev, n0, (const i32x4 *)x_dev, n1, nullptr, xcd);
            HIPCHK(hipGetLastError());
            return CTK_OK;
        });
    }
    SubsetArgs a;
    SubsetShape sh;
    CTKCHK(blockstat_check(who, h, T, ny, nx, off, n_off, ids, n_ids, want, ms2, a, sh));
    if ((want & CTK_BLOCK_PEAKS) && !x_dev) return ctk_set_error(CTK_E_INVALID, "%s: peaks need a field", who);
    if (n_ids == 0) return ctk_set_error(CTK_E_INVALID, "%s: an empty table", who);
    BlockstatCall c;
    CTKCHK(blockstat_begin(h, a, sh, nx, want, f64, c));
    return time_launches(h, who, reps, ms2, [&]() -> int { return launch_blockstat(h, flag_dev, x_dev, npix, T, c, 0); });
}
