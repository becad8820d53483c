// ctk_centred.hip -- the composite in the block's own frame of reference, on the device (included by ctk_api.hip): the sum of a field in
// a window of (2 hy + 1) x (2 hx + 1) grid points that moves with a list of R stamps (t, row, col) -- the centres of mass that
// run_lifecycle gives per (time step, block) -- binned by a life-cycle age per stamp, and how many values there were:
//     for r = 0 .. R-1 RISING, bin[r] >= 0, j in -hy..hy, i in -hx..hx:
//         y = row[r] + j (inside the grid, no step over a pole);  c = col[r] + i (wrap: mod nx, else inside the grid)
//         sum[bin[r]][j + hy][i + hx] += (double)x[t[r]][y][c];   n[...] += 1                        (float64 from +0.0, uint32)
// (with skipna a NaN value is not counted; the mean sum / n is left to the caller).  The reference has no function for it,
// include/contrack_hip.h states the definition and tests/centred_util.py is its numpy statement.
//
// k_centred: one lane owns a cell (bin, j, i) for ALL stamps of a launch.  Float64 addition is not associative, so a bin's stamps are
// never split over threads and nothing is added atomically: a cell meets its bin's stamps in the order given, which is what makes the
// result reproducible bit for bit.  It is the rule of k_composite with the time axis replaced by the stamp list.  The host sorts the
// stamps by bin with a stable counting sort (centred_csr: the given order survives inside a bin, bin < 0 is dropped there) and hands
// the kernel bin offsets plus 16-byte stamps in bin order; a workgroup works on one bin, so its stamps are wave-uniform and come
// through the constant address space as scalar loads, not one per lane.  Lanes of a wave take consecutive i: a wave's
// gather of one stamp is a few contiguous row segments, each split at most once by the longitude wrap.
//
// Parallelism (ctk_centred_plan, ctk_forms.h).  There are few cells and each is a long chain of dependent adds behind gathers.
// k_centred, the plain form: the loads of a batch of stamps -- 32 float32 or 16 float64, 128 bytes per lane -- are issued together and
// added in order afterwards, as comp_batch does; and while a launch has few workgroups they are single waves, so that a window's
// cells spread over as many CUs as there are waves.  With many bins (by = 'age') that fills the chip.  With one bin of all blocks it
// does not: 3321 cells of a 41 x 81 window are 52 waves, each behind one scalar and one vector memory latency per batch of 32 stamps.
// k_centred_fed, the fed form, is for that: 64 cells per workgroup of 16 waves; 15 feeder waves gather 8 (float64: 4) stamps each into
// one half of an LDS buffer, the owner wave adds those 120 (60) values in stamp order out of the other half while the feeders fetch the
// next -- the hand-over k_life_exact uses for its chains.  One barrier per round; the order of the additions is the plain form's.
// The accumulators, 12 bytes per cell, live in HBM: the owning lane loads its pair once, keeps it in registers and stores it once.
// Launches on the handle's stream are ordered and continue from the stored pair: that is how chunks (and a caller's own pieces,
// accumulate = 1) keep the stamp order.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage), the same for all instantiations of a kernel
// and type up to a few registers: see the tables at k_centred and k_centred_fed.
#pragma once

// a stamp as the kernel reads it: base = the element offset of (t, row 0, col 0) in the slab the launch sees -- (t - c0) * rows - y0
// planes of `rows` latitude rows that start at row y0 of the grid, times nx: it may be negative, base + y * nx + c never is
struct CtkStamp {
    int64_t base;
    int32_t row, col;
};
typedef const __attribute__((address_space(4))) CtkStamp ctk_const_stamp;                 // a wave-uniform index into it: s_loads
typedef const __attribute__((address_space(4))) uint32_t ctk_const_u32;

struct CentredArgs {
    const void *x;                // the slab (or the band of it) of the launch
    const CtkStamp *st;           // stamps in bin order
    const uint32_t *off;          // nbins + 1 offsets into st
    double *sum;                  // [nbins][2 hy + 1][2 hx + 1]
    uint32_t *cnt;
    int64_t blocks, parts;        // nbins * parts workgroup-sized pieces; parts per bin
    int32_t ny, nx, hy, hx, wcells, umax;
};

// stamps s .. s + U - 1 of the lane's bin: all U loads first (those inside the grid), then the sums in rising s
template <typename VT, bool SKIPNA, bool WRAP, int U>
__device__ __forceinline__ void centred_batch(const VT *__restrict__ x, ctk_const_stamp *st, uint32_t s, int j, int i, int ny, int nx, double &acc, uint32_t &n)
{
    VT v[U];
    uint32_t in = 0;
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int64_t base = st[s + u].base;
        const int y = st[s + u].row + j;
        int c = st[s + u].col + i;
        bool ok = (unsigned)y < (unsigned)ny;
        if (WRAP) { c += c < 0 ? nx : 0; c -= c >= nx ? nx : 0; }                 // (2 hx + 1 <= nx: once is enough)
        else ok = ok && (unsigned)c < (unsigned)nx;
        if (ok) { v[u] = x[base + (int64_t)y * nx + c]; in |= 1u << u; }            // (64-bit element offsets throughout)
    }
#pragma unroll
    for (int u = 0; u < U; u++)
        if ((in >> u) & 1u) {
            const double xv = (double)v[u];                                         // (a plain conversion: denormals kept)
            if (!SKIPNA || xv == xv) { acc = acc + xv; n++; }
        }
}

// Workgroup b of `blocks` takes part b % parts of bin b / parts.  umax: the widest batch (a power of two, at most
// CTK_CENTRED_UNROLL_MAX); the rest of the bin's stamps goes in ever shorter batches.
//                                     VGPRs    SGPRs  scratch  LDS   occupancy (waves per SIMD)
//   float32, any SKIPNA / WRAP        78-80     65       0      0     6
//   float64, any SKIPNA / WRAP        112-114   65       0      0     4
// (SGPRs within the 80 of CTK_SGPR_8WAVES, ctk_kernels.hip; the VGPRs are the batch: 32 values and the 64-bit addresses of the loads
// in flight.  Occupancy is not what limits a launch of a few dozen to a few thousand waves on 1024 SIMDs.)
template <typename VT, bool SKIPNA, bool WRAP>
__global__ __launch_bounds__(CTK_CENTRED_THREADS_MAX) CTK_SGPR_8WAVES void k_centred(const CentredArgs a)
{
    const VT *__restrict__ x = (const VT *)a.x;
    ctk_const_stamp *st = (ctk_const_stamp *)a.st;
    ctk_const_u32 *off = (ctk_const_u32 *)a.off;
    const int W = 2 * a.hx + 1;
    for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        const int64_t bin = b / a.parts;
        const int wc = (int)(b - bin * a.parts) * (int)blockDim.x + (int)threadIdx.x;          // this lane's cell of the window
        const uint32_t s1 = off[bin + 1];
        uint32_t s = off[bin];
        if (wc >= a.wcells || s == s1) continue;
        const int j = wc / W - a.hy, i = wc % W - a.hx;
        const int64_t at = bin * (int64_t)a.wcells + wc;
        double acc = a.sum[at];
        uint32_t n = a.cnt[at];
#define CTK_CENTRED_BATCH(U) centred_batch<VT, SKIPNA, WRAP, U>(x, st, s, j, i, a.ny, a.nx, acc, n)
        for (; a.umax >= 32 && s1 - s >= 32; s += 32) CTK_CENTRED_BATCH(32);
        for (; a.umax >= 16 && s1 - s >= 16; s += 16) CTK_CENTRED_BATCH(16);
        for (; a.umax >= 8 && s1 - s >= 8; s += 8) CTK_CENTRED_BATCH(8);
        for (; a.umax >= 4 && s1 - s >= 4; s += 4) CTK_CENTRED_BATCH(4);
        for (; a.umax >= 2 && s1 - s >= 2; s += 2) CTK_CENTRED_BATCH(2);
        for (; s < s1; s++) CTK_CENTRED_BATCH(1);
#undef CTK_CENTRED_BATCH
        a.sum[at] = acc;
        a.cnt[at] = n;
    }
}

// The fed form.  Workgroup b of `blocks` takes cells 64 * (b % parts) .. + 63 of bin b / parts: lane l of every wave stands for cell l.
// Waves 1 .. 15 are feeders: in round r feeder w gathers the bin's stamps s + (w - 1) * U .. + U - 1 (U = 8 float32 / 4 float64) for
// its cell into val[r & 1] and says in msk[r & 1] which of them count (inside the grid and, with SKIPNA, not NaN).  Wave 0 owns the
// cells: after the round's barrier it adds the F * U values in slot order -- stamp order -- while the feeders are already in round
// r + 1, writing the other half.  A half is written again in round r + 2, behind barrier r + 1, which the owner reaches only after it
// has finished with round r: one barrier per round is enough; the parity runs on over the workgroup's blocks for the same reason.
//                                     VGPRs  SGPRs  scratch  LDS (bytes)   workgroups per CU
//   float32, any SKIPNA / WRAP        30-36   68     0      69120         2
//   float64, any SKIPNA / WRAP        29-31   66     0      69120         2
template <typename VT, bool SKIPNA, bool WRAP>
__global__ __launch_bounds__(64 * CTK_CENTRED_FED_WAVES) void k_centred_fed(const CentredArgs a)
{
    constexpr int U = CTK_CENTRED_FED_BYTES / (int)sizeof(VT), F = CTK_CENTRED_FED_WAVES - 1, K = F * U;
    __shared__ VT val[2][K][64];
    __shared__ uint32_t msk[2][F][64];
    const VT *__restrict__ x = (const VT *)a.x;
    ctk_const_stamp *st = (ctk_const_stamp *)a.st;
    ctk_const_u32 *off = (ctk_const_u32 *)a.off;
    const int W = 2 * a.hx + 1;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int half = 0;
    for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        const int64_t bin = b / a.parts;
        const int wc = (int)(b - bin * a.parts) * 64 + lane;                        // this lane's cell of the window
        const uint32_t s0 = off[bin], s1 = off[bin + 1];
        if (s0 == s1) continue;                                                     // (the whole workgroup: no barrier is left out)
        const bool live = wc < a.wcells;
        const int j = wc / W - a.hy, i = wc % W - a.hx;
        const int64_t at = bin * (int64_t)a.wcells + wc;
        double acc = 0.0;
        uint32_t n = 0;
        if (w == 0 && live) { acc = a.sum[at]; n = a.cnt[at]; }
        for (uint32_t s = s0; s < s1; s += K, half ^= 1) {
            const uint32_t left = s1 - s;                                           // (slots at and beyond `left` are not read)
            if (w > 0) {
                const uint32_t k0 = (uint32_t)(w - 1) * U;
                VT v[U];
                uint32_t in = 0;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    v[u] = (VT)0;
                    if (k0 + u < left && live) {
                        const int64_t base = st[s + k0 + u].base;
                        const int y = st[s + k0 + u].row + j;
                        int c = st[s + k0 + u].col + i;
                        bool ok = (unsigned)y < (unsigned)a.ny;
                        if (WRAP) { c += c < 0 ? a.nx : 0; c -= c >= a.nx ? a.nx : 0; }
                        else ok = ok && (unsigned)c < (unsigned)a.nx;
                        if (ok) { v[u] = x[base + (int64_t)y * a.nx + c]; in |= 1u << u; }
                    }
                }
                if (k0 < left) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (SKIPNA && v[u] != v[u]) in &= ~(1u << u);
                        val[half][k0 + u][lane] = v[u];
                    }
                    msk[half][w - 1][lane] = in;
                }
            }
            __syncthreads();
            if (w == 0 && live) {
                for (uint32_t f = 0; f < (uint32_t)F && f * U < left; f++) {
                    const uint32_t in = msk[half][f][lane];
                    VT v[U];
#pragma unroll
                    for (int u = 0; u < U; u++) v[u] = val[half][f * U + u][lane];
#pragma unroll
                    for (int u = 0; u < U; u++)
                        if ((in >> u) & 1u) { acc = acc + (double)v[u]; n++; }      // (a plain conversion: denormals kept)
                }
            }
        }
        if (w == 0 && live) { a.sum[at] = acc; a.cnt[at] = n; }
    }
}

// The yardstick of tools/centred_probe.py, not a form of the composite: the same windows of the same stamps read with one lane per
// (stamp, cell), in no order and with nothing kept -- what the gathers alone cost when nothing depends on anything.
template <typename VT, bool WRAP>
__global__ __launch_bounds__(256) void k_centred_floor(const CentredArgs a, int64_t total, double *__restrict__ sink)
{
    const VT *__restrict__ x = (const VT *)a.x;
    const int W = 2 * a.hx + 1;
    const int64_t parts = (a.wcells + 255) / 256;                                   // workgroup b: part b % parts of stamp b / parts
    for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
        const int64_t r = b / parts;
        const int wc = (int)(b - r * parts) * 256 + (int)threadIdx.x;
        if (wc >= a.wcells) continue;
        const CtkStamp s = a.st[r];
        const int y = s.row + wc / W - a.hy;
        int c = s.col + wc % W - a.hx;
        bool ok = (unsigned)y < (unsigned)a.ny;
        if (WRAP) { c += c < 0 ? a.nx : 0; c -= c >= a.nx ? a.nx : 0; }
        else ok = ok && (unsigned)c < (unsigned)a.nx;
        if (ok) {
            const VT xv = x[s.base + (int64_t)y * a.nx + c];
            if (xv == (VT)-1.2345678e30f) sink[0] = (double)xv;                     // (as good as never: keeps the load)
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the arguments of one call, checked once
struct CentredCall {
    int64_t T = 0, R = 0;
    int ny = 0, nx = 0, nbins = 0, hy = 0, hx = 0, wrap = 0, skipna = 0;
    const int64_t *t = nullptr;
    const int32_t *row = nullptr, *col = nullptr, *bin = nullptr;
    int64_t wcells() const { return (2 * (int64_t)hy + 1) * (2 * (int64_t)hx + 1); }
    size_t cells() const { return (size_t)nbins * (size_t)wcells(); }
};

static int centred_check(const ctk_handle *h, const char *name, CentredCall &c, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row,
                         const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "%s: null handle", name);
    if (T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad shape (T=%lld ny=%d nx=%d)", name, (long long)T, ny, nx);
    if (nbins < 1) return ctk_set_error(CTK_E_INVALID, "%s: nbins=%d (at least 1)", name, nbins);
    if (hy < 0 || hx < 0) return ctk_set_error(CTK_E_INVALID, "%s: half widths hy=%d hx=%d (not negative)", name, hy, hx);
    if (R < 0 || R > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "%s: R=%lld stamps do not fit the uint32 counts (at most 2^32 - 1)", name, (long long)R);
    const int64_t H = 2 * (int64_t)hy + 1, W = 2 * (int64_t)hx + 1, lim = (int64_t)1 << 31;
    if (H >= lim || W >= lim || H * W >= lim || H * W * nbins >= lim)
        return ctk_set_error(CTK_E_INVALID, "%s: nbins * (2 hy + 1) * (2 hx + 1) = %d * %lld * %lld cells (below 2^31)", name, nbins, (long long)H, (long long)W);
    if (wrap && W > nx)
        return ctk_set_error(CTK_E_RANGE, "%s: a window of 2 * %d + 1 columns on a periodic grid of %d would count a column twice", name, hx, nx);
    if (R > 0 && (!t || !row || !col || !bin)) return ctk_set_error(CTK_E_INVALID, "%s: null stamp array", name);
    for (int64_t r = 0; r < R; r++) {
        if (t[r] < 0 || t[r] >= T) return ctk_set_error(CTK_E_INVALID, "%s: t[%lld] = %lld is not in [0, %lld)", name, (long long)r, (long long)t[r], (long long)T);
        if (r > 0 && t[r] < t[r - 1]) return ctk_set_error(CTK_E_INVALID, "%s: t[%lld] = %lld after %lld: the stamps must be in non-decreasing time order", name, (long long)r, (long long)t[r], (long long)t[r - 1]);
        if (row[r] < 0 || row[r] >= ny) return ctk_set_error(CTK_E_INVALID, "%s: row[%lld] = %d is not in [0, %d)", name, (long long)r, row[r], ny);
        if (col[r] < 0 || col[r] >= nx) return ctk_set_error(CTK_E_INVALID, "%s: col[%lld] = %d is not in [0, %d)", name, (long long)r, col[r], nx);
        if (bin[r] >= nbins) return ctk_set_error(CTK_E_INVALID, "%s: bin[%lld] = %d is not below nbins = %d (negative: dropped)", name, (long long)r, bin[r], nbins);
    }
    c.T = T; c.R = R; c.ny = ny; c.nx = nx; c.nbins = nbins; c.hy = hy; c.hx = hx; c.wrap = wrap != 0; c.skipna = skipna != 0;
    c.t = t; c.row = row; c.col = col; c.bin = bin;
    return CTK_OK;
}

// The stamps of the launches of one call in bin order (a stable counting sort per launch), and nbins + 1 offsets per launch.
struct CentredCsr {
    std::vector<CtkStamp> st;
    std::vector<uint32_t> off;
    std::vector<uint32_t> longest, kept;          // per launch: the stamps of its longest bin and of all its bins
    // stamps [r0, r1) for a launch on time steps from c0 of `rows` latitude rows from y0; returns where its offsets start in `off`
    size_t append(const CentredCall &c, int64_t r0, int64_t r1, int64_t c0, int64_t rows, int64_t y0)
    {
        const size_t o = off.size(), base = st.size();
        off.resize(o + (size_t)c.nbins + 1, 0);
        uint32_t *of = off.data() + o;
        for (int64_t r = r0; r < r1; r++) if (c.bin[r] >= 0) of[c.bin[r] + 1]++;
        of[0] = (uint32_t)base;
        for (int b = 0; b < c.nbins; b++) of[b + 1] += of[b];
        st.resize(base + (of[c.nbins] - of[0]));
        uint32_t most = 0;
        for (int b = 0; b < c.nbins; b++) most = std::max(most, of[b + 1] - of[b]);
        longest.push_back(most);
        kept.push_back(of[c.nbins] - of[0]);
        std::vector<uint32_t> next(of, of + c.nbins);
        for (int64_t r = r0; r < r1; r++) {
            if (c.bin[r] < 0) continue;
            CtkStamp &s = st[next[c.bin[r]]++];
            s.base = ((c.t[r] - c0) * rows - y0) * (int64_t)c.nx;
            s.row = c.row[r]; s.col = c.col[r];
        }
        return o;
    }
    size_t st_bytes() const { return (st.size() * sizeof(CtkStamp) + 15) & ~(size_t)15; }
    // to ce_idx on the handle's stream: the stamps, then the offsets
    int upload(ctk_handle *h)
    {
        CTKCHK(ensure(h, h->ce_idx, st_bytes() + off.size() * 4 + 16));
        if (!st.empty()) HIPCHK(hipMemcpyAsync(h->ce_idx.p, st.data(), st.size() * sizeof(CtkStamp), hipMemcpyHostToDevice, h->stream));
        if (!off.empty()) HIPCHK(hipMemcpyAsync((char *)h->ce_idx.p + st_bytes(), off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream));
        return CTK_OK;
    }
    const uint32_t *off_dev(const ctk_handle *h, size_t o) const { return (const uint32_t *)((const char *)h->ce_idx.p + st_bytes()) + o; }
};

// sum / n += k_centred over the stamps behind the offsets at off_dev, on the handle's stream
template <typename VT>
static int launch_centred_t(ctk_handle *h, const CentredCall &c, const VT *x_dev, const uint32_t *off_dev, uint32_t longest, uint32_t kept, double *sum_dev,
                            uint32_t *n_dev)
{
    const CtkCentredPlan pl = ctk_centred_plan((int)sizeof(VT), c.nbins, c.wcells(), longest, kept, h->ce_form_dbg, h->ce_unroll_dbg, h->ce_threads_dbg);
    h->ce_form = pl.form; h->ce_unroll = pl.unroll; h->ce_threads = pl.threads; h->ce_grid = pl.grid;
    CentredArgs a;
    a.x = x_dev; a.st = (const CtkStamp *)h->ce_idx.p; a.off = off_dev; a.sum = sum_dev; a.cnt = n_dev;
    a.blocks = pl.blocks; a.parts = pl.parts;
    a.ny = c.ny; a.nx = c.nx; a.hy = c.hy; a.hx = c.hx; a.wcells = (int32_t)c.wcells(); a.umax = pl.unroll;
#define CTK_CENTRED_LAUNCH(S, W)                                                                        \
    do {                                                                                                \
        if (pl.form) k_centred_fed<VT, S, W><<<pl.grid, 64 * CTK_CENTRED_FED_WAVES, 0, h->stream>>>(a); \
        else k_centred<VT, S, W><<<pl.grid, pl.threads, 0, h->stream>>>(a);                             \
    } while (0)
    if (c.skipna) { if (c.wrap) CTK_CENTRED_LAUNCH(true, true); else CTK_CENTRED_LAUNCH(true, false); }
    else          { if (c.wrap) CTK_CENTRED_LAUNCH(false, true); else CTK_CENTRED_LAUNCH(false, false); }
#undef CTK_CENTRED_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}
static int launch_centred(ctk_handle *h, const CentredCall &c, const void *x_dev, bool f64, const uint32_t *off_dev, uint32_t longest, uint32_t kept,
                          double *sum_dev, uint32_t *n_dev)
{
    return f64 ? launch_centred_t<double>(h, c, (const double *)x_dev, off_dev, longest, kept, sum_dev, n_dev)
               : launch_centred_t<float>(h, c, (const float *)x_dev, off_dev, longest, kept, sum_dev, n_dev);
}

static int centred_zero(ctk_handle *h, const CentredCall &c, double *sum_dev, uint32_t *n_dev)
{
    HIPCHK(hipMemsetAsync(sum_dev, 0, c.cells() * 8, h->stream));
    HIPCHK(hipMemsetAsync(n_dev, 0, c.cells() * 4, h->stream));
    return CTK_OK;
}

// the whole slab in HBM: one launch over all stamps
static int centred_slab(ctk_handle *h, const CentredCall &c, const void *x_dev, bool f64, double *sum_dev, uint32_t *n_dev, int accumulate)
{
    CentredCsr csr;
    const size_t o = csr.append(c, 0, c.R, 0, c.ny, 0);
    CTKCHK(csr.upload(h));
    int rc = accumulate ? CTK_OK : centred_zero(h, c, sum_dev, n_dev);
    if (rc == CTK_OK && !csr.st.empty()) rc = launch_centred(h, c, x_dev, f64, csr.off_dev(h, o), csr.longest[0], csr.kept[0], sum_dev, n_dev);
    const hipError_t e = hipStreamSynchronize(h->stream);                          // (the stamps have left csr when this returns)
    if (rc == CTK_OK && e != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    return rc;
}

static int centred_dev_impl(ctk_handle *h, const void *x_dev, bool f64, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row,
                            const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev,
                            int accumulate, const char *name)
{
    CentredCall c;
    if (h && !x_dev) CTKCHK(comp_resident(h, name, f64, T, ny, nx, &x_dev));          // (before the stamps are held against a shape that is not there)
    CTKCHK(centred_check(h, name, c, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna));
    if (!sum_dev || !n_dev) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    HIPCHK(hipSetDevice(h->device));
    return centred_slab(h, c, x_dev, f64, sum_dev, n_dev, accumulate);
}

extern "C" int ctk_centred_f32_dev(ctk_handle *h, const float *x_dev, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                                   const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate)
{
    return centred_dev_impl(h, x_dev, false, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna, sum_dev, n_dev, accumulate, "ctk_centred_f32_dev");
}
extern "C" int ctk_centred_f64_dev(ctk_handle *h, const double *x_dev, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                                   const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev, int accumulate)
{
    return centred_dev_impl(h, x_dev, true, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna, sum_dev, n_dev, accumulate, "ctk_centred_f64_dev");
}

// One chunk of the field that carries stamps: time steps [c0, c0 + nt), latitude rows [y0, y0 + rows), the stamps' offsets at `off`
struct CentredPiece { int64_t c0, nt, y0, rows; size_t off; uint32_t longest, kept; };

// host array or reader: the field passes through the two chunk buffers (io_in), chunk k+1 read and copied while k_centred reduces
// chunk k.  A chunk none of whose steps carries a stamp with bin >= 0 is skipped -- not read, not uploaded -- and of the others only
// the band of latitude rows that their windows touch travels, as one strided copy (a reader still fills whole planes of its pinned
// buffer: its contract is that of every other reader).  No source: the resident anomaly slab.  The accumulators stay in HBM until
// the last chunk.
static int centred_stream_impl(ctk_handle *h, StreamIO &io, bool f64, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row,
                               const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum, uint32_t *n,
                               int64_t chunk_steps, const char *name)
{
    CentredCall c;
    const bool resident = !io.host_in && !io.read;
    const void *res_dev = nullptr;
    if (h && resident) CTKCHK(comp_resident(h, name, f64, T, ny, nx, &res_dev));      // (before the stamps are held against a shape that is not there)
    CTKCHK(centred_check(h, name, c, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna));
    if (!sum || !n) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps=%lld", name, (long long)chunk_steps);
    HIPCHK(hipSetDevice(h->device));
    const size_t esz = f64 ? 8 : 4, row_bytes = (size_t)nx * esz, plane = (size_t)ny * row_bytes;
    CTKCHK(ensure(h, h->ce_sum, c.cells() * 8));
    CTKCHK(ensure(h, h->ce_n, c.cells() * 4));
    double *sdev = P<double>(h->ce_sum);
    uint32_t *ndev = P<uint32_t>(h->ce_n);
    const double t0 = now_ms();
    if (resident) {
        CTKCHK(centred_slab(h, c, res_dev, f64, sdev, ndev, 0));
    } else {
        io.esz = esz;
        io.chunk = ctk_stream_chunk(chunk_steps, T, plane);
        // the chunks that carry stamps, their bands and their stamps (t is non-decreasing: one walk)
        CentredCsr csr;
        std::vector<CentredPiece> pieces;
        int64_t max_rows = 0;
        for (int64_t r = 0; r < R;) {
            const int64_t k = t[r] / io.chunk, c0 = k * io.chunk, c1 = std::min<int64_t>(c0 + io.chunk, T);
            int64_t r1 = r, lo = ny, hi = -1;
            for (; r1 < R && t[r1] < c1; r1++)
                if (bin[r1] >= 0) { lo = std::min<int64_t>(lo, row[r1]); hi = std::max<int64_t>(hi, row[r1]); }
            if (hi >= 0) {
                CentredPiece p;
                p.c0 = c0; p.nt = c1 - c0;
                p.y0 = std::max<int64_t>(lo - hy, 0);
                p.rows = std::min<int64_t>(hi + hy, ny - 1) - p.y0 + 1;
                p.off = csr.append(c, r, r1, c0, p.rows, p.y0);
                p.longest = csr.longest.back(); p.kept = csr.kept.back();
                max_rows = std::max(max_rows, p.rows);
                pieces.push_back(p);
            }
            r = r1;
        }
        const size_t cbytes = (size_t)io.chunk * (size_t)(io.read ? ny : max_rows) * row_bytes;
        if (!pieces.empty()) CTKCHK(stream_setup(h, cbytes, 0, io.read != nullptr));
        int rc = csr.upload(h);
        if (rc == CTK_OK) rc = centred_zero(h, c, sdev, ndev);
        const double t_in = now_ms();
        io.passes_in++;
        for (size_t k = 0; k < pieces.size() && rc == CTK_OK; k++) {
            const CentredPiece &p = pieces[k];
            const int b = (int)(k & 1);
            char *dev = (char *)h->io_in.p + (size_t)b * cbytes;
            const size_t band = (size_t)p.rows * row_bytes;
            rc = [&]() -> int {
                if (k >= 2) HIPCHK(hipEventSynchronize(h->ev_thr[b]));              // the device buffer (and its pinned twin) is free again
                const char *src = (const char *)io.host_in + (size_t)p.c0 * plane;
                if (io.read) {
                    const double r0 = now_ms();
                    const int rr = io.read(io.read_user, p.c0, p.nt, h->pin_in[b]);
                    io.ms_read += now_ms() - r0;
                    if (rr) return ctk_set_error(CTK_E_INVALID, "%s: the reader returned %d for timesteps [%lld, %lld)", name, rr, (long long)p.c0, (long long)(p.c0 + p.nt));
                    src = (const char *)h->pin_in[b];
                }
                src += (size_t)p.y0 * row_bytes;
                if (p.rows == ny) HIPCHK(hipMemcpyAsync(dev, src, (size_t)p.nt * plane, hipMemcpyHostToDevice, h->copy_stream));
                else HIPCHK(hipMemcpy2DAsync(dev, band, src, plane, band, (size_t)p.nt, hipMemcpyHostToDevice, h->copy_stream));      // row s: the band of step c0 + s
                HIPCHK(hipEventRecord(h->ev_h2d[b], h->copy_stream));
                HIPCHK(hipStreamWaitEvent(h->stream, h->ev_h2d[b], 0));
                CTKCHK(launch_centred(h, c, dev, f64, csr.off_dev(h, p.off), p.longest, p.kept, sdev, ndev));      // (it clips at the grid's rows, not the band's)
                HIPCHK(hipEventRecord(h->ev_thr[b], h->stream));
                return CTK_OK;
            }();
        }
        io.ms_in += now_ms() - t_in;
        stream_ms_set(h, io);                                             // (no writer, no output side: those two stay 0)
        // (also after an error: a chunk may still be on its way into a buffer, and the stamps must have left csr)
        const hipError_t e1 = h->copy_stream ? hipStreamSynchronize(h->copy_stream) : hipSuccess;
        const hipError_t e2 = hipStreamSynchronize(h->stream);
        if (rc != CTK_OK) return rc;
        if (e1 != hipSuccess || e2 != hipSuccess) return ctk_set_error(CTK_E_NODEVICE, "%s: hipStreamSynchronize failed", name);
    }
    HIPCHK(hipMemcpy(sum, sdev, c.cells() * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n, ndev, c.cells() * 4, hipMemcpyDeviceToHost));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

extern "C" int ctk_centred_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                               const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum, uint32_t *n, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = x;
    return centred_stream_impl(h, io, false, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna, sum, n, chunk_steps, "ctk_centred_f32");
}
extern "C" int ctk_centred_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row, const int32_t *col,
                               const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum, uint32_t *n, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = x;
    return centred_stream_impl(h, io, true, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna, sum, n, chunk_steps, "ctk_centred_f64");
}
extern "C" int ctk_centred_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn field_reader, void *field_user, int64_t R, const int64_t *t,
                              const int32_t *row, const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum, uint32_t *n,
                              int64_t chunk_steps)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_centred_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    StreamIO io;
    io.read = field_reader; io.read_user = field_user;
    return centred_stream_impl(h, io, elem_bytes == 8, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna, sum, n, chunk_steps, "ctk_centred_cb");
}

// what ctk_centred_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_centred_plan(int elem_bytes, int nbins, int hy, int hx, int64_t max_bin, int64_t kept, int form, int unroll, int threads, int64_t *out6)
{
    int64_t *out5 = out6;
    const int64_t H = 2 * (int64_t)hy + 1, W = 2 * (int64_t)hx + 1, lim = (int64_t)1 << 31;
    if (!out5 || (elem_bytes != 4 && elem_bytes != 8) || nbins < 1 || hy < 0 || hx < 0 || H * W >= lim || H * W * nbins >= lim)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_centred_plan: bad arguments");
    if (max_bin < 0 || kept < max_bin) return ctk_set_error(CTK_E_INVALID, "ctk_debug_centred_plan: bad arguments");
    const CtkCentredPlan p = ctk_centred_plan(elem_bytes, nbins, H * W, max_bin, kept, form, unroll, threads);
    out5[0] = p.unroll; out5[1] = p.threads; out5[2] = p.parts; out5[3] = p.blocks; out5[4] = p.grid; out6[5] = p.form;
    return CTK_OK;
}

// test hook for the following centred launches on this handle: the form (0 plain, 1 fed), the widest batch of stamps and the cells per
// workgroup of the plain form (-1: the rule)
extern "C" int ctk_debug_set_centred(ctk_handle *h, int form, int unroll, int threads)
{
    if (!h || form < -1 || form > 1 || unroll < -1 || unroll == 0 || threads < -1 || threads == 0)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_centred: null handle, form not -1 / 0 / 1, or unroll / threads not -1 / positive");
    h->ce_form_dbg = form; h->ce_unroll_dbg = unroll; h->ce_threads_dbg = threads;
    return CTK_OK;
}

// out4 = { the batch of the last centred launch on this handle (0: none yet), its cells per workgroup, its workgroups, its form }
extern "C" int ctk_debug_centred_launch(ctk_handle *h, int64_t *out4)
{
    if (!h || !out4) return ctk_set_error(CTK_E_INVALID, "ctk_debug_centred_launch: null argument");
    out4[0] = h->ce_unroll; out4[1] = h->ce_threads; out4[2] = h->ce_grid; out4[3] = h->ce_form;
    return CTK_OK;
}

// k_centred alone between HIP events on the handle's stream (tools/centred_probe.py): one launch that starts from zeroed accumulators,
// then `reps` timed launches that continue from them; ms2 = {best, mean} per launch.  floor != 0: k_centred_floor instead, the plain
// unordered gather of the same windows (sum_dev is its sink, nothing is summed)
extern "C" int ctk_debug_time_centred(ctk_handle *h, const void *x_dev, int is_f64, int64_t T, int ny, int nx, int64_t R, const int64_t *t, const int32_t *row,
                                      const int32_t *col, const int32_t *bin, int nbins, int hy, int hx, int wrap, int skipna, double *sum_dev, uint32_t *n_dev,
                                      int floor, int reps, double *ms2)
{
    CentredCall c;
    CTKCHK(centred_check(h, "ctk_debug_time_centred", c, T, ny, nx, R, t, row, col, bin, nbins, hy, hx, wrap, skipna));
    if (!x_dev || !sum_dev || !n_dev || !ms2 || reps < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_centred: null buffer or reps < 1");
    if ((int64_t)(reps + 1) * R > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_centred: (reps + 1) * R counts overflow uint32");
    HIPCHK(hipSetDevice(h->device));
    const bool f64 = is_f64 != 0;
    CentredCsr csr;
    const size_t o = csr.append(c, 0, R, 0, ny, 0);
    if (csr.st.empty()) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_centred: no stamp with bin >= 0");
    CTKCHK(csr.upload(h));
    CTKCHK(centred_zero(h, c, sum_dev, n_dev));
    auto launch = [&]() -> int {
        if (!floor) return launch_centred(h, c, x_dev, f64, csr.off_dev(h, o), csr.longest[0], csr.kept[0], sum_dev, n_dev);
        CentredArgs a = {};
        a.x = x_dev; a.st = (const CtkStamp *)h->ce_idx.p;
        a.ny = ny; a.nx = nx; a.hy = hy; a.hx = hx; a.wcells = (int32_t)c.wcells();
        const int64_t total = (int64_t)csr.st.size() * ((a.wcells + 255) / 256);
        const unsigned grid = (unsigned)std::min<int64_t>(total, (int64_t)h->n_cus * 32);
        if (f64) { if (c.wrap) k_centred_floor<double, true><<<grid, 256, 0, h->stream>>>(a, total, sum_dev); else k_centred_floor<double, false><<<grid, 256, 0, h->stream>>>(a, total, sum_dev); }
        else     { if (c.wrap) k_centred_floor<float, true><<<grid, 256, 0, h->stream>>>(a, total, sum_dev); else k_centred_floor<float, false><<<grid, 256, 0, h->stream>>>(a, total, sum_dev); }
        HIPCHK(hipGetLastError());
        return CTK_OK;
    };
    return time_launches(h, "ctk_debug_time_centred", reps, ms2, launch);
}
