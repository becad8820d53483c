// ctk_lwa.hip -- the third family of blocking indices on the device (included by ctk_api.hip): finite-amplitude local wave activity of
// a height field (Huang & Nakamura 2016; Chen, Lu, Burrows & Leung 2015 for Z500, with the anticyclonic / cyclonic split; Martineau et
// al. 2017; Nakamura & Huang 2018).  include/contrack_hip.h states the contract, tests/lwa_util.py is its numpy statement.  Per step
// and DOMAIN D = (d_0 .. d_{n-1}) -- the rows of one hemisphere from the equator side to the pole -- and per ACTIVE row j = d_p:
//     cap_j = nx * sum_{p' >= p} W[d_p']                      the area poleward of row j, an exact uint64 (W: uint32 row weights)
//     Z_j   = the value of the smallest key k (an_key, ctk_select.h) with  A(k) = sum of W over the domain's non-NaN pixels of key <= k  >= cap_j
//     a = sum_{p' >= p, z > Z_j} (z - Z_j) q[d_p']            y = sum_{p' < p, z < Z_j} (Z_j - z) q[d_p']          float64, in domain order
//     out[j][c] = (dtype)((a + y) S[j])    (part 1: a alone, part 2: y alone);  Z_j = NaN (the NaNs ate the area): the row is NaN
//
// k_lwa_contour: a workgroup per (step, domain) finds Z_j of ALL active rows at once by bisection on the key space.  Every row
// starts from the interval [smallest key, largest key] of the domain's pixels and halves it once per round, so all intervals are
// nodes of one binary tree: equal or disjoint.  The caps fall towards the pole, the contours with them, so the pivots of a round
// are monotone over the active rows: a pixel finds by binary search in LDS how many pivots its key does not exceed and adds its
// weight to ONE of n_act + 1 uint64 buckets; suffix sums of the buckets are A(pivot) of every row.  As many rounds as the
// difference of the two keys has bits -- at most 32 for float32, 64 for float64 --; integer weights
// make the sums independent of the order of the atomics.  The plane is read from L2 once per round.
// k_lwa_integral: a workgroup per (step, domain, strip of columns) holds the strip's domain rows in LDS; a thread per (active row,
// column) walks the domain in order -- one loop, the row weight q a wave-uniform load, the side of the contour a select.
// Both write active rows only: the launch zeroes `out` and `ref` before them.
#pragma once

// the row table of a call on the device.  Per domain position i (npos of them, the domains one after the other): rows[i], W and q of
// that row; per active entry e (in domain order): its position in its domain, its cap and its S
struct LwaTab {
    const uint64_t *cap;
    const double *S, *q;
    const uint32_t *W;
    const int32_t *rows, *act_pos, *dom_off, *act_off;      // dom_off, act_off: ndom + 1 each
    int ndom;
};

template <typename VT> struct LwaKey;
template <> struct LwaKey<float> { typedef uint32_t type; static constexpr int BITS = 32; };
template <> struct LwaKey<double> { typedef uint64_t type; static constexpr int BITS = 64; };

// z: (steps, ny, nx); ref: (steps, ny), zeroed by the launch; pairs = steps * ndom.  Dynamic LDS: four words of `slots` (the longest
// domain + 1: every row may be active) and one word per wave (ctk_lwa_plan's lds_sel).
template <typename VT>
__global__ __launch_bounds__(CTK_LWA_SEL_THREADS) CTK_SGPR_8WAVES void k_lwa_contour(const VT *__restrict__ z, int ny, int nx, int64_t pairs, LwaTab tab, int slots,
                                                                                  VT *__restrict__ ref, int xcd)
{
    typedef typename LwaKey<VT>::type KT;
    constexpr int NT = CTK_LWA_SEL_THREADS;
    extern __shared__ __attribute__((aligned(16))) char lwa_lds[];
    uint64_t *bucket = (uint64_t *)lwa_lds, *lo = bucket + slots, *hi = lo + slots, *mid = hi + slots, *part = mid + slots;       // (keys kept in 64 bits; part: one per wave)
    const int tid = (int)threadIdx.x;
    const int64_t npix = (int64_t)ny * nx;
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b < pairs; b += gridDim.x) {
        const int64_t s = b / tab.ndom;
        const int d = (int)(b - s * tab.ndom);
        const int p0 = tab.dom_off[d], n = tab.dom_off[d + 1] - p0, e0 = tab.act_off[d], na = tab.act_off[d + 1] - e0;
        if (na == 0) continue;                                                    // (the whole workgroup)
        const int32_t *rows = tab.rows + p0;
        const uint32_t *W = tab.W + p0;
        const VT *zs = z + s * npix;
        const int per = (na + NT) / NT;                                           // buckets per thread of the suffix sums: per * NT >= na + 1
        const int probes = 32 - __builtin_clz((unsigned)na);                      // halvings that bring [0, na] down to one place
        const uint32_t cells = (uint32_t)n * (uint32_t)nx;                        // (a plane has fewer than 2^31 pixels)
        // the smallest and the largest key of the pixels that count, and their area: every contour lies between the two, so the
        // bisection starts there and needs as many rounds as their difference has bits
        uint64_t kmin = ~(uint64_t)0, kmax = 0, total = 0;
        for (uint32_t i = (uint32_t)tid; i < cells; i += NT) {
            const uint32_t p = i / (uint32_t)nx, c = i - p * (uint32_t)nx;
            const uint32_t w = W[p];
            const VT v = zs[(int64_t)rows[p] * nx + c];
            if (!w || an_isnan(v)) continue;
            const uint64_t k = (uint64_t)an_key(v);
            kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; total += w;
        }
        if (tid == 0) { part[0] = ~(uint64_t)0; part[1] = 0; part[2] = 0; }
        __syncthreads();
        if (total) {
            atomicMin((unsigned long long *)&part[0], (unsigned long long)kmin);
            atomicMax((unsigned long long *)&part[1], (unsigned long long)kmax);
            atomicAdd((unsigned long long *)&part[2], (unsigned long long)total);
        }
        __syncthreads();
        kmin = part[0]; kmax = part[1]; total = part[2];
        const int rounds = total && kmax > kmin ? 64 - __builtin_clzll(kmax - kmin) : 0;
        for (int a = tid; a < na; a += NT) { lo[a] = kmin; hi[a] = kmax; }
        __syncthreads();
        for (int r = 0; r < rounds; r++) {
            for (int a = tid; a <= na; a += NT) {
                bucket[a] = 0;
                if (a < na) mid[a] = lo[a] + ((hi[a] - lo[a]) >> 1);
            }
            __syncthreads();
            // four pixels per lane and trip, searched side by side: the LDS reads of one hide behind those of the others
            for (uint32_t i0 = (uint32_t)tid; i0 < cells; i0 += 4 * NT) {
                uint64_t k[4];
                uint32_t w[4];
                int l[4], h[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint32_t i = i0 + (uint32_t)u * NT;
                    w[u] = 0; k[u] = 0; l[u] = 0; h[u] = na;
                    if (i < cells) {
                        const uint32_t p = i / (uint32_t)nx, c = i - p * (uint32_t)nx;
                        const VT v = zs[(int64_t)rows[p] * nx + c];
                        if (!an_isnan(v)) { w[u] = W[p]; k[u] = (uint64_t)an_key(v); }
                    }
                }
                for (int t = 0; t < probes; t++) {                               // l[u]: how many pivots are >= k[u] (they fall with a)
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        if (l[u] < h[u]) {
                            const int m = (l[u] + h[u]) >> 1;
                            if (mid[m] >= k[u]) l[u] = m + 1; else h[u] = m;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (w[u]) atomicAdd((unsigned long long *)&bucket[l[u]], (unsigned long long)w[u]);
            }
            __syncthreads();
            // A(mid[a]) = the buckets behind a.  Thread t owns buckets [t * per, t * per + per); a suffix scan over the threads -- down
            // the lanes of a wave, then over the 16 wave totals -- gives each what lies behind its own
            const int b0 = tid * per, b1 = min(b0 + per, na + 1);
            uint64_t own = 0;
            for (int a = b0; a < b1; a++) own += bucket[a];
            uint64_t suffix = own;                                                // of this lane and the lanes behind it in its wave
            const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
            for (int dl = 1; dl < 64; dl <<= 1) {
                const uint64_t o = (uint64_t)__shfl_down((unsigned long long)suffix, dl, 64);
                if (lane + dl < 64) suffix += o;
            }
            if (lane == 0) part[wave] = suffix;
            __syncthreads();
            if (b0 <= na) {
                uint64_t behind = suffix - own;
                for (int w2 = wave + 1; w2 < NT / 64; w2++) behind += part[w2];
                for (int a = b1 - 1; a >= b0; a--) {
                    if (a < na) {
                        // (a row out of reach -- the NaNs ate its area -- goes up every round; its interval of b bits is down to one
                        // key after b - 1 or b rounds, and the clamp keeps lo <= hi whatever the number of rounds: a pivot never wraps)
                        if (behind >= tab.cap[e0 + a]) hi[a] = mid[a];
                        else lo[a] = mid[a] < hi[a] ? mid[a] + 1 : hi[a];
                    }
                    behind += bucket[a];
                }
            }
            __syncthreads();
        }
        for (int a = tid; a < na; a += NT) {
            const int j = rows[tab.act_pos[e0 + a]];
            ref[s * ny + j] = total >= tab.cap[e0 + a] ? an_unkey((KT)lo[a]) : (VT)__builtin_nan("");
        }
        __syncthreads();
    }
}

// z, out: (steps, ny, nx); ref: (steps, ny), what k_lwa_contour left; workgroup b of `blocks` = steps * ndom * nstrips takes strip
// b % nstrips of domain (b / nstrips) % ndom of step b / (nstrips * ndom).  Dynamic LDS: rows of the longest domain x strip pixels.
template <typename VT, bool VEC>
__global__ __launch_bounds__(CTK_LWA_THREADS) CTK_SGPR_8WAVES void k_lwa_integral(const VT *__restrict__ z, int ny, int nx, int strip, int nstrips, int64_t blocks, LwaTab tab,
                                                                                   const VT *__restrict__ ref, int which, VT *__restrict__ out, int xcd)
{
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char lwa_lds[];
    VT *zl = (VT *)lwa_lds;                                                       // [n][strip]
    ctk_const_f64 *qt = (ctk_const_f64 *)tab.q;
    const int tid = (int)threadIdx.x;
    const int64_t npix = (int64_t)ny * nx;
    const int64_t per_step = (int64_t)tab.ndom * nstrips;
    constexpr int N16 = 16 / (int)sizeof(VT);
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b < blocks; b += gridDim.x) {
        const int64_t s = b / per_step;
        const int rest = (int)(b - s * per_step), d = rest / nstrips, c0 = (rest - d * nstrips) * strip;
        const int wc = min(strip, nx - c0);
        const int p0 = tab.dom_off[d], n = tab.dom_off[d + 1] - p0, e0 = tab.act_off[d], na = tab.act_off[d + 1] - e0;
        if (na == 0) continue;                                                    // (the whole workgroup)
        const int32_t *rows = tab.rows + p0;
        const VT *zs = z + s * npix + c0;                                         // column c0 of row 0 of this step (64-bit throughout)
        if (VEC) {                                                                // nx, strip, c0 and wc are multiples of 4: 16-byte pieces
            const int u = wc / N16;
            for (int i = tid; i < n * u; i += CTK_LWA_THREADS) {
                const int p = i / u, k = (i - p * u) * N16;
                *(i32x4 *)(zl + p * strip + k) = *(const i32x4 *)(zs + (int64_t)rows[p] * nx + k);
            }
        } else {
            for (int i = tid; i < n * wc; i += CTK_LWA_THREADS) {
                const int p = i / wc, c = i - p * wc;
                zl[p * strip + c] = zs[(int64_t)rows[p] * nx + c];
            }
        }
        __syncthreads();
        for (int i = tid; i < na * wc; i += CTK_LWA_THREADS) {
            const int a = i / wc, c = i - a * wc;
            const int p = tab.act_pos[e0 + a], j = rows[p];
            const VT Z = ref[s * ny + j];
            const double Zd = (double)Z;
            double up = 0.0, dn = 0.0;
            for (int pp = 0; pp < n; pp++) {                                      // (pp, and with it q, is wave-uniform; `pole` is per lane)
                const VT v = zl[pp * strip + c];
                const double q = qt[p0 + pp], vd = (double)v;
                const bool pole = pp >= p;
                const double t = (pole ? vd - Zd : Zd - vd) * q;
                if (pole ? v > Z : v < Z) {                                        // (a NaN pixel fails both)
                    if (pole) up = up + t; else dn = dn + t;
                }
            }
            const double r = (which == 0 ? up + dn : which == 1 ? up : dn) * tab.S[e0 + a];
            out[s * npix + (int64_t)j * nx + c0 + c] = an_isnan(Z) ? (VT)__builtin_nan("") : (VT)r;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the row table of a call as the caller gave it (host pointers)
struct LwaArgs {
    int ndom;
    const int32_t *dom_off, *dom_rows;
    const uint8_t *active;
    const uint32_t *W;
    const double *q, *S;
    int part;
};
// ... checked and laid out for the device (lwa_check)
struct LwaHost {
    std::vector<uint64_t> cap;
    std::vector<double> S, q;
    std::vector<uint32_t> W;
    std::vector<int32_t> rows, act_pos, dom_off, act_off;
    int max_rows = 0;              // the longest domain
    int r0 = 0, r1 = 0;            // rows [r0, r1) span the domains: what a host-array call uploads of every plane
    int a0 = 0, a1 = 0;            // rows [a0, a1) span the active rows: what it downloads
};

static int lwa_check(const char *who, const void *h, int64_t steps, int ny, int nx, const LwaArgs &a, LwaHost &t)
{
    if (!h || !a.dom_off || !a.dom_rows || !a.active || !a.W || !a.q || !a.S || ny < 1 || nx < 1)
        return ctk_set_error(CTK_E_INVALID, "%s: bad arguments (null pointer or a size below 1)", who);
    if (steps < 1) return ctk_set_error(CTK_E_INVALID, "%s: steps = %lld", who, (long long)steps);
    if (a.ndom != 1 && a.ndom != 2) return ctk_set_error(CTK_E_INVALID, "%s: ndom = %d (one or two domains)", who, a.ndom);
    if (a.part < 0 || a.part > 2) return ctk_set_error(CTK_E_INVALID, "%s: part = %d (0 total, 1 anticyclonic, 2 cyclonic)", who, a.part);
    if ((int64_t)ny * nx > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: a plane of %lld pixels (at most 2^31 - 1)", who, (long long)ny * nx);
    if (a.dom_off[0] != 0) return ctk_set_error(CTK_E_INVALID, "%s: dom_off[0] = %d (must be 0)", who, a.dom_off[0]);
    for (int d = 0; d < a.ndom; d++) {
        const int64_t len = (int64_t)a.dom_off[d + 1] - a.dom_off[d];
        if (len < 1 || len > ny) return ctk_set_error(CTK_E_INVALID, "%s: domain %d has %lld rows (1 .. ny = %d)", who, d, (long long)len, ny);
    }
    t = LwaHost();
    std::vector<int> owner((size_t)ny, -1);                                     // the domain an active row was found in
    t.r0 = ny; t.a0 = ny;
    t.dom_off.assign(a.dom_off, a.dom_off + a.ndom + 1);
    t.act_off.assign(1, 0);
    for (int d = 0; d < a.ndom; d++) {
        const int p0 = a.dom_off[d], n = a.dom_off[d + 1] - p0;
        t.max_rows = std::max(t.max_rows, n);
        std::vector<char> seen((size_t)ny, 0);
        unsigned __int128 area = 0;
        for (int p = 0; p < n; p++) {
            const int64_t j = a.dom_rows[p0 + p];
            if (j < 0 || j >= ny) return ctk_set_error(CTK_E_INVALID, "%s: domain %d names row %lld outside [0, %d)", who, d, (long long)j, ny);
            if (seen[(size_t)j]) return ctk_set_error(CTK_E_INVALID, "%s: domain %d names row %lld twice", who, d, (long long)j);
            seen[(size_t)j] = 1;
            if (!std::isfinite(a.q[j]) || a.q[j] < 0.0) return ctk_set_error(CTK_E_INVALID, "%s: q[%lld] = %g (must be finite and >= 0)", who, (long long)j, a.q[j]);
            area += a.W[j];
            t.rows.push_back((int32_t)j); t.W.push_back(a.W[j]); t.q.push_back(a.q[j]);
            t.r0 = std::min(t.r0, (int)j); t.r1 = std::max(t.r1, (int)j + 1);
        }
        area *= (unsigned)nx;
        // (defensive: uint32 weights on a plane of fewer than 2^31 pixels stay below 2^63 -- the caps are uint64 whatever W becomes)
        if (area >> 63) return ctk_set_error(CTK_E_INVALID, "%s: nx x the weights of domain %d reach 2^63", who, d);
        uint64_t behind = (uint64_t)area;                                         // nx * the weights of rows p' >= p
        for (int p = 0; p < n; p++) {
            const int j = a.dom_rows[p0 + p];
            if (a.active[j]) {
                if (owner[(size_t)j] >= 0) return ctk_set_error(CTK_E_INVALID, "%s: the active row %d lies in two domains", who, j);
                owner[(size_t)j] = d;
                if (!(a.S[j] > 0.0) || !std::isfinite(a.S[j])) return ctk_set_error(CTK_E_INVALID, "%s: S[%d] = %g (must be finite and > 0 on an active row)", who, j, a.S[j]);
                if (behind == 0) return ctk_set_error(CTK_E_INVALID, "%s: the active row %d has no area poleward of it (cap = 0)", who, j);
                t.act_pos.push_back(p); t.cap.push_back(behind); t.S.push_back(a.S[j]);
                t.a0 = std::min(t.a0, j); t.a1 = std::max(t.a1, j + 1);
            }
            behind -= (uint64_t)a.W[j] * (uint64_t)nx;
        }
        t.act_off.push_back((int32_t)t.act_pos.size());
    }
    for (int j = 0; j < ny; j++)
        if (a.active[j] && owner[(size_t)j] < 0) return ctk_set_error(CTK_E_INVALID, "%s: the active row %d lies in no domain", who, j);
    if (t.a1 == 0) t.a0 = 0;
    return CTK_OK;
}

// the plan of a launch over `steps` steps, or CTK_E_INVALID at the capacity edge
static int lwa_plan_of(ctk_handle *h, const char *who, int esz, const LwaHost &t, int nx, int64_t steps, bool aligned, CtkLwaPlan &pl)
{
    pl = ctk_lwa_plan(esz, t.max_rows, nx, (int64_t)t.dom_off.size() - 1, steps, aligned, h->lw_knobs.cap());
    if (!pl.ok)
        return ctk_set_error(CTK_E_INVALID, "%s: a domain of %d rows does not fit in LDS (%d bytes: %d-byte pixels in strips of %d, 32 bytes per row for the contours)", who,
                             t.max_rows, CTK_LWA_LDS_MAX, esz, pl.vec ? 4 : 1);
    return CTK_OK;
}

// the device table of a call
static int lwa_table(ctk_handle *h, const LwaHost &t, LwaTab &tab)
{
    const size_t npos = t.rows.size(), nact = t.act_pos.size(), nd1 = t.dom_off.size();
    const size_t o_cap = 0, o_S = o_cap + nact * 8, o_q = o_S + nact * 8, o_W = o_q + npos * 8, o_rows = o_W + npos * 4, o_pos = o_rows + npos * 4,
                 o_doff = o_pos + nact * 4, o_aoff = o_doff + nd1 * 4, bytes = o_aoff + nd1 * 4;
    std::vector<char> img(bytes);
    if (nact) { memcpy(&img[o_cap], t.cap.data(), nact * 8); memcpy(&img[o_S], t.S.data(), nact * 8); memcpy(&img[o_pos], t.act_pos.data(), nact * 4); }
    memcpy(&img[o_q], t.q.data(), npos * 8); memcpy(&img[o_W], t.W.data(), npos * 4); memcpy(&img[o_rows], t.rows.data(), npos * 4);
    memcpy(&img[o_doff], t.dom_off.data(), nd1 * 4); memcpy(&img[o_aoff], t.act_off.data(), nd1 * 4);
    CTKCHK(ensure(h, h->lw_tab, bytes));
    HIPCHK(hipStreamSynchronize(h->stream));                                  // (a launch still reading the table of the call before)
    HIPCHK(hipMemcpy(h->lw_tab.p, img.data(), bytes, hipMemcpyHostToDevice));
    const char *base = (const char *)h->lw_tab.p;
    tab.cap = (const uint64_t *)(base + o_cap); tab.S = (const double *)(base + o_S); tab.q = (const double *)(base + o_q);
    tab.W = (const uint32_t *)(base + o_W); tab.rows = (const int32_t *)(base + o_rows); tab.act_pos = (const int32_t *)(base + o_pos);
    tab.dom_off = (const int32_t *)(base + o_doff); tab.act_off = (const int32_t *)(base + o_aoff);
    tab.ndom = (int)nd1 - 1;
    return CTK_OK;
}

// stage 1 / stage 2 of `steps` steps of z (steps, ny, nx) on the handle's stream; ref: (steps, ny) in device memory
template <typename VT>
static int launch_lwa_contour(ctk_handle *h, const VT *z, int ny, int nx, int64_t steps, const LwaTab &tab, const LwaHost &t, const CtkLwaPlan &pl, VT *ref)
{
    HIPCHK(hipMemsetAsync(ref, 0, (size_t)steps * ny * sizeof(VT), h->stream));
    if (t.act_pos.empty()) return CTK_OK;
    const int xcd = h->lw_knobs.xcd(pl.sel_xcd);
    k_lwa_contour<VT><<<pl.sel_grid, CTK_LWA_SEL_THREADS, (size_t)pl.lds_sel, h->stream>>>(z, ny, nx, pl.sel_blocks, tab, t.max_rows + 1, ref, xcd);
    HIPCHK(hipGetLastError());
    return CTK_OK;
}
template <typename VT>
static int launch_lwa_integral(ctk_handle *h, const VT *z, int ny, int nx, int64_t steps, const LwaTab &tab, const LwaHost &t, const CtkLwaPlan &pl, const VT *ref, int part,
                               VT *out)
{
    HIPCHK(hipMemsetAsync(out, 0, (size_t)steps * ny * nx * sizeof(VT), h->stream));
    h->lw_knobs.launched(pl.vec, pl.grid);
    if (t.act_pos.empty()) return CTK_OK;
    const int xcd = h->lw_knobs.xcd(pl.xcd);
    if (pl.vec) k_lwa_integral<VT, true><<<pl.grid, CTK_LWA_THREADS, (size_t)pl.lds, h->stream>>>(z, ny, nx, pl.strip, (int)pl.nstrips, pl.blocks, tab, ref, part, out, xcd);
    else k_lwa_integral<VT, false><<<pl.grid, CTK_LWA_THREADS, (size_t)pl.lds, h->stream>>>(z, ny, nx, pl.strip, (int)pl.nstrips, pl.blocks, tab, ref, part, out, xcd);
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

template <typename VT>
static int lwa_dev_impl(ctk_handle *h, const VT *x_dev, int64_t steps, int ny, int nx, const LwaArgs &a, VT *out_dev, VT *ref, const char *who)
{
    LwaHost t;
    CTKCHK(lwa_check(who, h, steps, ny, nx, a, t));
    if (!x_dev || !out_dev) return ctk_set_error(CTK_E_INVALID, "%s: null input or output", who);
    HIPCHK(hipSetDevice(h->device));
    CtkLwaPlan pl;
    CTKCHK(lwa_plan_of(h, who, (int)sizeof(VT), t, nx, steps, (((uintptr_t)x_dev | (uintptr_t)out_dev) & 15) == 0, pl));
    LwaTab tab;
    CTKCHK(lwa_table(h, t, tab));
    CTKCHK(ensure(h, h->lw_ref, (size_t)steps * ny * sizeof(VT)));
    CTKCHK(launch_lwa_contour<VT>(h, x_dev, ny, nx, steps, tab, t, pl, (VT *)h->lw_ref.p));
    CTKCHK(launch_lwa_integral<VT>(h, x_dev, ny, nx, steps, tab, t, pl, (const VT *)h->lw_ref.p, a.part, out_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (ref) HIPCHK(hipMemcpy(ref, h->lw_ref.p, (size_t)steps * ny * sizeof(VT), hipMemcpyDeviceToHost));
    return CTK_OK;
}

extern "C" int ctk_lwa_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows,
                               const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part, float *out_dev, float *ref)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    return lwa_dev_impl<float>(h, x_dev, steps, ny, nx, a, out_dev, ref, "ctk_lwa_f32_dev");
}
extern "C" int ctk_lwa_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows,
                               const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part, double *out_dev, double *ref)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    return lwa_dev_impl<double>(h, x_dev, steps, ny, nx, a, out_dev, ref, "ctk_lwa_f64_dev");
}

template <typename VT>
static int lwa_stream_impl(ctk_handle *h, StreamIO &io, int64_t steps, int ny, int nx, const LwaArgs &a, VT *ref, int64_t chunk_steps, int keep_resident, const char *name)
{
    LwaHost t;
    CTKCHK(lwa_check(name, h, steps, ny, nx, a, t));
    CTKCHK(row_band_begin(h, io, steps, (size_t)ny * nx * sizeof(VT), sizeof(VT), chunk_steps, keep_resident, name));
    CtkLwaPlan pl0;
    CTKCHK(lwa_plan_of(h, name, (int)sizeof(VT), t, nx, io.chunk, true, pl0));     // (the capacity edge, before anything is touched)
    LwaTab tab;
    CTKCHK(row_band_produce(
        h, io, steps, ny, nx, {t.r0, t.r1, t.a0, t.a1}, keep_resident, name,
        [&]() -> int {
            CTKCHK(lwa_table(h, t, tab));
            return ensure(h, h->lw_ref, (size_t)steps * ny * sizeof(VT));       // the contours of the whole call: they leave at its end
        },
        [&](const ProduceIn &c, char *out) -> int {
            CtkLwaPlan pl;
            CTKCHK(lwa_plan_of(h, name, (int)sizeof(VT), t, nx, c.nt, (((uintptr_t)c.dev | (uintptr_t)out) & 15) == 0, pl));
            VT *zr = (VT *)h->lw_ref.p + c.c0 * ny;
            CTKCHK(launch_lwa_contour<VT>(h, (const VT *)c.dev, ny, nx, c.nt, tab, t, pl, zr));
            return launch_lwa_integral<VT>(h, (const VT *)c.dev, ny, nx, c.nt, tab, t, pl, zr, a.part, (VT *)out);
        }));
    if (ref) HIPCHK(hipMemcpy(ref, h->lw_ref.p, (size_t)steps * ny * sizeof(VT), hipMemcpyDeviceToHost));
    return CTK_OK;
}

extern "C" int ctk_lwa_f32(ctk_handle *h, const float *x, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                           const uint32_t *W, const double *q, const double *S, int part, float *out, float *ref, int64_t chunk_steps, int keep_resident)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return lwa_stream_impl<float>(h, io, steps, ny, nx, a, ref, chunk_steps, keep_resident, "ctk_lwa_f32");
}
extern "C" int ctk_lwa_f64(ctk_handle *h, const double *x, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows, const uint8_t *active,
                           const uint32_t *W, const double *q, const double *S, int part, double *out, double *ref, int64_t chunk_steps, int keep_resident)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return lwa_stream_impl<double>(h, io, steps, ny, nx, a, ref, chunk_steps, keep_resident, "ctk_lwa_f64");
}
extern "C" int ctk_lwa_stream_cb(ctk_handle *h, int elem_bytes, int64_t steps, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, int ndom, const int32_t *dom_off,
                                 const int32_t *dom_rows, const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part, ctk_write_values_fn writer,
                                 void *writer_user, void *ref, int64_t chunk_steps, int keep_resident)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    StreamIO io;
    CTKCHK(stream_cb_io("ctk_lwa_stream_cb", h, elem_bytes, reader, reader_user, writer, writer_user, io));
    if (elem_bytes == 8) return lwa_stream_impl<double>(h, io, steps, ny, nx, a, (double *)ref, chunk_steps, keep_resident, "ctk_lwa_stream_cb");
    return lwa_stream_impl<float>(h, io, steps, ny, nx, a, (float *)ref, chunk_steps, keep_resident, "ctk_lwa_stream_cb");
}

// what ctk_lwa_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_lwa_plan(int elem_bytes, int64_t rows, int64_t nx, int64_t ndom, int64_t steps, int aligned, int64_t *out12)
{
    if (!out12 || (elem_bytes != 4 && elem_bytes != 8) || rows < 1 || nx < 1 || steps < 1 || (ndom != 1 && ndom != 2) || rows * nx > 0x7fffffffll)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_lwa_plan: bad arguments");
    const CtkLwaPlan p = ctk_lwa_plan(elem_bytes, rows, nx, ndom, steps, aligned != 0);
    out12[0] = p.ok; out12[1] = p.vec; out12[2] = p.strip; out12[3] = p.nstrips; out12[4] = p.lds; out12[5] = p.lds_sel; out12[6] = p.blocks; out12[7] = p.grid; out12[8] = p.xcd;
    out12[9] = p.sel_blocks; out12[10] = p.sel_grid; out12[11] = p.sel_xcd;
    return CTK_OK;
}

// test hook: out2 = { the form of the last k_lwa_integral launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups }
extern "C" int ctk_debug_lwa_form(ctk_handle *h, int64_t *out2)
{
    return knobs_form(h, &ctk_handle::lw_knobs, out2);
}

// test hook / experiments (tools/lwa_probe.py) for the following launches of both kernels on this handle: as ctk_debug_set_reversal
extern "C" int ctk_debug_set_lwa(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    return knobs_set("ctk_debug_set_lwa", h, &ctk_handle::lw_knobs, xcd_mode, grid_max);
}

// measurement (tools/lwa_probe.py): one stage alone between HIP events on slabs in device memory -- one launch that is not counted,
// then `reps` timed ones; ms2 = {best, mean}.  stage 1: the contours (k_lwa_contour and the memset before it), stage 2: the integrals
// on the contours of a stage-1 run made first (k_lwa_integral and its memset), stage 0: the plain copy kernel over the same two
// buffers (the table arguments may be NULL).
extern "C" int ctk_debug_time_lwa(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int ny, int nx, int ndom, const int32_t *dom_off, const int32_t *dom_rows,
                                  const uint8_t *active, const uint32_t *W, const double *q, const double *S, int part, void *out_dev, int stage, int reps, double *ms2)
{
    const LwaArgs a = {ndom, dom_off, dom_rows, active, W, q, S, part};
    if (!h || !x_dev || !out_dev || !ms2 || reps < 1 || steps < 1 || ny < 1 || nx < 1 || stage < 0 || stage > 2) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_lwa: bad arguments");
    if ((((uintptr_t)x_dev | (uintptr_t)out_dev) & 15) != 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_lwa: 16-byte aligned buffers");
    HIPCHK(hipSetDevice(h->device));
    const size_t esz = is_f64 ? 8 : 4;
    if (stage == 0) return time_copy16(h, "ctk_debug_time_lwa", h->lw_knobs, x_dev, out_dev, steps * (int64_t)ny * nx * (int64_t)esz, reps, ms2);
    LwaHost t;
    CTKCHK(lwa_check("ctk_debug_time_lwa", h, steps, ny, nx, a, t));
    CtkLwaPlan pl;
    CTKCHK(lwa_plan_of(h, "ctk_debug_time_lwa", (int)esz, t, nx, steps, true, pl));
    LwaTab tab;
    CTKCHK(lwa_table(h, t, tab));
    CTKCHK(ensure(h, h->lw_ref, (size_t)steps * ny * esz));
    auto contour = [&]() -> int {
        return is_f64 ? launch_lwa_contour<double>(h, (const double *)x_dev, ny, nx, steps, tab, t, pl, (double *)h->lw_ref.p)
                      : launch_lwa_contour<float>(h, (const float *)x_dev, ny, nx, steps, tab, t, pl, (float *)h->lw_ref.p);
    };
    if (stage == 1) return time_launches(h, "ctk_debug_time_lwa", reps, ms2, contour);
    CTKCHK(contour());
    return time_launches(h, "ctk_debug_time_lwa", reps, ms2, [&]() -> int {
        return is_f64 ? launch_lwa_integral<double>(h, (const double *)x_dev, ny, nx, steps, tab, t, pl, (const double *)h->lw_ref.p, part, (double *)out_dev)
                      : launch_lwa_integral<float>(h, (const float *)x_dev, ny, nx, steps, tab, t, pl, (const float *)h->lw_ref.p, part, (float *)out_dev);
    });
}
