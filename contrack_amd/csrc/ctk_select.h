// ctk_select.h -- the exact radix selection the three percentile entries share (device code only; included by ctk_api.hip behind
// ctk_forms.h): the order-preserving integer keys of a float (an_key), numpy's linear interpolation from order statistics
// (an_np_quantile) and the per-pixel selection with its histograms in LDS (pf_select).  Who calls it:
//   k_quantile (ctk_anom.hip)                      the scalar threshold: one pool per grid point, the whole time axis
//   k_pfield_direct / k_pfield_ring (ctk_pfield.hip)  the threshold field: one pool per (group, grid point)
//   the sweeps of ctk_pctl.hip                      an_key / an_np_quantile / pctl_atomic_min only (pooled bands, another algorithm)
#pragma once

// gfx950 only.  PfSel<KT, 64, 256> alone keeps 67 KB of static LDS per workgroup (64 pixels x 257 histogram bins, and the partial sums):
// more than the 64 KB a workgroup gets on gfx90a / gfx942.  The Makefile's ARCH is overridable for gfx950 variants (xnack / sramecc
// suffixes), not for other parts.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libcontrack_hip.so is written for gfx950 (MI355X): build with ARCH=gfx950"
#endif

template <typename VT>
__device__ __forceinline__ bool an_isnan(VT v) { return v != v; }

__device__ __forceinline__ uint32_t an_key(float v) { const uint32_t u = __float_as_uint(v); return (u >> 31) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint64_t an_key(double v) { const uint64_t u = (uint64_t)__double_as_longlong(v); return (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
__device__ __forceinline__ float an_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ double an_unkey(uint64_t k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }

// np.quantile(method='linear') of n >= 1 values from its order statistics: a = the value of rank lo = floor((n - 1) q), le = how
// many values are <= a, nx = the smallest value above a (read only where rank lo + 1 exists and is not a again).  Shared by
// pf_select and k_pctl_finish (ctk_pctl.hip).
__device__ __forceinline__ double an_np_quantile(uint64_t n, double q, double a, double nx, uint64_t le)
{
    const double h = ((double)n - 1.0) * q;
    const uint64_t lo = (uint64_t)floor(h);
    const double t = h - (double)lo;
    const double bb = (le > lo + 1 || lo + 1 >= n) ? a : nx;
    // numpy's _lerp exactly: a + (b - a) * t, taken from the other end for t >= 0.5 -- no shortcut for t == 0 or a == b
    // (numpy gives NaN there when a or b is infinite: inf * 0, inf - inf)
    const double d = bb - a;
    double r = a + d * t;
    if (t >= 0.5) r = bb - d * (1.0 - t);
    return r;
}

__device__ __forceinline__ void pctl_atomic_min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
__device__ __forceinline__ void pctl_atomic_min(uint64_t *p, uint64_t v) { atomicMin((unsigned long long *)p, (unsigned long long)v); }

template <typename KT, int TILE, int NT>
struct PfSel {
    uint32_t hist[TILE][257];
    uint32_t part[TILE][NT / TILE];      // sums of 256 / (NT / TILE) consecutive bins
    uint32_t n[TILE], k[TILE], k0[TILE], le[TILE];
    KT prefix[TILE], next[TILE];
};

// the q-quantile of the `len` pool values fetch(0 .. len) of this lane's pixel (tid % TILE; the NT / TILE lanes tid / TILE of a pixel
// share the pool); every thread of the workgroup calls it, lane 0 of a live pixel gets the result.  Ends behind a barrier.
template <typename VT, typename KT, int TILE, int NT, typename F>
__device__ __forceinline__ double pf_select(PfSel<KT, TILE, NT> &S, F fetch, int len, bool live, double q)
{
    constexpr int L = NT / TILE, SEG = 256 / L, NB = (int)sizeof(KT);
    static_assert(NT % TILE == 0 && L <= 256 && 256 % L == 0, "lanes per pixel must divide the 256 bins");
    static_assert(sizeof(PfSel<KT, TILE, NT>) <= ctk_pfield_select_bytes(TILE, NT), "ctk_pfield_select_bytes is what the plan counts");
    const int tid = (int)threadIdx.x, px = tid % TILE, lane = tid / TILE;
    if (lane == 0) { S.prefix[px] = 0; S.next[px] = ~(KT)0; S.n[px] = 0; S.le[px] = 0; }
#pragma unroll
    for (int b = NB - 1; b >= 0; b--) {
        const bool first = b == NB - 1;
        for (int i = tid; i < TILE * 257; i += NT) (&S.hist[0][0])[i] = 0;
        __syncthreads();
        if (live && (first || S.n[px])) {
            const KT pre = S.prefix[px];
            KT nx = ~(KT)0;
            for (int j = lane; j < len; j += L) {
                const VT v = fetch(j);
                if (an_isnan(v)) continue;                                     // (np.nanquantile)
                const KT k = an_key(v);
                const KT up = first ? pre : (KT)(k >> (8 * (b + 1) < 8 * NB ? 8 * (b + 1) : 0));
                if (up == pre) atomicAdd(&S.hist[px][(uint32_t)(k >> (8 * b)) & 255u], 1u);
                else if (b == 0 && up > pre && k < nx) nx = k;
            }
            if (b == 0 && nx != ~(KT)0) pctl_atomic_min(&S.next[px], nx);
        }
        __syncthreads();
        if (live) {
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < SEG; i++) s += S.hist[px][lane * SEG + i];
            S.part[px][lane] = s;
        }
        __syncthreads();
        if (lane == 0 && live) {
            uint32_t n = S.n[px];
            if (first) {
                n = 0;
                for (int i = 0; i < L; i++) n += S.part[px][i];
                const uint32_t k0 = n ? (uint32_t)floor(((double)n - 1.0) * q) : 0u;
                S.n[px] = n; S.k0[px] = k0; S.k[px] = k0;
            }
            if (n) {
                const uint32_t k = S.k[px];
                uint32_t cum = 0;
                int sg = 0;
                for (; sg < L - 1; sg++) { const uint32_t c = S.part[px][sg]; if (cum + c > k) break; cum += c; }
                int bin = sg * SEG;
                for (; bin < sg * SEG + SEG - 1; bin++) { const uint32_t c = S.hist[px][bin]; if (cum + c > k) break; cum += c; }
                const KT pre = S.prefix[px];
                S.prefix[px] = (KT)(pre << 8) | (KT)bin;
                S.k[px] = k - cum;
                if (b == 0) {
                    S.le[px] = (S.k0[px] - k) + cum + S.hist[px][bin];
                    int nb = bin + 1;                                          // the next key under the same prefix, if there is one
                    for (; nb < sg * SEG + SEG; nb++) if (S.hist[px][nb]) break;
                    if (nb == sg * SEG + SEG) {
                        int s2 = sg + 1;
                        for (; s2 < L; s2++) if (S.part[px][s2]) break;
                        nb = 256;
                        if (s2 < L) for (nb = s2 * SEG; !S.hist[px][nb]; nb++) {}
                    }
                    if (nb < 256) S.next[px] = (KT)(pre << 8) | (KT)nb;        // (below every key under a larger prefix)
                }
            }
        }
        __syncthreads();
    }
    if (lane != 0 || !live) return 0.0;
    if (!S.n[px]) return __builtin_nan("");
    const double a = (double)an_unkey(S.prefix[px]);
    return an_np_quantile((uint64_t)S.n[px], q, a, S.next[px] == ~(KT)0 ? a : (double)an_unkey(S.next[px]), (uint64_t)S.le[px]);
}
