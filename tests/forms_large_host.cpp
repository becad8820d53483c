// The launch rules of contrack_amd/csrc/ctk_forms.h that the map consumers ask (ctk_time_slice, ctk_composite_plan, ctk_band_plan and
// ctk_band_fits, ctk_centred_plan, ctk_level_plan, ctk_reversal_plan, ctk_anom_plan, ctk_stream_chunk, ctk_life_plan, ctk_pctl_form /
// ctk_pctl_refusal) at slabs of T * npix = 2^31 +- 1, 2^32 +- 1, 2^33 and 2^40 elements and at the shapes of
// tests/test_gpu_consumers_large.py: a launch stays below 2^32 work-items, gridDim.y stays within 65535, blocks == bps * steps, the time
// slices cover T, and a grid smaller than its blocks still walks all of them.  tests/test_forms_large_host.py builds this with
// -fsanitize=address,undefined and runs it: a signed overflow inside a rule ends the program.  No GPU, nothing of HIP is linked.
#include <cstdio>
#include <cstdint>
#include <vector>

#include "../contrack_amd/csrc/ctk_forms.h"

static int g_bad = 0;
static long g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { printf("%s:%d: %s   [%s]\n", __FILE__, __LINE__, #c, g_case); g_bad++; } } while (0)
static char g_case[160];

static const int64_t k32 = (int64_t)1 << 32;

// a striding kernel: workgroup b takes b, b + grid, ... below blocks -- all of them, each once
static bool walks_all(int64_t blocks, int64_t grid)
{
    if (blocks == 0) return true;
    if (grid < 1) return false;
    // the last workgroup's last piece and the count of pieces, without walking 2^40 of them
    const int64_t full = blocks / grid, rest = blocks % grid;                      // `rest` workgroups take full + 1 pieces
    const int64_t last = rest ? (rest - 1) + full * grid : (grid - 1) + (full - 1) * grid;
    return last == blocks - 1 && rest * (full + 1) + (grid - rest) * full == blocks;
}

// the rules that see the plane as npix pixels and T steps
static void slab(int64_t T, int64_t npix)
{
    snprintf(g_case, sizeof g_case, "T=%lld npix=%lld", (long long)T, (long long)npix);
    // k_freq / k_spell: slices of the T steps in gridDim.y (kSpellSliceMin 16 and kFreqSliceMin, kSliceMax 64, kSliceWaves 16384)
    for (int64_t smin : {(int64_t)1, (int64_t)4, (int64_t)16})
        for (int64_t forced : {(int64_t)0, (int64_t)1, (int64_t)7}) {
            const int64_t s = ctk_time_slice(forced, T, npix, smin, 64, 16384);
            CHECK(s >= 1);
            const int64_t gy = (T + s - 1) / s;
            CHECK(gy >= 1 && gy <= 65535);
            CHECK(gy * s >= T && (gy - 1) * s < T);                                // the slices cover T, none is empty
            if (!forced && T <= 65535 * smin) CHECK(s >= smin && s <= 64);
        }
    // k_composite
    for (int eb : {4, 8})
        for (int u : {-1, 1, 5, 16, 1000}) {
            const CtkCompositePlan p = ctk_composite_plan(eb, npix, u);
            CHECK(p.unroll >= 1 && p.unroll <= CTK_COMPOSITE_UNROLL_MAX && (p.unroll & (p.unroll - 1)) == 0);
            CHECK(p.blocks * CTK_COMPOSITE_THREADS >= npix && (p.blocks - 1) * CTK_COMPOSITE_THREADS < npix);
            CHECK(p.grid >= 1 && (int64_t)p.grid * CTK_COMPOSITE_THREADS < k32 && (int64_t)p.grid <= p.blocks);
            CHECK(walks_all(p.blocks, p.grid));
        }
    // k_level_mean: npix pixels, T steps of nsel levels
    for (int eb : {4, 8})
        for (int64_t nsel : {(int64_t)1, (int64_t)3, (int64_t)8, (int64_t)CTK_LEVEL_MAX_SEL})
            for (bool al : {true, false})
                for (int64_t gmax : {(int64_t)CTK_LEVEL_GRID_MAX, (int64_t)1, (int64_t)1000, k32 * 4}) {
                    const CtkLevelPlan p = ctk_level_plan(eb, nsel, npix, T, al, gmax);
                    CHECK(p.vpt == (p.vec ? 16 / eb : 1) && (!p.vec || (npix * eb) % 16 == 0));
                    CHECK(p.bps * CTK_LEVEL_THREADS * p.vpt >= npix && (p.bps - 1) * CTK_LEVEL_THREADS * p.vpt < npix);
                    CHECK(p.blocks == p.bps * T);
                    CHECK(p.grid >= 1 && (int64_t)p.grid * CTK_LEVEL_THREADS < k32 && (int64_t)p.grid <= p.blocks);
                    CHECK(walks_all(p.blocks, p.grid));
                }
    // k_anom_ring / k_anom_plain: T output steps
    for (int eb : {4, 8})
        for (int smooth : {1, 2, 32, 33, 1000}) {
            const CtkAnomPlan p = ctk_anom_plan(eb, smooth, T, npix);
            CHECK(p.tile >= 1 && p.gy >= 1 && p.gy <= 65535);
            CHECK((int64_t)p.gy * p.tile >= T && ((int64_t)p.gy - 1) * p.tile < T);
            if (npix < k32 * CTK_ANOM_THREADS - CTK_ANOM_THREADS) CHECK((int64_t)p.gx * CTK_ANOM_THREADS >= npix && ((int64_t)p.gx - 1) * CTK_ANOM_THREADS < npix);
            CHECK((p.form == CTK_ANOM_RING) == ((size_t)smooth * CTK_ANOM_THREADS * eb <= CTK_ANOM_RING_BYTES) && p.lds <= CTK_ANOM_RING_BYTES);
        }
    // the streamed entries: steps per chunk
    for (int64_t given : {(int64_t)0, (int64_t)1, (int64_t)1000, T, T + 5})
        for (int64_t halo : {(int64_t)1, (int64_t)31}) {
            const size_t step_bytes = (size_t)npix * 4;
            const int64_t c = ctk_stream_chunk(given, T, step_bytes, halo);
            CHECK(c >= 1 && c <= T);
            if (given > 0 && given <= T && given >= halo) CHECK(c == given);
            if (!given && halo <= T) CHECK(c >= halo || c == T);
        }
    // the percentile sweeps over a band of npix values
    for (int G : {1, 12, 366})
        for (int W : {1, 3, 400}) {
            const CtkPctlForm f = ctk_pctl_form(32, npix, G, W);
            CHECK(f.levels == 3 && f.bits[0] + f.bits[1] + f.bits[2] == 32 && f.shift[2] == 0 && f.sweeps == 4);
            const int64_t chunks = (npix + CTK_PCTL_CHUNK - 1) / CTK_PCTL_CHUNK;
            const int64_t per_group = (T + G - 1) / G;
            const int r = ctk_pctl_refusal(npix, G, W, per_group);
            if (r == CTK_PCTL_FINE) {
                CHECK(chunks <= 65535 && (int64_t)f.chunks == chunks && (int64_t)f.chunks * f.chunk >= npix);
                CHECK(per_group == 0 || per_group * npix <= 0xffffffffll);                 // the uint32 counters of a day
                // (gridDim.x = T is not this rule's: the entries take T <= 2^31 - 1, and from 2^24 steps on the launch of the
                // 256-thread sweep has 2^32 work-items or more, which the runtime refuses with an error)
            } else {
                CHECK(chunks > 65535 || per_group * (double)npix > 4294967295.0 || (W < G && W > CTK_PCTL_MAX_WINDOW) || (int64_t)G * f.stride > CTK_PCTL_MAX_SLOTS);
            }
            CHECK(ctk_pctl_form(64, npix, G, W).levels == 6);
        }
}

// the rules that see rows and columns
static void grid(int64_t T, int ny, int nx)
{
    snprintf(g_case, sizeof g_case, "T=%lld ny=%d nx=%d", (long long)T, ny, nx);
    // k_band / k_band_sect
    for (bool al : {true, false})
        for (int nsect : {0, 2, 64}) {
            if (!ctk_band_fits(T, nx, nsect)) continue;                            // the entries refuse
            const CtkBandPlan p = ctk_band_plan(T, nx, al);
            CHECK(p.quads * 4 >= nx && (p.quads - 1) * 4 < nx);
            CHECK((int64_t)p.grid * CTK_BAND_THREADS >= T * p.quads && ((int64_t)p.grid - 1) * CTK_BAND_THREADS < T * p.quads);
            CHECK((int64_t)p.grid * CTK_BAND_THREADS < k32);
            const int64_t n = T * (nsect > 0 ? nsect : 1), gs = (n + CTK_BAND_THREADS - 1) / CTK_BAND_THREADS;
            CHECK(gs * CTK_BAND_THREADS < k32);
            CHECK(p.vec == (nx % 4 == 0 && al) && p.rows == CTK_BAND_ROWS);
        }
    // k_reversal
    for (int eb : {4, 8})
        for (bool al : {true, false})
            for (int64_t gmax : {(int64_t)CTK_LEVEL_GRID_MAX, (int64_t)1, (int64_t)1000}) {
                const CtkReversalPlan p = ctk_reversal_plan(eb, ny, nx, T, al, gmax);
                const int64_t lanes = (int64_t)ny * (nx / p.vpt);
                CHECK(!p.vec || ((int64_t)nx * eb) % 16 == 0);
                CHECK(p.bps * CTK_REVERSAL_THREADS >= lanes && (p.bps - 1) * CTK_REVERSAL_THREADS < lanes);
                CHECK(p.blocks == p.bps * T);
                CHECK(p.grid >= 1 && (int64_t)p.grid * CTK_REVERSAL_THREADS < k32 && (int64_t)p.grid <= p.blocks);
                CHECK(walks_all(p.blocks, p.grid));
            }
    // the lifecycle strips: nsx * nby workgroups per step cover the plane
    for (bool f64 : {false, true})
        for (uintptr_t off : {(uintptr_t)0, (uintptr_t)4, (uintptr_t)16}) {
            const CtkLifePlan p = ctk_life_plan(T, ny, nx, f64, (uintptr_t)4096, (uintptr_t)4096 + off);
            CHECK(p.rw >= 1 && (int64_t)p.nsx * CTK_LIFE_SW >= nx && ((int64_t)p.nsx - 1) * CTK_LIFE_SW < nx);
            CHECK((int64_t)p.nby * p.rw * CTK_LIFE_WAVES >= ny && ((int64_t)p.nby - 1) * p.rw * CTK_LIFE_WAVES < ny);
            CHECK(p.ks >= 1 && p.ks <= CTK_LIFE_KS_MAX);
            if (nx <= CTK_LIFE_KS_BYTES * 8) CHECK((int64_t)p.ks * ((nx + 31) / 32) * 4 <= CTK_LIFE_KS_BYTES);       // (a bit per column of one id fits)
            CHECK(p.vec == ((nx & 3) == 0 && (off & (f64 ? 31u : 15u)) == 0));
        }
}

// block-centred composite: bins x cells
static void centred(int64_t nbins, int hy, int hx, int64_t max_bin, int64_t kept)
{
    snprintf(g_case, sizeof g_case, "nbins=%lld hy=%d hx=%d max_bin=%lld kept=%lld", (long long)nbins, hy, hx, (long long)max_bin, (long long)kept);
    const int64_t wcells = (2 * (int64_t)hy + 1) * (2 * (int64_t)hx + 1);
    for (int eb : {4, 8})
        for (int form : {-1, 0, 1})
            for (int th : {-1, 64, 200, 4096}) {
                const CtkCentredPlan p = ctk_centred_plan(eb, nbins, wcells, max_bin, kept, form, -1, th);
                CHECK(p.threads == 64 || p.threads == 128 || p.threads == 256);
                CHECK(p.parts * p.threads >= wcells && (p.parts - 1) * p.threads < wcells);
                CHECK(p.blocks == nbins * p.parts);
                const int64_t wg = p.form ? 64 * CTK_CENTRED_FED_WAVES : p.threads;
                CHECK(p.grid >= 1 && (int64_t)p.grid * wg < k32 && (int64_t)p.grid <= p.blocks);
                CHECK(walks_all(p.blocks, p.grid));
                CHECK(p.unroll >= 1 && p.unroll <= CTK_CENTRED_UNROLL_MAX);
            }
}

int main()
{
    const int64_t sizes[] = {((int64_t)1 << 31) - 1, (int64_t)1 << 31, ((int64_t)1 << 31) + 1, k32 - 1, k32, k32 + 1, (int64_t)1 << 33, (int64_t)1 << 40};
    const int64_t plane = 721 * 1440;
    for (int64_t N : sizes) {
        slab(N, 1);                                                                // all of it in time
        slab(1, N);                                                                // all of it in one plane
        slab((N + plane - 1) / plane, plane);                                      // quarter-degree planes
        slab(N / plane, plane);
        for (int64_t npix : {(int64_t)65160, (int64_t)1 << 20, (int64_t)3, (int64_t)257})
            for (int64_t d : {(int64_t)-1, (int64_t)0, (int64_t)1})
                if (N / npix + d >= 1) slab(N / npix + d, npix);
        grid((N + plane - 1) / plane, 721, 1440);
        grid(N / 65160, 181, 360);
        grid(N, 1, 1);
        grid(N / 7 + 1, 1, 7);
        if (N / 3 < 0x7fffffff) grid(3, 1, (int)(N / 3));
        if (N / 5 < 0x7fffffff) grid(1, (int)(N / 5), 5);
        grid(N / (1024 * 1024) + 1, 1024, 1023);
    }
    // the shapes of tests/test_gpu_consumers_large.py
    slab(4200, plane);
    slab(1050, plane);                                                             // the level mean: 1050 steps of 4 levels
    slab(4200, 2 * 1440);                                                          // the band of the std and percentile entries
    grid(4200, 721, 1440);
    {
        snprintf(g_case, sizeof g_case, "the large test's own launches");
        const int64_t s = ctk_time_slice(0, 4200, plane, 16, 64, 16384);
        CHECK(s == 64 && (4200 + s - 1) / s == 66);
        const CtkLevelPlan lv = ctk_level_plan(4, 3, plane, 1050, true);
        CHECK(lv.vec == 1 && lv.bps == 1014 && lv.blocks == 1014 * 1050 && (int64_t)lv.grid == lv.blocks && lv.xcd == 1);
        const CtkReversalPlan rv = ctk_reversal_plan(4, 721, 1440, 4200, true);
        CHECK(rv.vec == 1 && rv.bps == 1014 && rv.blocks == 1014 * 4200 && (int64_t)rv.grid == rv.blocks);
        const CtkBandPlan bd = ctk_band_plan(4200, 1440, true);
        CHECK(bd.vec && bd.quads == 360 && bd.grid == (4200 * 360 + 255) / 256 && ctk_band_fits(4200, 1440, 2));
        CHECK(ctk_pctl_refusal(2 * 1440, 12, 3, 350) == CTK_PCTL_FINE);
        CHECK(ctk_pfield_plan(4, 1050, 12, 3).form == CTK_PFIELD_RING);
        CHECK(ctk_std_plan(12, 3, 1).tile == CTK_STD_MAX_TILE);
        // what the band entries refuse: from 2^32 work-items on, and no product of theirs overflows on the way
        CHECK(ctk_band_fits(11930000, 1440, 0) && !ctk_band_fits(11940000, 1440, 0) && !ctk_band_fits(INT64_MAX, 2147483647, 2147483647));
        CHECK(ctk_band_fits(67108000, 1, 64) && !ctk_band_fits(67109000, 1, 64));
    }
    for (int64_t nbins : {(int64_t)1, (int64_t)3, (int64_t)400, (int64_t)1 << 24, ((int64_t)1 << 31) - 1})
        for (int h : {0, 2, 20, 500})
            for (int64_t mb : {(int64_t)1, (int64_t)40, (int64_t)127, (int64_t)128, k32 - 1})
                if ((2 * (int64_t)h + 1) * (2 * (int64_t)h + 2 + 1) * nbins < ((int64_t)1 << 31)) centred(nbins, h, h + 1, mb, mb * (nbins < 1000 ? nbins : 1000));
    centred(3, 2, 3, 20, 40);
    if (g_bad) { printf("forms_large_host: %d of %ld checks failed\n", g_bad, g_checks); return 1; }
    printf("forms_large_host: ok (%ld checks)\n", g_checks);
    return 0;
}
