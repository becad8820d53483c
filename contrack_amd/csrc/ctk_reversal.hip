// ctk_reversal.hip -- the second family of blocking indices on the device (included by ctk_api.hip): the reversal of the meridional
// height gradient of Tibaldi & Molteni (1990), in two dimensions as Scherrer et al. (2006) and Davini et al. (2012) evaluate it.  A
// stencil in latitude over a (steps, ny, nx) field; include/contrack_hip.h states the arithmetic, tests/reversal_util.py is its numpy
// statement.  Per pixel of an ACTIVE row j with its equatorward partner row eq[j], its poleward partner po[j] and (third criterion)
// eq2[j], all in float64, no fused multiply-add:
//     dS = z[j] - z[eq] ;  dN = z[po] - z[j] ;  dS2 = z[eq] - z[eq2]
//     blocked = dS > tS[j]  and  dN < tN[j]  [and dS2 < tS2[j]]              -- limits pre-multiplied by the row distances: no divide
//     out = blocked ? (dtype)(dS / dE[j]) : 0      ('gradient')        out = blocked ? 1 : 0      ('mask')
// Inactive rows (eq[j] < 0) are 0 and read nothing.  The output is the kind of field ctk_track_* tracks with threshold 0, op '>'.
//
// k_reversal: one lane per 16 bytes of adjacent longitudes of one row of one step (4 float32 / 2 float64; LevelLane of ctk_level.hip),
// or per pixel where a row does not start on a 16-byte boundary (an odd row length, an offset pointer).  The lane loads its own row
// and the two or three partner rows -- plain loads: every row is wanted again by up to three other rows of the same plane, those
// reads are meant to be L2 hits -- and stores 16 bytes, zeros on inactive rows: the kernel writes the whole plane, nothing is set
// beforehand.  The row table (partners, dE, limits) lies in a small device buffer read through the constant address space.  A
// workgroup stays inside one step (ctk_reversal_plan, ctk_forms.h); large launches give every XCD one contiguous eighth of the
// workgroups (xcd_chunk), so that all readers of a row share one L2.
//
// Host-array entries: the row-band plane producer of ctk_api.hip (row_band_produce) with the rows [r0, r1) that some active row reads
// and the rows [a0, a1) the active rows span.  The device chunks keep the full-plane layout, so the kernel is the one of the _dev entries.
#pragma once

// the row table of a call on the device: dE, tS, tN, tS2 (ny float64 each), then eq, po, eq2 (ny int32 each)
struct ReversalTab {
    const double *dE, *tS, *tN, *tS2;
    const int32_t *eq, *po, *eq2;
};

// z, out: (steps, ny, nx).  lpr lanes per row (nx / N); workgroup b of `blocks` = bps * steps takes part b % bps of the plane of step
// b / bps.  Lane q of a plane owns pixels [c, c + N) of row q / lpr.
template <typename VT, bool VEC, bool SECOND, bool MASK>
__global__ __launch_bounds__(CTK_REVERSAL_THREADS) void k_reversal(const VT *__restrict__ z, int ny, int nx, uint32_t lpr, int64_t bps, int64_t blocks,
                                                                   ReversalTab tab, VT *__restrict__ out, int xcd)
{
#pragma clang fp contract(off)
    typedef LevelLane<VT, VEC> L;
    typedef typename L::type V;
    ctk_const_f64 *dE = (ctk_const_f64 *)tab.dE, *tS = (ctk_const_f64 *)tab.tS, *tN = (ctk_const_f64 *)tab.tN, *tS2 = (ctk_const_f64 *)tab.tS2;
    ctk_const_i32 *eq = (ctk_const_i32 *)tab.eq, *po = (ctk_const_i32 *)tab.po, *eq2 = (ctk_const_i32 *)tab.eq2;
    const int64_t npix = (int64_t)ny * nx;
    const uint32_t lanes = (uint32_t)ny * lpr;                                    // lanes of one plane (npix < 2^31: reversal_check)
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b < blocks; b += gridDim.x) {       // (a permutation of the launch's workgroups)
        const int64_t s = b / bps;
        const uint32_t q = (uint32_t)(b - s * bps) * CTK_REVERSAL_THREADS + threadIdx.x;
        if (q >= lanes) continue;
        const uint32_t j = q / lpr, c = (q - j * lpr) * L::N;
        const VT *zs = z + s * npix + c;                                          // column c of row 0 of this step (64-bit throughout)
        V r;
#pragma unroll
        for (int i = 0; i < L::N; i++) L::set(r, i, (VT)0);
        const int je = eq[j];
        if (je >= 0) {
            const int jp = po[j];
            const V own = *(const V *)(zs + (int64_t)j * nx), ve = *(const V *)(zs + (int64_t)je * nx), vp = *(const V *)(zs + (int64_t)jp * nx);
            V ve2 = ve;
            if (SECOND) ve2 = *(const V *)(zs + (int64_t)eq2[j] * nx);
            const double lim_s = tS[j], lim_n = tN[j], lim_s2 = SECOND ? tS2[j] : 0.0, de = dE[j];
#pragma unroll
            for (int i = 0; i < L::N; i++) {
                const double dS = L::get(own, i) - L::get(ve, i), dN = L::get(vp, i) - L::get(own, i);
                bool blocked = dS > lim_s && dN < lim_n;                           // (a NaN anywhere: every compare false)
                if (SECOND) blocked = blocked && (L::get(ve, i) - L::get(ve2, i)) < lim_s2;
                if (blocked) L::set(r, i, MASK ? (VT)1 : (VT)(dS / de));           // float64 divide, one rounding to VT -- blocked pixels only
            }
        }
        *(V *)(out + s * npix + (int64_t)j * nx + c) = r;
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// the row table of a call as the caller gave it (host pointers; eq2 / tS2 null: two criteria)
struct ReversalArgs {
    const int32_t *eq, *po, *eq2;
    const double *dE, *tS, *tN, *tS2;
    int mask;
};

static int reversal_check(const char *who, const void *h, int64_t steps, int ny, int nx, const ReversalArgs &a)
{
    if (!h || !a.eq || !a.po || !a.dE || !a.tS || !a.tN || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments (null pointer or a size below 1)", who);
    if (steps < 1) return ctk_set_error(CTK_E_INVALID, "%s: steps = %lld", who, (long long)steps);
    if ((a.eq2 == nullptr) != (a.tS2 == nullptr)) return ctk_set_error(CTK_E_INVALID, "%s: eq2 and tS2 go together (both or neither)", who);
    if ((int64_t)ny * nx > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: a plane of %lld pixels (at most 2^31 - 1)", who, (long long)ny * nx);
    for (int j = 0; j < ny; j++) {
        const int64_t e = a.eq[j], p = a.po[j], e2 = a.eq2 ? a.eq2[j] : 0;
        if (e < -1 || e >= ny || p < -1 || p >= ny || e2 < -1 || e2 >= ny)
            return ctk_set_error(CTK_E_INVALID, "%s: row %d has a partner outside [-1, %d) (eq %lld, po %lld, eq2 %lld)", who, j, ny, (long long)e, (long long)p, (long long)e2);
        if (e < 0) continue;
        if (p < 0 || e2 < 0) return ctk_set_error(CTK_E_INVALID, "%s: the active row %d lacks a partner (po %lld, eq2 %lld)", who, j, (long long)p, (long long)e2);
        if (!(a.dE[j] > 0.0) || !std::isfinite(a.dE[j])) return ctk_set_error(CTK_E_INVALID, "%s: dE[%d] = %g (must be finite and > 0)", who, j, a.dE[j]);
        if (!std::isfinite(a.tS[j]) || !std::isfinite(a.tN[j]) || (a.tS2 && !std::isfinite(a.tS2[j])))
            return ctk_set_error(CTK_E_INVALID, "%s: a limit of row %d is not finite", who, j);
    }
    return CTK_OK;
}

// the device table of a call (inactive rows: partners -1, zeros)
static int reversal_table(ctk_handle *h, int ny, const ReversalArgs &a, ReversalTab &t)
{
    const size_t n = (size_t)ny;
    CTKCHK(ensure(h, h->gr_tab, n * 44));
    std::vector<double> d(4 * n, 0.0);
    std::vector<int32_t> r(3 * n, -1);
    for (size_t j = 0; j < n; j++) {
        if (a.eq[j] < 0) continue;
        d[j] = a.dE[j]; d[n + j] = a.tS[j]; d[2 * n + j] = a.tN[j]; d[3 * n + j] = a.tS2 ? a.tS2[j] : 0.0;
        r[j] = a.eq[j]; r[n + j] = a.po[j]; r[2 * n + j] = a.eq2 ? a.eq2[j] : a.eq[j];
    }
    HIPCHK(hipStreamSynchronize(h->stream));                                  // (a launch still reading the table of the call before)
    HIPCHK(hipMemcpy(h->gr_tab.p, d.data(), 4 * n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy((char *)h->gr_tab.p + 4 * n * 8, r.data(), 3 * n * 4, hipMemcpyHostToDevice));
    t.dE = (const double *)h->gr_tab.p; t.tS = t.dE + n; t.tN = t.tS + n; t.tS2 = t.tN + n;
    t.eq = (const int32_t *)(t.tS2 + n); t.po = t.eq + n; t.eq2 = t.po + n;
    return CTK_OK;
}

// out[s] = the index of step s of z (steps, ny, nx), on the handle's stream
template <typename VT>
static int launch_reversal(ctk_handle *h, const VT *z, int ny, int nx, int64_t steps, const ReversalTab &tab, bool second, bool mask, VT *out)
{
    const bool aligned = (((uintptr_t)z | (uintptr_t)out) & 15) == 0;
    const CtkReversalPlan pl = ctk_reversal_plan((int)sizeof(VT), ny, nx, steps, aligned, h->gr_knobs.cap());
    h->gr_knobs.launched(pl.vec, pl.grid);
    const int xcd = h->gr_knobs.xcd(pl.xcd);
    const uint32_t lpr = (uint32_t)(nx / pl.vpt);
#define CTK_REVERSAL_LAUNCH(V, S, M) k_reversal<VT, V, S, M><<<pl.grid, CTK_REVERSAL_THREADS, 0, h->stream>>>(z, ny, nx, lpr, pl.bps, pl.blocks, tab, out, xcd)
#define CTK_REVERSAL_SM(V) do { if (second) { if (mask) CTK_REVERSAL_LAUNCH(V, true, true); else CTK_REVERSAL_LAUNCH(V, true, false); } \
                                else { if (mask) CTK_REVERSAL_LAUNCH(V, false, true); else CTK_REVERSAL_LAUNCH(V, false, false); } } while (0)
    if (pl.vec) CTK_REVERSAL_SM(true); else CTK_REVERSAL_SM(false);
#undef CTK_REVERSAL_SM
#undef CTK_REVERSAL_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

template <typename VT>
static int reversal_dev_impl(ctk_handle *h, const VT *x_dev, int64_t steps, int ny, int nx, const ReversalArgs &a, VT *out_dev, const char *who)
{
    CTKCHK(reversal_check(who, h, steps, ny, nx, a));
    if (!x_dev || !out_dev) return ctk_set_error(CTK_E_INVALID, "%s: null input or output", who);
    HIPCHK(hipSetDevice(h->device));
    ReversalTab tab;
    CTKCHK(reversal_table(h, ny, a, tab));
    CTKCHK(launch_reversal<VT>(h, x_dev, ny, nx, steps, tab, a.eq2 != nullptr, a.mask != 0, out_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

extern "C" int ctk_reversal_f32_dev(ctk_handle *h, const float *x_dev, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2,
                                    const double *dE, const double *tS, const double *tN, const double *tS2, int mask, float *out_dev)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    return reversal_dev_impl<float>(h, x_dev, steps, ny, nx, a, out_dev, "ctk_reversal_f32_dev");
}
extern "C" int ctk_reversal_f64_dev(ctk_handle *h, const double *x_dev, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2,
                                    const double *dE, const double *tS, const double *tN, const double *tS2, int mask, double *out_dev)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    return reversal_dev_impl<double>(h, x_dev, steps, ny, nx, a, out_dev, "ctk_reversal_f64_dev");
}

template <typename VT>
static int reversal_stream_impl(ctk_handle *h, StreamIO &io, int64_t steps, int ny, int nx, const ReversalArgs &a, int64_t chunk_steps, int keep_resident, const char *name)
{
    CTKCHK(reversal_check(name, h, steps, ny, nx, a));
    CTKCHK(row_band_begin(h, io, steps, (size_t)ny * nx * sizeof(VT), sizeof(VT), chunk_steps, keep_resident, name));
    const CtkReversalRows rr = ctk_reversal_rows(a.eq, a.po, a.eq2, ny);
    ReversalTab tab;
    return row_band_produce(
        h, io, steps, ny, nx, {rr.r0, rr.r1, rr.a0, rr.a1}, keep_resident, name, [&]() -> int { return reversal_table(h, ny, a, tab); },
        [&](const ProduceIn &c, char *out) -> int { return launch_reversal<VT>(h, (const VT *)c.dev, ny, nx, c.nt, tab, a.eq2 != nullptr, a.mask != 0, (VT *)out); });
}

extern "C" int ctk_reversal_f32(ctk_handle *h, const float *x, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2, const double *dE,
                                const double *tS, const double *tN, const double *tS2, int mask, float *out, int64_t chunk_steps, int keep_resident)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return reversal_stream_impl<float>(h, io, steps, ny, nx, a, chunk_steps, keep_resident, "ctk_reversal_f32");
}
extern "C" int ctk_reversal_f64(ctk_handle *h, const double *x, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po, const int32_t *eq2, const double *dE,
                                const double *tS, const double *tN, const double *tS2, int mask, double *out, int64_t chunk_steps, int keep_resident)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    StreamIO io;
    io.host_in = x; io.host_out_v = out;
    return reversal_stream_impl<double>(h, io, steps, ny, nx, a, chunk_steps, keep_resident, "ctk_reversal_f64");
}
extern "C" int ctk_reversal_stream_cb(ctk_handle *h, int elem_bytes, int64_t steps, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *eq,
                                      const int32_t *po, const int32_t *eq2, const double *dE, const double *tS, const double *tN, const double *tS2, int mask,
                                      ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps, int keep_resident)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    StreamIO io;
    CTKCHK(stream_cb_io("ctk_reversal_stream_cb", h, elem_bytes, reader, reader_user, writer, writer_user, io));
    if (elem_bytes == 8) return reversal_stream_impl<double>(h, io, steps, ny, nx, a, chunk_steps, keep_resident, "ctk_reversal_stream_cb");
    return reversal_stream_impl<float>(h, io, steps, ny, nx, a, chunk_steps, keep_resident, "ctk_reversal_stream_cb");
}

// what ctk_reversal_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_reversal_plan(int elem_bytes, int64_t ny, int64_t nx, int64_t steps, int aligned, int64_t *out6)
{
    if (!out6 || (elem_bytes != 4 && elem_bytes != 8) || ny < 1 || nx < 1 || steps < 1 || ny * nx > 0x7fffffffll)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_reversal_plan: bad arguments");
    const CtkReversalPlan p = ctk_reversal_plan(elem_bytes, ny, nx, steps, aligned != 0);
    out6[0] = p.vec; out6[1] = p.vpt; out6[2] = p.bps; out6[3] = p.blocks; out6[4] = p.grid; out6[5] = p.xcd;
    return CTK_OK;
}

// test hook: out2 = { the form of the last k_reversal launch on this handle (1 vector, 0 scalar, -1 none yet), its workgroups }
extern "C" int ctk_debug_reversal_form(ctk_handle *h, int64_t *out2)
{
    return knobs_form(h, &ctk_handle::gr_knobs, out2);
}

// test hook / experiments (tools/reversal_probe.py) for the following k_reversal launches on this handle: the xcd_chunk mode (0 launch
// order, 1 eighths, n > 1 tiles of n workgroups; -1: the rule of ctk_reversal_plan) and a lower cap on the workgroups of a launch, so
// that a small case walks the stride loop (0: CTK_LEVEL_GRID_MAX)
extern "C" int ctk_debug_set_reversal(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    return knobs_set("ctk_debug_set_reversal", h, &ctk_handle::gr_knobs, xcd_mode, grid_max);
}

// measurement (tools/reversal_probe.py): k_reversal alone between HIP events on slabs in device memory -- one launch that is not
// counted, then `reps` timed ones; ms2 = {best, mean}.  eq == NULL: the plain copy kernel over the same two buffers instead (the
// whole slab rounded down to 16-byte words), in the workgroup order the k_reversal launch of this shape takes.
extern "C" int ctk_debug_time_reversal(ctk_handle *h, const void *x_dev, int is_f64, int64_t steps, int ny, int nx, const int32_t *eq, const int32_t *po,
                                       const int32_t *eq2, const double *dE, const double *tS, const double *tN, const double *tS2, int mask, void *out_dev, int reps,
                                       double *ms2)
{
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    if (!h || !x_dev || !out_dev || !ms2 || reps < 1 || steps < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_reversal: bad arguments");
    if (eq) CTKCHK(reversal_check("ctk_debug_time_reversal", h, steps, ny, nx, a));
    else if ((((uintptr_t)x_dev | (uintptr_t)out_dev) & 15) != 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_reversal: the copy needs 16-byte aligned buffers");
    HIPCHK(hipSetDevice(h->device));
    if (!eq) return time_copy16(h, "ctk_debug_time_reversal", h->gr_knobs, x_dev, out_dev, steps * (int64_t)ny * nx * (is_f64 ? 8 : 4), reps, ms2);
    ReversalTab tab;
    CTKCHK(reversal_table(h, ny, a, tab));
    return time_launches(h, "ctk_debug_time_reversal", reps, ms2, [&]() -> int {
        return is_f64 ? launch_reversal<double>(h, (const double *)x_dev, ny, nx, steps, tab, eq2 != nullptr, mask != 0, (double *)out_dev)
                      : launch_reversal<float>(h, (const float *)x_dev, ny, nx, steps, tab, eq2 != nullptr, mask != 0, (float *)out_dev);
    });
}
