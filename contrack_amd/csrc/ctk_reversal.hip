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
// Host-array entries: of every plane only the rows [r0, r1) that some active row reads travel to the device (one strided copy per
// chunk, the plane as pitch) and only the rows [a0, a1) the active rows span travel back; the rest of `out` is zeroed on the host.
// The device chunks keep the full-plane layout, so the kernel is the one of the _dev entries.  Two input and two output chunks on the
// handle's copy stream (stream_produce, ctk_api.hip).  keep_resident: the full-plane result is written into the resident slot of the
// field to track (an_out), where ctk_track_resident and the `resident` consumers find it.
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

// a plain copy of n16 16-byte words, one load and one store per lane: the floor of a read-once, write-once kernel over the same two
// buffers (ctk_debug_time_reversal)
__global__ __launch_bounds__(256) void k_reversal_copy(const i32x4 *__restrict__ src, i32x4 *__restrict__ dst, int64_t n16, int xcd)
{
    for (int64_t b = xcd_chunk(blockIdx.x, gridDim.x, xcd); b * 256 < n16; b += gridDim.x) {
        const int64_t i = b * 256 + threadIdx.x;
        if (i < n16) dst[i] = src[i];
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
    const CtkReversalPlan pl = ctk_reversal_plan((int)sizeof(VT), ny, nx, steps, aligned, h->gr_grid_dbg > 0 ? h->gr_grid_dbg : CTK_LEVEL_GRID_MAX);
    h->gr_form = pl.vec; h->gr_grid = pl.grid;
    const int xcd = h->gr_xcd_dbg >= 0 ? h->gr_xcd_dbg : pl.xcd;
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

// rows of every plane of `out` (steps, ny, nx) outside [a0, a1): zero
static void reversal_zero_rest(void *out, int64_t steps, size_t plane, size_t off, size_t width)
{
    if (width == plane) return;
    for (int64_t s = 0; s < steps; s++) {
        char *p = (char *)out + (size_t)s * plane;
        memset(p, 0, off);
        memset(p + off + width, 0, plane - off - width);
    }
}

template <typename VT>
static int reversal_stream_impl(ctk_handle *h, StreamIO &io, int64_t steps, int ny, int nx, const ReversalArgs &a, int64_t chunk_steps, int keep_resident, const char *name)
{
    CTKCHK(reversal_check(name, h, steps, ny, nx, a));
    if (!io.read && !io.host_in) return ctk_set_error(CTK_E_INVALID, "%s: null input", name);
    const bool sink = io.host_out_v || io.write_v;
    if (!sink && !keep_resident) return ctk_set_error(CTK_E_INVALID, "%s: nothing to produce (no output and keep_resident = 0)", name);
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps = %lld", name, (long long)chunk_steps);
    HIPCHK(hipSetDevice(h->device));
    const size_t row = (size_t)nx * sizeof(VT), plane = (size_t)ny * row;
    const CtkReversalRows rr = ctk_reversal_rows(a.eq, a.po, a.eq2, ny);
    io.esz = sizeof(VT);
    io.chunk = ctk_stream_chunk(chunk_steps, steps, plane);
    const double t_call = now_ms();
    CTKCHK(stream_setup(h, (size_t)io.chunk * plane, 0, io.read != nullptr));
    if (keep_resident) {
        h->an_T = -1; h->an_gen++; h->an_pct_n = -1;                   // the resident slab (if any) is dropped or about to be overwritten
        CTKCHK(ensure(h, h->an_out, (size_t)steps * plane));
        if (io.write_v) CTKCHK(stream_setup(h, 0, (size_t)io.chunk * plane, true));
    } else {
        CTKCHK(stream_setup(h, 0, (size_t)io.chunk * plane, io.write_v != nullptr));
    }
    ReversalTab tab;
    CTKCHK(reversal_table(h, ny, a, tab));
    // the rows of `out` that nothing is downloaded into are zeroed by a helper thread while the chunks travel (other bytes than the
    // copies write; at 1 degree, one hemisphere, that is three quarters of the array)
    struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } zero;
    if (io.host_out_v) zero.t = std::thread(reversal_zero_rest, io.host_out_v, steps, plane, (size_t)rr.a0 * row, (size_t)(rr.a1 - rr.a0) * row);
    // the chunks (stream_produce): io.host_in is the whole (steps, ny, nx) array (rows [r0, r1) of every plane travel), io.read a
    // reader of whole planes.  The results go to io.host_out_v (rows [a0, a1) of every plane) / io.write_v (whole planes) chunk by
    // chunk and (keep) into an_out.
    const size_t in_off = (size_t)rr.r0 * row, in_w = (size_t)(rr.r1 - rr.r0) * row, out_off = (size_t)rr.a0 * row, out_w = (size_t)(rr.a1 - rr.a0) * row;
    Producer p;
    p.in_bytes = (size_t)io.chunk * plane; p.out_step = plane;
    p.upload = [&](const ProduceIn &c) -> int {
        const char *src = c.src ? c.src : (const char *)io.host_in + (size_t)c.c0 * plane;
        if (in_w == plane) HIPCHK(hipMemcpyAsync(c.dev, src, (size_t)c.nt * plane, hipMemcpyHostToDevice, h->copy_stream));
        else if (in_w) HIPCHK(hipMemcpy2DAsync(c.dev + in_off, plane, src + in_off, plane, in_w, (size_t)c.nt, hipMemcpyHostToDevice, h->copy_stream));      // row s of the copy: rows [r0, r1) of step c0 + s
        return CTK_OK;
    };
    p.launch = [&](const ProduceIn &c, ProduceOut &o) -> int {
        o.t0 = c.c0; o.nt = c.nt;
        o.dev = keep_resident ? (char *)h->an_out.p + (size_t)c.c0 * plane : (char *)h->io_out.p + (size_t)c.b * (size_t)io.chunk * plane;
        return launch_reversal<VT>(h, (const VT *)c.dev, ny, nx, c.nt, tab, a.eq2 != nullptr, a.mask != 0, (VT *)o.dev);
    };
    if (out_w != plane)
        p.download = [&](const ProduceOut &o, char *dst) -> int {
            if (out_w) HIPCHK(hipMemcpy2D(dst + out_off, plane, o.dev + out_off, plane, out_w, (size_t)o.nt, hipMemcpyDeviceToHost));
            return CTK_OK;
        };
    const int rc = stream_produce(h, io, steps, name, p);
    if (zero.t.joinable()) zero.t.join();
    CTKCHK(stream_produce_end(h, io, rc, t_call));
    if (keep_resident) { h->an_T = steps; h->an_ny = ny; h->an_nx = nx; h->an_f64 = sizeof(VT) == 8; }
    return CTK_OK;
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
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_reversal_stream_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    if (h && !reader) return ctk_set_error(CTK_E_INVALID, "ctk_reversal_stream_cb: null reader");
    const ReversalArgs a = {eq, po, eq2, dE, tS, tN, tS2, mask};
    StreamIO io;
    io.read = reader; io.read_user = reader_user; io.write_v = writer; io.write_user = writer_user;
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
    if (!h || !out2) return ctk_set_error(CTK_E_INVALID, "null argument");
    out2[0] = h->gr_form; out2[1] = h->gr_grid;
    return CTK_OK;
}

// test hook / experiments (tools/reversal_probe.py) for the following k_reversal launches on this handle: the xcd_chunk mode (0 launch
// order, 1 eighths, n > 1 tiles of n workgroups; -1: the rule of ctk_reversal_plan) and a lower cap on the workgroups of a launch, so
// that a small case walks the stride loop (0: CTK_LEVEL_GRID_MAX)
extern "C" int ctk_debug_set_reversal(ctk_handle *h, int xcd_mode, int64_t grid_max)
{
    if (!h || xcd_mode < -1 || grid_max < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_reversal: bad argument");
    h->gr_xcd_dbg = xcd_mode;
    h->gr_grid_dbg = grid_max;
    return CTK_OK;
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
    ReversalTab tab = {};
    if (eq) CTKCHK(reversal_table(h, ny, a, tab));
    const int64_t n16 = steps * (int64_t)ny * nx * (is_f64 ? 8 : 4) / 16;
    const int64_t cblocks = (n16 + 255) / 256;
    const unsigned cgrid = (unsigned)std::min<int64_t>(std::max<int64_t>(cblocks, 1), CTK_LEVEL_GRID_MAX);
    const int cxcd = h->gr_xcd_dbg >= 0 ? h->gr_xcd_dbg : (cgrid >= CTK_LEVEL_XCD_MIN ? 1 : 0);
    return time_launches(h, "ctk_debug_time_reversal", reps, ms2, [&]() -> int {
        if (!eq) {
            k_reversal_copy<<<cgrid, 256, 0, h->stream>>>((const i32x4 *)x_dev, (i32x4 *)out_dev, n16, cxcd);
            HIPCHK(hipGetLastError());
            return CTK_OK;
        }
        return is_f64 ? launch_reversal<double>(h, (const double *)x_dev, ny, nx, steps, tab, eq2 != nullptr, mask != 0, (double *)out_dev)
                      : launch_reversal<float>(h, (const float *)x_dev, ny, nx, steps, tab, eq2 != nullptr, mask != 0, (float *)out_dev);
    });
}
