// ctk_band.hip -- the reductions over SPACE per time step (included by ctk_api.hip): what a time-longitude (Hovmoeller) diagram of a
// latitude band and a blocked-area series of a longitude sector are made of.  On the int32 flag slab (T, ny, nx), a band of rows
// [y0, y1), float64 row weights w[ny] -- the class passes the float32 area weights of the reference's life cycle, contrack.py:846-848,
// whose sum over a contour is its `Size`, contrack.py:874 -- and optionally a field x of the same shape, per step t and column c:
//     cnt[t][c]  = #{y in [y0, y1) : flag[t][y][c] > above}                                                             (uint32)
//     area[t][c] = from +0.0, for y = y0 .. y1 - 1 RISING:  s = s + (flag[t][y][c] > above ? w[y] : 0.0)                (float64)
//     wx[t][c]   = the same walk with  w[y] * (double)x[t][y][c]  -- the product rounded to float64, then added          (float64)
// and per sector (x0, len) -- the columns x0, x0 + 1, ... modulo nx -- the column values added in that column order from +0.0 (the
// counts: summed).  A sum that starts at +0.0 never becomes -0.0, so adding +0.0 for an unflagged pixel and adding nothing are the same
// bits; a value of x at an unflagged pixel is never loaded.  tests/band_util.py is the numpy statement.
//
// k_band: a thread owns 4 neighbouring columns of one step for ALL rows of the band: the latitude walk is the only ordered part, so
// (step, column quad) pairs are the parallelism -- T * nx / 4 threads -- and no sum is ever split or added atomically: that is what
// makes the result the same bits whatever the form or the chunking.  A wave reads 1 KiB of neighbouring columns per row; the loads
// of a batch of rows are in flight together before the first add (ctk_band_plan, ctk_forms.h: 8 rows, the rest of the band in ever
// shorter batches).  Two forms: 16-byte nontemporal loads when nx % 4 == 0 and the flag pointer is 16-byte aligned (the slab is read
// once, as in k_freq), four int32 loads with the columns beyond the row padded with INT_MIN -- never > above -- otherwise.  w[y] is
// the same for the whole grid: read through the constant address space it is a scalar load.  The field is read UNDER the flag test,
// as k_composite reads it: only the lanes whose flag passed ask for it.
//
// k_band_sect: one thread per (step, sector) walks its columns of the chunk's column tables in order, 8 loads ahead of the adds.  The
// tables are a few MB that k_band has just written, and 1 / (y1 - y0) of what it read.
#pragma once

typedef const __attribute__((address_space(4))) double ctk_const_f64;       // a wave-uniform index into it is an s_load

// rows y .. y + U - 1 of one thread's quad: all U flag loads, then the field loads of the pixels that passed, then the sums in rising y
template <typename VT, bool FIELD, bool VEC, int U>
__device__ __forceinline__ void band_batch(const int32_t *__restrict__ fp, const VT *__restrict__ xp, int64_t nx, int ncol, int y, ctk_const_f64 *w, int32_t above,
                                           uint32_t (&c)[4], double (&a)[4], double (&s)[4])
{
    ctk_i32x4 f[U];
    VT v[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int32_t *p = fp + (int64_t)(y + u) * nx;
        if (VEC) f[u] = __builtin_nontemporal_load((const ctk_i32x4 *)p);
        else {
            f[u].x = p[0];
            f[u].y = ncol > 1 ? p[1] : INT32_MIN;
            f[u].z = ncol > 2 ? p[2] : INT32_MIN;
            f[u].w = ncol > 3 ? p[3] : INT32_MIN;
        }
    }
    if (FIELD) {
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (f[u][k] > above) v[u][k] = xp[(int64_t)(y + u) * nx + k];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const double wy = w[y + u];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool on = f[u][k] > above;
            c[k] += on;
            a[k] = a[k] + (on ? wy : 0.0);
            if (FIELD) {
                if (on) s[k] = s[k] + wy * (double)v[u][k];              // (-ffp-contract=off: the product is rounded, then added)
            }
        }
    }
}

// flag, x: (T, ny, nx); thread i of T * nq takes step i / nq and the columns 4 * (i % nq) ...; umax: the widest batch of rows (a power
// of two, at most CTK_BAND_ROWS_MAX).  cnt / area / wx: (T, nx)
template <typename VT, bool FIELD, bool VEC>
__global__ __launch_bounds__(CTK_BAND_THREADS) CTK_SGPR_8WAVES void k_band(const int32_t *__restrict__ flag, const VT *__restrict__ x, int64_t T, int ny, int nx, int64_t nq,
                                                                          int y0, int y1, const double *__restrict__ w_ptr, int32_t above, int umax,
                                                                          uint32_t *__restrict__ cnt, double *__restrict__ area, double *__restrict__ wx)
{
    const int64_t i = (int64_t)blockIdx.x * CTK_BAND_THREADS + threadIdx.x;          // (64-bit: more than 2^32 elements)
    if (i >= T * nq) return;
    const int64_t t = i / nq;
    const int c0 = (int)(i - t * nq) * 4;
    const int ncol = min(4, nx - c0);
    ctk_const_f64 *w = (ctk_const_f64 *)w_ptr;
    const int64_t at = t * (int64_t)ny * nx + c0;
    const int32_t *fp = flag + at;
    const VT *xp = FIELD ? x + at : nullptr;
    uint32_t c[4] = {0, 0, 0, 0};
    double a[4] = {0.0, 0.0, 0.0, 0.0}, s[4] = {0.0, 0.0, 0.0, 0.0};
    int y = y0;
#define CTK_BAND_BATCH(U) band_batch<VT, FIELD, VEC, U>(fp, xp, nx, ncol, y, w, above, c, a, s)
    for (; umax >= 16 && y + 16 <= y1; y += 16) CTK_BAND_BATCH(16);
    for (; umax >= 8 && y + 8 <= y1; y += 8) CTK_BAND_BATCH(8);
    for (; umax >= 4 && y + 4 <= y1; y += 4) CTK_BAND_BATCH(4);
    for (; umax >= 2 && y + 2 <= y1; y += 2) CTK_BAND_BATCH(2);
    for (; y < y1; y++) CTK_BAND_BATCH(1);
#undef CTK_BAND_BATCH
    const int64_t o = t * nx + c0;
    for (int k = 0; k < ncol; k++) {
        cnt[o + k] = c[k];
        area[o + k] = a[k];
        if (FIELD) wx[o + k] = s[k];
    }
}

// the column tables (T, nx) -> the sector tables (T, nsect); sect: nsect pairs (x0, len).  wx / swx nullptr: no field
__global__ __launch_bounds__(CTK_BAND_THREADS) void k_band_sect(const uint32_t *__restrict__ cnt, const double *__restrict__ area, const double *__restrict__ wx, int64_t T,
                                                               int nx, const int32_t *__restrict__ sect, int nsect, uint32_t *__restrict__ scnt,
                                                               double *__restrict__ sarea, double *__restrict__ swx)
{
    const int64_t i = (int64_t)blockIdx.x * CTK_BAND_THREADS + threadIdx.x;
    if (i >= T * nsect) return;
    const int64_t t = i / nsect;
    const int sct = (int)(i - t * nsect);
    const int len = sect[2 * sct + 1];
    int col = sect[2 * sct];
    const uint32_t *cp = cnt + t * nx;
    const double *ap = area + t * nx, *xp = wx ? wx + t * nx : nullptr;
    uint32_t n = 0;
    double a = 0.0, s = 0.0;
    constexpr int U = 8;
    int k = 0;
    for (; k + U <= len; k += U) {
        uint32_t cv[U];
        double av[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            cv[u] = cp[col]; av[u] = ap[col]; xv[u] = xp ? xp[col] : 0.0;
            col = col + 1 == nx ? 0 : col + 1;
        }
#pragma unroll
        for (int u = 0; u < U; u++) { n += cv[u]; a = a + av[u]; s = s + xv[u]; }
    }
    for (; k < len; k++) {
        n += cp[col]; a = a + ap[col];
        if (xp) s = s + xp[col];
        col = col + 1 == nx ? 0 : col + 1;
    }
    scnt[i] = n; sarea[i] = a;
    if (swx) swx[i] = s;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// where the tables of one launch go (device pointers; wx / sec_wx only with a field, sec_* only with sectors)
struct BandDev { uint32_t *cnt; double *area, *wx; uint32_t *sec_cnt; double *sec_area, *sec_wx; };

// handle, shape, band, weights, sectors and what is asked for; the handle's device is current afterwards
static int band_args_check(ctk_handle *h, const char *name, int64_t T, int ny, int nx, const ctk_band_spec *sp)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "%s: null handle", name);
    if (!sp) return ctk_set_error(CTK_E_INVALID, "%s: null spec", name);
    if (T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad shape (T=%lld ny=%d nx=%d)", name, (long long)T, ny, nx);
    if ((int64_t)ny * nx > 0xffffffffll)
        return ctk_set_error(CTK_E_RANGE, "%s: a plane of ny * nx = %lld pixels does not fit the uint32 counts (at most 2^32 - 1)", name, (long long)ny * nx);
    if (sp->y0 < 0 || sp->y0 >= sp->y1 || sp->y1 > ny) return ctk_set_error(CTK_E_INVALID, "%s: the band [%d, %d) is not inside the %d rows", name, sp->y0, sp->y1, ny);
    if (!sp->w) return ctk_set_error(CTK_E_INVALID, "%s: null weights", name);
    for (int y = 0; y < ny; y++)
        if (!std::isfinite(sp->w[y])) return ctk_set_error(CTK_E_INVALID, "%s: w[%d] is not finite", name, y);
    if (sp->nsect < 0) return ctk_set_error(CTK_E_INVALID, "%s: nsect=%d (at least 0)", name, sp->nsect);
    if (sp->nsect > 0 && !sp->sectors) return ctk_set_error(CTK_E_INVALID, "%s: sectors is NULL but nsect=%d", name, sp->nsect);
    for (int s = 0; s < sp->nsect; s++) {
        const int32_t x0 = sp->sectors[2 * s], len = sp->sectors[2 * s + 1];
        if (x0 < 0 || x0 >= nx || len < 1 || len > nx)
            return ctk_set_error(CTK_E_INVALID, "%s: sector %d = (x0=%d, len=%d) needs 0 <= x0 < %d and 1 <= len <= %d", name, s, x0, len, nx, nx);
    }
    if (!sp->columns && sp->nsect == 0) return ctk_set_error(CTK_E_INVALID, "%s: neither the column tables nor a sector is asked for", name);
    if (!ctk_band_fits(T, nx, sp->nsect))
        return ctk_set_error(CTK_E_RANGE, "%s: T=%lld steps of %d columns are too many for one launch", name, (long long)T, nx);
    HIPCHK(hipSetDevice(h->device));
    return CTK_OK;
}

// the output pointers that the request needs (host or device alike)
static int band_out_check(const char *name, const ctk_band_spec *sp, const ctk_band_out *out, bool field)
{
    if (!out) return ctk_set_error(CTK_E_INVALID, "%s: null output", name);
    if (sp->columns && (!out->cnt || !out->area || (field && !out->wx))) return ctk_set_error(CTK_E_INVALID, "%s: null buffer (column tables)", name);
    if (sp->nsect > 0 && (!out->sec_cnt || !out->sec_area || (field && !out->sec_wx))) return ctk_set_error(CTK_E_INVALID, "%s: null buffer (sector tables)", name);
    return CTK_OK;
}

// spec->resident: the anomaly slab ctk_anom_* left on this handle, if it is the one the caller means (shape, type and generation)
static int band_resident(ctk_handle *h, const char *name, const ctk_band_spec *sp, bool f64, int64_t T, int ny, int nx, const void **x_dev)
{
    *x_dev = h->an_slab.find(T, ny, nx, f64);
    if (!*x_dev)
        return ctk_set_error(CTK_E_STATE, "%s: the field is the resident anomaly slab, but none of this shape and type is resident (ctk_anom_* with keep_resident)", name);
    if (h->an_slab.gen != sp->resident_gen)
        return ctk_set_error(CTK_E_STATE, "%s: the resident anomaly slab is generation %llu, the call names the stale generation %llu", name,
                             (unsigned long long)h->an_slab.gen, (unsigned long long)sp->resident_gen);
    return CTK_OK;
}

// weights and sectors go to the device (bd_tab: ny doubles, then nsect pairs)
static int band_tables(ctk_handle *h, int ny, const ctk_band_spec *sp, const double **w_dev, const int32_t **sect_dev)
{
    const size_t wb = (size_t)ny * 8, sb = (size_t)sp->nsect * 8;
    CTKCHK(ensure(h, h->bd_tab, wb + std::max<size_t>(sb, 8)));
    HIPCHK(hipMemcpyAsync(h->bd_tab.p, sp->w, wb, hipMemcpyHostToDevice, h->stream));
    if (sb) HIPCHK(hipMemcpyAsync((char *)h->bd_tab.p + wb, sp->sectors, sb, hipMemcpyHostToDevice, h->stream));
    *w_dev = (const double *)h->bd_tab.p;
    *sect_dev = (const int32_t *)((char *)h->bd_tab.p + wb);
    return CTK_OK;
}

// k_band (and, with sectors, k_band_sect) over nt steps on the handle's stream; esz 0: no field
template <typename VT, bool FIELD>
static int launch_band_t(ctk_handle *h, const int32_t *flag_dev, const VT *x_dev, int64_t nt, int ny, int nx, const ctk_band_spec *sp, const double *w_dev,
                         const BandDev &o)
{
    const CtkBandPlan pl = ctk_band_plan(nt, nx, ((uintptr_t)flag_dev & 15) == 0, h->bd_form_dbg, h->bd_rows_dbg);
    h->bd_form = pl.vec ? 0 : 1; h->bd_rows = pl.rows; h->bd_grid = pl.grid;
#define CTK_BAND_LAUNCH(V) \
    k_band<VT, FIELD, V><<<pl.grid, CTK_BAND_THREADS, 0, h->stream>>>(flag_dev, x_dev, nt, ny, nx, pl.quads, sp->y0, sp->y1, w_dev, sp->above, pl.rows, o.cnt, o.area, o.wx)
    if (pl.vec) CTK_BAND_LAUNCH(true); else CTK_BAND_LAUNCH(false);
#undef CTK_BAND_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}
static int launch_band(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int esz, int64_t nt, int ny, int nx, const ctk_band_spec *sp, const double *w_dev,
                       const int32_t *sect_dev, const BandDev &o)
{
    if (esz == 8) CTKCHK((launch_band_t<double, true>(h, flag_dev, (const double *)x_dev, nt, ny, nx, sp, w_dev, o)));
    else if (esz == 4) CTKCHK((launch_band_t<float, true>(h, flag_dev, (const float *)x_dev, nt, ny, nx, sp, w_dev, o)));
    else CTKCHK((launch_band_t<float, false>(h, flag_dev, nullptr, nt, ny, nx, sp, w_dev, o)));
    if (sp->nsect > 0) {
        const int64_t n = nt * sp->nsect;
        k_band_sect<<<(unsigned)((n + CTK_BAND_THREADS - 1) / CTK_BAND_THREADS), CTK_BAND_THREADS, 0, h->stream>>>(o.cnt, o.area, esz ? o.wx : nullptr, nt, nx, sect_dev,
                                                                                                                  sp->nsect, o.sec_cnt, o.sec_area, esz ? o.sec_wx : nullptr);
        HIPCHK(hipGetLastError());
    }
    return CTK_OK;
}

// the handle's column tables for `steps` steps (bd_cols: counts, areas, weighted sums) and sector tables (bd_sec), as one BandDev;
// `which` of `sets` sets of them (the streamed entries fill one while the other leaves the device)
static int band_scratch(ctk_handle *h, int64_t steps, int nx, int nsect, bool cols, bool secs, BandDev *o, int which = 0, int sets = 1)
{
    if (cols) {
        const size_t n = (size_t)steps * nx, cb = (n * 4 + 7) & ~(size_t)7, one = cb + 2 * n * 8;
        CTKCHK(ensure(h, h->bd_cols, one * sets));
        char *p = (char *)h->bd_cols.p + one * which;
        o->cnt = (uint32_t *)p;
        o->area = (double *)(p + cb);
        o->wx = o->area + n;
    }
    if (secs && nsect > 0) {
        const size_t n = (size_t)steps * nsect, cb = (n * 4 + 7) & ~(size_t)7, one = cb + 2 * n * 8;
        CTKCHK(ensure(h, h->bd_sec, one * sets));
        char *p = (char *)h->bd_sec.p + one * which;
        o->sec_cnt = (uint32_t *)p;
        o->sec_area = (double *)(p + cb);
        o->sec_wx = o->sec_area + n;
    }
    return CTK_OK;
}

static int band_dev_prepare(ctk_handle *h, const char *name, const int32_t *flag_dev, const void **x_dev, int *esz, int64_t T, int ny, int nx, const ctk_band_spec *sp,
                            const ctk_band_out *out, const double **w_dev, const int32_t **sect_dev, BandDev *o)
{
    CTKCHK(band_args_check(h, name, T, ny, nx, sp));
    if (!flag_dev) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    const bool field = *x_dev != nullptr || sp->resident;
    if (field && *esz != 4 && *esz != 8) return ctk_set_error(CTK_E_INVALID, "%s: elem_bytes must be 4 (float32) or 8 (float64)", name);
    if (!field) *esz = 0;
    CTKCHK(band_out_check(name, sp, out, field));
    if (sp->resident) {
        if (*x_dev) return ctk_set_error(CTK_E_INVALID, "%s: a field is given and the resident anomaly slab is named as well", name);
        CTKCHK(band_resident(h, name, sp, *esz == 8, T, ny, nx, x_dev));
    }
    CTKCHK(band_tables(h, ny, sp, w_dev, sect_dev));
    *o = BandDev{out->cnt, out->area, out->wx, out->sec_cnt, out->sec_area, out->sec_wx};
    if (!sp->columns) CTKCHK(band_scratch(h, T, nx, 0, true, false, o));          // sectors only: the column tables stay in the handle
    return CTK_OK;
}

extern "C" int ctk_band_dev(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int elem_bytes, int64_t T, int ny, int nx, const ctk_band_spec *spec,
                            const ctk_band_out *out_dev)
{
    const double *w_dev = nullptr;
    const int32_t *sect_dev = nullptr;
    BandDev o;
    CTKCHK(band_dev_prepare(h, "ctk_band_dev", flag_dev, &x_dev, &elem_bytes, T, ny, nx, spec, out_dev, &w_dev, &sect_dev, &o));
    CTKCHK(launch_band(h, flag_dev, x_dev, elem_bytes, T, ny, nx, spec, w_dev, sect_dev, o));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

// the way out of the streamed entries: the tables of chunk k are copied from device set k & 1 into the pinned twin of that set on the
// handle's stream, behind the kernels that made them, and reach the caller's arrays when the set is needed again (chunk k + 2) or at
// the end -- no chunk waits for its results, and the host only moves tables that are 1 / (y1 - y0) of the input or less
struct BandPiece { void *dst; const void *dev; size_t pin_off, bytes; };
struct BandWayOut {
    ctk_handle *h;
    Event ev[2];
    std::vector<BandPiece> pend[2];
    double ms = 0;
    explicit BandWayOut(ctk_handle *hh) : h(hh) {}
    int init(size_t bytes_per_set)
    {
        for (Event &e : ev) HIPCHK(e.create(hipEventDisableTiming));
        if (h->bd_pin.grow(bytes_per_set, hipHostMallocDefault) != hipSuccess) return ctk_set_error(CTK_E_NOMEM, "pinned table buffer (%zu bytes)", bytes_per_set);
        return CTK_OK;
    }
    // the pieces of set b that are still on their way reach the caller's arrays
    int land(int b)
    {
        if (pend[b].empty()) return CTK_OK;
        const double d0 = now_ms();
        HIPCHK(hipEventSynchronize(ev[b]));
        for (const BandPiece &p : pend[b]) memcpy(p.dst, (const char *)h->bd_pin[b] + p.pin_off, p.bytes);
        pend[b].clear();
        ms += now_ms() - d0;
        return CTK_OK;
    }
    // queue the copies of set b's pieces behind the work on the handle's stream
    int send(int b, const std::vector<BandPiece> &pieces)
    {
        for (const BandPiece &p : pieces)
            HIPCHK(hipMemcpyAsync((char *)h->bd_pin[b] + p.pin_off, p.dev, p.bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipEventRecord(ev[b], h->stream));
        pend[b] = pieces;
        return CTK_OK;
    }
};

// host arrays or reader callbacks.  A field that travels is stream_in's first slab and the flags its second (as ctk_composite_*);
// otherwise the flags are the only slab.  The tables of chunk k are computed into one of two chunk-sized sets of the handle's buffers
// and go to row c0 of the result (BandWayOut); with sectors only, the column tables never leave the device.
static int band_stream_impl(ctk_handle *h, StreamIO &io, int esz, bool travels, int64_t T, int ny, int nx, const ctk_band_spec *sp, const ctk_band_out *out,
                            int64_t chunk_steps, const char *name)
{
    CTKCHK(band_args_check(h, name, T, ny, nx, sp));
    if (chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps=%lld", name, (long long)chunk_steps);
    const bool field = travels || sp->resident;
    if (field && esz != 4 && esz != 8) return ctk_set_error(CTK_E_INVALID, "%s: elem_bytes must be 4 (float32) or 8 (float64)", name);
    if (!field) esz = 0;
    CTKCHK(band_out_check(name, sp, out, field));
    if (travels && sp->resident) return ctk_set_error(CTK_E_INVALID, "%s: a field is given and the resident anomaly slab is named as well", name);
    const void *res_dev = nullptr;
    if (sp->resident) CTKCHK(band_resident(h, name, sp, esz == 8, T, ny, nx, &res_dev));
    const double *w_dev = nullptr;
    const int32_t *sect_dev = nullptr;
    CTKCHK(band_tables(h, ny, sp, &w_dev, &sect_dev));
    const int64_t npix = (int64_t)ny * nx;
    io.esz = travels ? (size_t)esz : 4;
    io.esz2 = travels ? 4 : 0;
    io.chunk = ctk_stream_chunk(chunk_steps, T, (size_t)npix * io.esz);
    BandDev o[2] = {};
    for (int b = 0; b < 2; b++) CTKCHK(band_scratch(h, io.chunk, nx, sp->nsect, true, true, &o[b], b, 2));
    // a set's pinned twin: the tables that leave, 20 bytes per (step, column) and per (step, sector) at the most
    const size_t ccap = sp->columns ? (size_t)io.chunk * nx : 0, scap = (size_t)io.chunk * sp->nsect;
    BandWayOut way(h);
    CTKCHK(way.init((ccap + scap) * 20 + 64));                           // (every piece starts at a multiple of 8)
    const double t0 = now_ms();
    CTKCHK(stream_consume(h, io, esz == 8, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        const int b = (int)((c0 / io.chunk) & 1);
        CTKCHK(way.land(b));                                                // (chunk k - 2 used this set)
        const int32_t *fl = travels ? (const int32_t *)io.dev2 : (const int32_t *)chunk;
        const void *xv = travels ? chunk : res_dev ? (const void *)((const char *)res_dev + (size_t)c0 * npix * esz) : nullptr;
        CTKCHK(launch_band(h, fl, xv, esz, nt, ny, nx, sp, w_dev, sect_dev, o[b]));
        std::vector<BandPiece> pieces;
        size_t off = 0;
        auto piece = [&](void *dst, const void *dev, size_t n, size_t at, size_t width) {
            pieces.push_back(BandPiece{(char *)dst + at * width, dev, off, n * width});
            off += (n * width + 7) & ~(size_t)7;
        };
        if (sp->columns) {
            const size_t n = (size_t)nt * nx, at = (size_t)c0 * nx;
            piece(out->cnt, o[b].cnt, n, at, 4);
            piece(out->area, o[b].area, n, at, 8);
            if (field) piece(out->wx, o[b].wx, n, at, 8);
        }
        if (sp->nsect > 0) {
            const size_t n = (size_t)nt * sp->nsect, at = (size_t)c0 * sp->nsect;
            piece(out->sec_cnt, o[b].sec_cnt, n, at, 4);
            piece(out->sec_area, o[b].sec_area, n, at, 8);
            if (field) piece(out->sec_wx, o[b].sec_wx, n, at, 8);
        }
        return way.send(b, pieces);
    }));
    const int64_t chunks = (T + io.chunk - 1) / io.chunk;
    for (int64_t k = std::max<int64_t>(chunks - 2, 0); k < chunks; k++) CTKCHK(way.land((int)(k & 1)));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_D2H] = way.ms; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

static int band_host_impl(ctk_handle *h, const int32_t *flag, const void *x, int esz, int64_t T, int ny, int nx, const ctk_band_spec *sp, const ctk_band_out *out,
                          int64_t chunk_steps, const char *name)
{
    if (h && !flag) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    StreamIO io;
    if (x) { io.host_in = x; io.host_in2 = flag; }
    else io.host_in = flag;
    return band_stream_impl(h, io, esz, x != nullptr, T, ny, nx, sp, out, chunk_steps, name);
}

extern "C" int ctk_band_f32(ctk_handle *h, const int32_t *flag, const float *x, int64_t T, int ny, int nx, const ctk_band_spec *spec, const ctk_band_out *out,
                            int64_t chunk_steps)
{
    return band_host_impl(h, flag, x, 4, T, ny, nx, spec, out, chunk_steps, "ctk_band_f32");
}
extern "C" int ctk_band_f64(ctk_handle *h, const int32_t *flag, const double *x, int64_t T, int ny, int nx, const ctk_band_spec *spec, const ctk_band_out *out,
                            int64_t chunk_steps)
{
    return band_host_impl(h, flag, x, 8, T, ny, nx, spec, out, chunk_steps, "ctk_band_f64");
}
extern "C" int ctk_band_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn flag_reader, void *flag_user, ctk_read_chunk_fn field_reader,
                           void *field_user, const ctk_band_spec *spec, const ctk_band_out *out, int64_t chunk_steps)
{
    if (h && !flag_reader) return ctk_set_error(CTK_E_INVALID, "ctk_band_cb: null flag reader");
    StreamIO io;
    if (field_reader) { io.read = field_reader; io.read_user = field_user; io.read2 = flag_reader; io.read2_user = flag_user; }
    else { io.read = flag_reader; io.read_user = flag_user; }
    return band_stream_impl(h, io, elem_bytes, field_reader != nullptr, T, ny, nx, spec, out, chunk_steps, "ctk_band_cb");
}

// what ctk_band_plan decides (host only: no handle, no GPU)
extern "C" int ctk_debug_band_plan(int64_t T, int nx, int aligned16, int form, int rows, int64_t *out4)
{
    if (!out4 || T < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_band_plan: bad arguments");
    const CtkBandPlan p = ctk_band_plan(T, nx, aligned16 != 0, form, rows);
    out4[0] = p.vec ? 0 : 1; out4[1] = p.rows; out4[2] = p.quads; out4[3] = p.grid;
    return CTK_OK;
}

// test hook for the following k_band launches on this handle: the form (0: 16-byte loads where the shape and the pointer allow them,
// 1: the general form; -1 the rule) and the widest batch of rows in flight (-1: the rule)
extern "C" int ctk_debug_set_band(ctk_handle *h, int form, int rows)
{
    if (!h || form < -1 || form > 1 || rows < -1 || rows == 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_band: null handle, form not -1 / 0 / 1 or rows not -1 / positive");
    h->bd_form_dbg = form; h->bd_rows_dbg = rows;
    return CTK_OK;
}

// out3 = { the form of the last k_band launch on this handle (0 vector, 1 general, -1 none yet), its widest batch of rows, its workgroups }
extern "C" int ctk_debug_band_launch(ctk_handle *h, int64_t *out3)
{
    if (!h || !out3) return ctk_set_error(CTK_E_INVALID, "ctk_debug_band_launch: null argument");
    out3[0] = h->bd_form; out3[1] = h->bd_rows; out3[2] = h->bd_grid;
    return CTK_OK;
}

// k_band (with sectors: and k_band_sect) alone between HIP events on the handle's stream (tools/band_probe.py): the arguments of
// ctk_band_dev; ms2 = {best, mean} per launch
extern "C" int ctk_debug_time_band(ctk_handle *h, const int32_t *flag_dev, const void *x_dev, int elem_bytes, int64_t T, int ny, int nx, const ctk_band_spec *spec,
                                   const ctk_band_out *out_dev, int reps, double *ms2)
{
    if (h && (!ms2 || reps < 1)) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_band: null buffer or reps < 1");
    const double *w_dev = nullptr;
    const int32_t *sect_dev = nullptr;
    BandDev o;
    CTKCHK(band_dev_prepare(h, "ctk_debug_time_band", flag_dev, &x_dev, &elem_bytes, T, ny, nx, spec, out_dev, &w_dev, &sect_dev, &o));
    return time_launches(h, "ctk_debug_time_band", reps, ms2, [&]() { return launch_band(h, flag_dev, x_dev, elem_bytes, T, ny, nx, spec, w_dev, sect_dev, o); });
}
