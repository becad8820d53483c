// ctk_anom_seg.hip -- the entries of calc_clim / calc_anom (row N2, ctk_anom.hip): one host slab (ctk_anom_*), over independent time
// segments, resident and streamed (included by ctk_api.hip).  The climatology is pooled over every timestep of a group whatever its
// segment.  The smoothing stays inside a segment: anom[t] is the mean over the centred window of `smooth` steps, each raw anomaly
// rounded to the slab's type and added in float64 in rising step order, only if that window lies inside t's segment, else NaN.
// ctk_anom_* is the same host path with no segments -- one, the whole axis: NaN where the window leaves the axis -- so it takes at
// most 2^31 - 1 steps, as every entry on a slab in HBM does (anom_seg_args).  It launches k_anom (ctk_anom.hip), which needs no
// segment test; sums and rounding places here are k_anom's, so one segment gives ctk_anom_*'s bits.
//
// k_anom_ring: one thread per pixel and tile of output steps.  The thread walks the steps its tile needs once (tile + smooth - 1 of
// them), computes each raw anomaly x[j] - clim[group[j]] once and keeps the last `smooth` of them in a ring in LDS (slot k of lane l at
// ring[k * 256 + l]: consecutive lanes, consecutive banks); every output re-adds the ring from its oldest slot, which is k_anom's
// order of additions.  x, group and clim are read once per step and tile instead of `smooth` times per output.  k_anom_plain is
// k_anom with the segment test, for a smoothing whose ring does not fit (ctk_anom_plan, ctk_forms.h).
// Both take the slab as a window: plane 0 of `x` is step xbase, steps [xlo, xhi) of it may be read; plane 0 of `out` is step o0.  The
// resident entry passes the whole slab, the streamed entry a chunk with the smooth - 1 steps before it.
//
// Streamed (ctk_anom_stream_*): pass 1 adds each chunk into float64 sums and int32 counts per (group, pixel) kept in HBM (k_clim_acc;
// a group's steps arrive in rising t and are added in that order: k_clim_raw's bits), k_clim_fin turns them into the raw group
// means, k_clim_roll runs on them unchanged.  Pass 2 streams the chunks again through two windows of chunk + smooth - 1 steps; the
// last smooth - 1 steps of a window are copied in front of the next one on the device, so the reader is never asked for a step twice
// in a pass.  Output lags input by (smooth - 1) / 2 steps; the last chunk closes the gap.
#pragma once

template <typename VT>
__global__ __launch_bounds__(CTK_ANOM_THREADS) void k_anom_ring(const VT *__restrict__ x, int64_t xbase, int64_t xlo, int64_t xhi, const VT *__restrict__ clim,
                                                                const int32_t *__restrict__ group, const uint8_t *__restrict__ valid, int64_t npix, int smooth,
                                                                int64_t o0, int64_t o1, int64_t tile, VT *__restrict__ out)
{
    extern __shared__ __align__(16) unsigned char an_ring_lds[];
    VT *ring = (VT *)an_ring_lds + threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * CTK_ANOM_THREADS + threadIdx.x;
    if (p >= npix) return;                                                       // (no barrier below: a lane's ring is its own)
    const int64_t t0 = o0 + (int64_t)blockIdx.y * tile, t1 = min(o1, t0 + tile);
    const int back = smooth / 2, fwd = (smooth - 1) / 2;
    int slot = 0;
#pragma unroll 4
    for (int64_t j = t0 - back; j < t1 + fwd; j++) {
        if (j >= xlo && j < xhi)                                                 // (a step outside is in no valid window)
            ring[slot * CTK_ANOM_THREADS] = (VT)((double)x[(j - xbase) * npix + p] - (double)clim[(int64_t)group[j] * npix + p]);
        const int next = slot + 1 == smooth ? 0 : slot + 1;                       // the oldest slot: step j - (smooth - 1)
        const int64_t t = j - fwd;
        if (t >= t0) {
            VT r = (VT)__builtin_nanf("");
            if (valid[t]) {
                double s = 0.0;
                int k = next;
                for (int i = 0; i < smooth; i++) { s += (double)ring[k * CTK_ANOM_THREADS]; k = k + 1 == smooth ? 0 : k + 1; }
                r = (VT)(s / smooth);
            }
            out[(t - o0) * npix + p] = r;
        }
        slot = next;
    }
}

template <typename VT>
__global__ __launch_bounds__(CTK_ANOM_THREADS) void k_anom_plain(const VT *__restrict__ x, int64_t xbase, int64_t xlo, int64_t xhi, const VT *__restrict__ clim,
                                                                 const int32_t *__restrict__ group, const uint8_t *__restrict__ valid, int64_t npix, int smooth,
                                                                 int64_t o0, int64_t o1, int64_t tile, VT *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * CTK_ANOM_THREADS + threadIdx.x;
    if (p >= npix) return;
    const int64_t t0 = o0 + (int64_t)blockIdx.y * tile, t1 = min(o1, t0 + tile);
    for (int64_t t = t0; t < t1; t++) {
        const int64_t lo = t - smooth / 2, hi = t + (smooth - 1) / 2;
        VT r = (VT)__builtin_nanf("");
        if (valid[t] && lo >= xlo && hi < xhi) {
            double s = 0.0;
            for (int64_t j = lo; j <= hi; j++) s += (double)(VT)((double)x[(j - xbase) * npix + p] - (double)clim[(int64_t)group[j] * npix + p]);
            r = (VT)(s / smooth);
        }
        out[(t - o0) * npix + p] = r;
    }
}

// sums / counts of the groups += the nt steps of a chunk (group: the chunk's ids).  Workgroup row y takes the groups g with
// g % gridDim.y == y and walks the chunk in time order: the running sum of the group it is in stays in registers and goes back to HBM
// when the group changes, so every (group, pixel) sum sees its steps in rising t, one addition each, as k_clim_raw's loop
template <typename VT>
__global__ __launch_bounds__(256) void k_clim_acc(const VT *__restrict__ x, const int32_t *__restrict__ group, int64_t nt, int64_t npix, double *__restrict__ sums,
                                                  int32_t *__restrict__ counts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    int cur = -1, c = 0;
    double s = 0.0;
    for (int64_t t = 0; t < nt; t++) {
        const int g = group[t];
        if (g % (int)gridDim.y != (int)blockIdx.y) continue;
        if (g != cur) {
            if (cur >= 0) { sums[(int64_t)cur * npix + p] = s; counts[(int64_t)cur * npix + p] = c; }
            cur = g;
            s = sums[(int64_t)g * npix + p]; c = counts[(int64_t)g * npix + p];
        }
        const VT v = x[t * npix + p];
        if (!an_isnan(v)) { s += (double)v; c++; }
    }
    if (cur >= 0) { sums[(int64_t)cur * npix + p] = s; counts[(int64_t)cur * npix + p] = c; }
}

// raw[g][p] = the group mean of the sums (k_clim_raw's last line)
template <typename VT>
__global__ __launch_bounds__(256) void k_clim_fin(const double *__restrict__ sums, const int32_t *__restrict__ counts, int64_t n, VT *__restrict__ raw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = counts[i];
    raw[i] = c ? (VT)(sums[i] / c) : (VT)__builtin_nanf("");
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// valid[t] = the centred window of `smooth` steps around t lies inside t's segment (starts checked; none: one segment)
static void anom_window_valid(const int64_t *starts, int64_t nseg, int64_t T, int smooth, std::vector<uint8_t> &valid)
{
    valid.assign((size_t)T, 0);
    const int64_t one = 0;
    if (nseg < 1) { starts = &one; nseg = 1; }
    for (int64_t k = 0; k < nseg; k++) {
        const int64_t s = starts[k], e = k + 1 < nseg ? starts[k + 1] : T;
        for (int64_t t = s + smooth / 2; t + (smooth - 1) / 2 < e; t++) valid[(size_t)t] = 1;
    }
}

static int anom_seg_check(const char *who, const void *h, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                          const int64_t *starts, int64_t nseg)
{
    if (!h || !group || T < 1 || ny < 1 || nx < 1 || ngroups < 1 || window < 1 || smooth < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments", who);
    for (int64_t t = 0; t < T; t++)
        if (group[t] < 0 || group[t] >= ngroups) return ctk_set_error(CTK_E_INVALID, "%s: group[%lld] = %d outside 0..%d", who, (long long)t, group[t], ngroups - 1);
    return segment_starts_check(who, starts, nseg, T);
}

// the arguments of the resident entries (the slab lies in HBM: T counts planes of an int32 index)
static int anom_seg_args(const char *who, const void *h, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                         const int64_t *starts, int64_t nseg)
{
    CTKCHK(anom_seg_check(who, h, T, ny, nx, group, ngroups, window, smooth, starts, nseg));
    if (T > 0x7fffffffll) return ctk_set_error(CTK_E_INVALID, "%s: T=%lld timesteps (at most 2^31 - 1)", who, (long long)T);
    return CTK_OK;
}

// anomalies of the output steps [o0, o1) on the handle's stream (the window arguments: see the kernels)
template <typename VT>
static int launch_anom_seg(ctk_handle *h, const VT *x, int64_t xbase, int64_t xlo, int64_t xhi, const VT *clim, const int32_t *group_dev, const uint8_t *valid_dev,
                           int64_t npix, int smooth, int64_t o0, int64_t o1, VT *out)
{
    const CtkAnomPlan pl = ctk_anom_plan((int)sizeof(VT), smooth, o1 - o0, npix, h->an_waves_dbg > 0 ? h->an_waves_dbg : CTK_ANOM_WAVES,
                                         h->an_gy_dbg > 0 ? std::min<int64_t>(h->an_gy_dbg, 65535) : 65535);
    h->an_form = pl.form;
    h->an_last[0] = pl.tile; h->an_last[1] = pl.gx; h->an_last[2] = pl.gy; h->an_last[3] = (int64_t)pl.lds; h->an_last[4] = o0; h->an_last[5] = o1;
    h->an_launches++;
    const dim3 grid(pl.gx, pl.gy);
    if (pl.form == CTK_ANOM_RING)
        k_anom_ring<VT><<<grid, CTK_ANOM_THREADS, pl.lds, h->stream>>>(x, xbase, xlo, xhi, clim, group_dev, valid_dev, npix, smooth, o0, o1, pl.tile, out);
    else
        k_anom_plain<VT><<<grid, CTK_ANOM_THREADS, 0, h->stream>>>(x, xbase, xlo, xhi, clim, group_dev, valid_dev, npix, smooth, o0, o1, pl.tile, out);
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// climatology and anomalies of a slab in device memory: the uploaded copy of a host slab (anom_seg_impl), or the resident vertical
// mean (ctk_anom_seg_resident, ctk_level.hip); the caller has checked the arguments (anom_seg_args).  whole_axis: ctk_anom_* -- no
// segments are given and the anomalies come from k_anom (ctk_anom.hip) instead of the planned form
template <typename VT>
static int anom_seg_dev(ctk_handle *h, const VT *x_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                        const VT *clim_in, VT *anom_out, VT *clim_out, int keep_resident, const int64_t *starts, int64_t nseg, bool whole_axis = false)
{
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    if (!whole_axis) h->an_launches = 0;                               // (ctk_anom_* leaves what ctk_debug_anom_launch reports alone)
    const int64_t npix = (int64_t)ny * nx;
    const size_t esz = sizeof(VT), n = (size_t)T * (size_t)npix, cb = (size_t)ngroups * npix * esz;
    CTKCHK(ensure(h, h->an_clim, cb));
    h->an_pct_n = -1;                                                  // (an_raw is overwritten below)
    CTKCHK(ensure(h, h->an_raw, cb));
    CTKCHK(ensure(h, h->an_idx, ((size_t)2 * T + ngroups + 2) * 4));
    CTKCHK(ensure(h, h->an_valid, (size_t)T));
    std::vector<int32_t> idx((size_t)2 * T + ngroups + 1);
    int32_t *tlist = idx.data(), *goff = tlist + T, *grp = goff + ngroups + 1;
    steps_by_group(group, T, ngroups, tlist, goff);
    memcpy(grp, group, (size_t)T * 4);
    HIPCHK(hipMemcpy(h->an_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    const int32_t *d_tlist = P<int32_t>(h->an_idx), *d_goff = d_tlist + T, *d_grp = d_goff + ngroups + 1;
    const unsigned gx = (unsigned)((npix + 255) / 256);
    if (clim_in) {
        HIPCHK(hipMemcpy(h->an_clim.p, clim_in, cb, hipMemcpyHostToDevice));
    } else {
        k_clim_raw<VT><<<dim3(gx, (unsigned)ngroups), 256, 0, s>>>(x_dev, d_tlist, d_goff, npix, (VT *)h->an_raw.p);
        k_clim_roll<VT><<<dim3(gx, (unsigned)std::min(ngroups, 64)), 256, 0, s>>>((const VT *)h->an_raw.p, ngroups, window, npix, (VT *)h->an_clim.p);
        HIPCHK(hipGetLastError());
    }
    if (clim_out) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipMemcpy(clim_out, h->an_clim.p, cb, hipMemcpyDeviceToHost)); }
    if (anom_out || keep_resident) {
        DevBuf &out = h->an_slab.buf;
        h->an_slab.drop();                                             // the resident slab (if any) is being overwritten
        CTKCHK(ensure(h, out, n * esz));                               // (only here: a climatology-only call leaves the slab alone)
        if (whole_axis) {                                              // (0.7 % ahead of the ring form at smooth 1 on 0.25 degree planes: profiles/NOTES.md)
            const int tseg = 32;
            k_anom<VT><<<dim3(gx, (unsigned)((T + tseg - 1) / tseg)), 256, 0, s>>>(x_dev, (const VT *)h->an_clim.p, d_grp, T, npix, smooth, tseg, (VT *)out.p);
            HIPCHK(hipGetLastError());
        } else {
            std::vector<uint8_t> valid;
            anom_window_valid(starts, nseg, T, smooth, valid);
            HIPCHK(hipMemcpy(h->an_valid.p, valid.data(), (size_t)T, hipMemcpyHostToDevice));
            CTKCHK(launch_anom_seg<VT>(h, x_dev, 0, 0, T, (const VT *)h->an_clim.p, d_grp, P<uint8_t>(h->an_valid), npix, smooth, 0, T, (VT *)out.p));
        }
        HIPCHK(hipStreamSynchronize(s));
        if (keep_resident) h->an_slab.keep(T, ny, nx, sizeof(VT) == 8);
        if (anom_out) CTKCHK(download(h, out.p, anom_out, n * esz));
    }
    return CTK_OK;
}

// a host slab: uploaded into io_in, then anom_seg_dev.  who: the entry, as its messages name it
template <typename VT>
static int anom_seg_impl(const char *who, ctk_handle *h, const VT *x_host, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                         const VT *clim_in, VT *anom_out, VT *clim_out, int keep_resident, const int64_t *starts, int64_t nseg, bool whole_axis = false)
{
    if (h && (!x_host || (!anom_out && !clim_out && !keep_resident))) return ctk_set_error(CTK_E_INVALID, "%s: bad arguments", who);
    CTKCHK(anom_seg_args(who, h, T, ny, nx, group, ngroups, window, smooth, starts, nseg));
    HIPCHK(hipSetDevice(h->device));
    const size_t bytes = (size_t)T * (size_t)ny * (size_t)nx * sizeof(VT);
    CTKCHK(claim_io(h, h->io_in, bytes));
    HIPCHK(hipMemcpy(h->io_in.p, x_host, bytes, hipMemcpyHostToDevice));
    return anom_seg_dev<VT>(h, (const VT *)h->io_in.p, T, ny, nx, group, ngroups, window, smooth, clim_in, anom_out, clim_out, keep_resident, starts, nseg, whole_axis);
}

// ctk_anom_*: no segments (one, the whole axis).  T above 2^31 - 1 is refused (anom_seg_args): the step lists are int32
extern "C" int ctk_anom_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                            const float *clim_in, float *anom_out, float *clim_out, int keep_resident)
{
    return anom_seg_impl<float>("ctk_anom", h, x, T, ny, nx, group, ngroups, window, smooth, clim_in, anom_out, clim_out, keep_resident, nullptr, 0, true);
}
extern "C" int ctk_anom_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                            const double *clim_in, double *anom_out, double *clim_out, int keep_resident)
{
    return anom_seg_impl<double>("ctk_anom", h, x, T, ny, nx, group, ngroups, window, smooth, clim_in, anom_out, clim_out, keep_resident, nullptr, 0, true);
}
extern "C" int ctk_anom_seg_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                                const float *clim_in, float *anom_out, float *clim_out, int keep_resident, const int64_t *starts, int64_t nseg)
{
    return anom_seg_impl<float>("ctk_anom_seg", h, x, T, ny, nx, group, ngroups, window, smooth, clim_in, anom_out, clim_out, keep_resident, starts, nseg);
}
extern "C" int ctk_anom_seg_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                                const double *clim_in, double *anom_out, double *clim_out, int keep_resident, const int64_t *starts, int64_t nseg)
{
    return anom_seg_impl<double>("ctk_anom_seg", h, x, T, ny, nx, group, ngroups, window, smooth, clim_in, anom_out, clim_out, keep_resident, starts, nseg);
}

// test hook: the kernel form of the last ctk_anom_seg_* / ctk_anom_stream_* launch on this handle (CtkAnomForm; -1: none yet)
extern "C" int ctk_debug_anom_form(ctk_handle *h, int64_t *form)
{
    if (!h || !form) return ctk_set_error(CTK_E_INVALID, "null argument");
    *form = h->an_form;
    return CTK_OK;
}

// test hook for the following launch_anom_seg on this handle: ctk_anom_plan's waves_wanted and grid_y_max (0: the rule's CTK_ANOM_WAVES and
// 65535; grid_y_max above 65535 stays 65535), so that a small slab reaches the tile edges
extern "C" int ctk_debug_set_anom(ctk_handle *h, int64_t waves_wanted, int64_t grid_y_max)
{
    if (!h || waves_wanted < 0 || grid_y_max < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_anom: bad argument");
    h->an_waves_dbg = waves_wanted;
    h->an_gy_dbg = grid_y_max;
    return CTK_OK;
}

// what ctk_anom_plan decides (host only: no handle, no GPU); waves_wanted / grid_y_max as ctk_debug_set_anom; out5 = {form, lds, tile, gx, gy}
extern "C" int ctk_debug_anom_plan(int elem_bytes, int smooth, int64_t nt, int64_t npix, int64_t waves_wanted, int64_t grid_y_max, int64_t *out5)
{
    if (!out5 || (elem_bytes != 4 && elem_bytes != 8) || smooth < 1 || nt < 1 || npix < 1 || waves_wanted < 0 || grid_y_max < 0)
        return ctk_set_error(CTK_E_INVALID, "ctk_debug_anom_plan: bad arguments");
    const CtkAnomPlan p = ctk_anom_plan(elem_bytes, smooth, nt, npix, waves_wanted > 0 ? waves_wanted : CTK_ANOM_WAVES,
                                        grid_y_max > 0 ? std::min<int64_t>(grid_y_max, 65535) : 65535);
    out5[0] = p.form; out5[1] = (int64_t)p.lds; out5[2] = p.tile; out5[3] = p.gx; out5[4] = p.gy;
    return CTK_OK;
}

// test hook: out8 = {form, tile, gx, gy, lds, o0, o1} of the last launch_anom_seg on this handle (form -1: none yet) and the number of
// such launches the last ctk_anom_seg_* / ctk_anom_stream_* / ctk_anom_seg_resident call made
extern "C" int ctk_debug_anom_launch(ctk_handle *h, int64_t *out8)
{
    if (!h || !out8) return ctk_set_error(CTK_E_INVALID, "null argument");
    out8[0] = h->an_form; out8[1] = h->an_last[0]; out8[2] = h->an_last[1]; out8[3] = h->an_last[2]; out8[4] = h->an_last[3]; out8[5] = h->an_last[4];
    out8[6] = h->an_last[5]; out8[7] = h->an_launches;
    return CTK_OK;
}

// ---- streamed ------------------------------------------------------------------------------------------------------------------
template <typename VT>
static int anom_stream_impl(ctk_handle *h, StreamIO &io, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                            const int64_t *starts, int64_t nseg, const VT *clim_in, VT *clim_out, int64_t chunk_steps, const char *name)
{
    const bool sink = io.host_out_v || io.write_v;
    if (h && ((!io.host_in && !io.read) || (!sink && !clim_out) || chunk_steps < 0)) return ctk_set_error(CTK_E_INVALID, "%s: no source, nothing to produce or chunk_steps < 0", name);
    CTKCHK(anom_seg_check(name, h, T, ny, nx, group, ngroups, window, smooth, starts, nseg));
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->an_launches = 0;
    const int64_t npix = (int64_t)ny * nx;
    const size_t plane = (size_t)npix * sizeof(VT), cb = (size_t)ngroups * plane, ng = (size_t)ngroups * (size_t)npix;
    io.esz = sizeof(VT);
    io.chunk = ctk_stream_chunk(chunk_steps, T, plane, std::max<int64_t>(smooth - 1, 1));                 // (at least the halo: see pass 2)
    const double t_call = now_ms();
    CTKCHK(ensure(h, h->an_clim, cb));
    h->an_pct_n = -1;                                                  // (an_raw is overwritten below)
    CTKCHK(ensure(h, h->an_raw, cb));
    CTKCHK(ensure(h, h->an_idx, (size_t)T * 4));
    CTKCHK(stream_setup(h, (size_t)(io.chunk + smooth - 1) * plane, 0, io.read != nullptr));
    if (sink) CTKCHK(stream_setup(h, 0, (size_t)(io.chunk + smooth) * plane, io.write_v != nullptr));
    HIPCHK(hipMemcpy(h->an_idx.p, group, (size_t)T * 4, hipMemcpyHostToDevice));
    const int32_t *d_grp = P<int32_t>(h->an_idx);
    const unsigned gx = (unsigned)((npix + 255) / 256);
    if (clim_in) {
        HIPCHK(hipMemcpy(h->an_clim.p, clim_in, cb, hipMemcpyHostToDevice));
    } else {
        CTKCHK(ensure(h, h->an_acc, ng * 12));
        double *sums = P<double>(h->an_acc);
        int32_t *counts = (int32_t *)(sums + ng);
        HIPCHK(hipMemsetAsync(sums, 0, ng * 12, s));
        const unsigned gy = (unsigned)std::min(ngroups, 32);
        CTKCHK(stream_consume(h, io, sizeof(VT) == 8, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
            k_clim_acc<VT><<<dim3(gx, gy), 256, 0, s>>>((const VT *)chunk, d_grp + c0, nt, npix, sums, counts);
            HIPCHK(hipGetLastError());
            return CTK_OK;
        }));
        k_clim_fin<VT><<<(unsigned)((ng + 255) / 256), 256, 0, s>>>(sums, counts, (int64_t)ng, (VT *)h->an_raw.p);
        k_clim_roll<VT><<<dim3(gx, (unsigned)std::min(ngroups, 64)), 256, 0, s>>>((const VT *)h->an_raw.p, ngroups, window, npix, (VT *)h->an_clim.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));                               // (pass 2 reuses the chunk buffers)
    }
    if (clim_out) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipMemcpy(clim_out, h->an_clim.p, cb, hipMemcpyDeviceToHost)); }
    int rc = CTK_OK;
    if (sink) {
        std::vector<uint8_t> valid;
        anom_window_valid(starts, nseg, T, smooth, valid);
        CTKCHK(ensure(h, h->an_valid, (size_t)T));
        HIPCHK(hipMemcpy(h->an_valid.p, valid.data(), (size_t)T, hipMemcpyHostToDevice));
        // pass 2 (window_produce): windows of smooth - 1 kept steps and a chunk in io_in, two output buffers in io_out.  Complete
        // once the steps below `end` are there: the outputs whose window ends below it, and everything once the last chunk is there
        const int64_t fwd = (smooth - 1) / 2;
        rc = window_produce(
            h, io, T, smooth - 1, plane, name, [&](int64_t end, int64_t from) { return end >= T ? T : std::max(from, end - fwd); },
            [&](int b, int64_t) { return (char *)h->io_out.p + (size_t)b * (size_t)(io.chunk + smooth) * plane; },
            [&](const char *win, int64_t xbase, int64_t xlo, int64_t xhi, int64_t o0, int64_t o1, char *out) {
                return launch_anom_seg<VT>(h, (const VT *)win, xbase, xlo, xhi, (const VT *)h->an_clim.p, d_grp, P<uint8_t>(h->an_valid), npix, smooth, o0, o1, (VT *)out);
            });
    }
    return stream_produce_end(h, io, rc, t_call);
}

extern "C" int ctk_anom_stream_f32(ctk_handle *h, const float *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                                   const int64_t *starts, int64_t nseg, const float *clim_in, float *anom_out, float *clim_out, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = x; io.host_out_v = anom_out;
    return anom_stream_impl<float>(h, io, T, ny, nx, group, ngroups, window, smooth, starts, nseg, clim_in, clim_out, chunk_steps, "ctk_anom_stream_f32");
}
extern "C" int ctk_anom_stream_f64(ctk_handle *h, const double *x, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int window, int smooth,
                                   const int64_t *starts, int64_t nseg, const double *clim_in, double *anom_out, double *clim_out, int64_t chunk_steps)
{
    StreamIO io;
    io.host_in = x; io.host_out_v = anom_out;
    return anom_stream_impl<double>(h, io, T, ny, nx, group, ngroups, window, smooth, starts, nseg, clim_in, clim_out, chunk_steps, "ctk_anom_stream_f64");
}
extern "C" int ctk_anom_stream_cb(ctk_handle *h, int elem_bytes, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *group,
                                  int ngroups, int window, int smooth, const int64_t *starts, int64_t nseg, const void *clim_in, void *clim_out,
                                  ctk_write_values_fn writer, void *writer_user, int64_t chunk_steps)
{
    if (elem_bytes != 4 && elem_bytes != 8) return ctk_set_error(CTK_E_INVALID, "ctk_anom_stream_cb: elem_bytes must be 4 (float32) or 8 (float64)");
    if (h && !reader) return ctk_set_error(CTK_E_INVALID, "ctk_anom_stream_cb: null reader");
    StreamIO io;
    io.read = reader; io.read_user = reader_user; io.write_v = writer; io.write_user = writer_user;
    if (elem_bytes == 8)
        return anom_stream_impl<double>(h, io, T, ny, nx, group, ngroups, window, smooth, starts, nseg, (const double *)clim_in, (double *)clim_out, chunk_steps, "ctk_anom_stream_cb");
    return anom_stream_impl<float>(h, io, T, ny, nx, group, ngroups, window, smooth, starts, nseg, (const float *)clim_in, (float *)clim_out, chunk_steps, "ctk_anom_stream_cb");
}
