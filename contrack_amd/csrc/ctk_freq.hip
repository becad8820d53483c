// ctk_freq.hip -- the blocking-frequency climatology of the reference's tutorial on the device (included by ctk_api.hip):
//     xr.where(block['flag'] > 1, 1, 0).sum(dim='time') / block.ntime * 100                                    README.rst:159-160
// per group of timesteps (month, season ... -- or one group):
//     counts[g][p] = #{t : group[t] == g and flag[t][p] > above}
// The division is left to the caller (counts are exact integers; the percent in float64 is counts / n[g] * 100).
//
// k_freq: one thread per 4 consecutive pixels of the flattened plane and one slice of timesteps (blockIdx.y).  Nontemporal 16-byte
// loads when the plane and the pointer allow it (measured 2-9 % faster than plain ones on this once-read stream, profiles/NOTES.md),
// 4 int32 loads otherwise; the 4 counters stay in VGPRs and are flushed with one no-return
// atomicAdd per NONZERO counter when the group changes (groups need not be sorted in time: DJF wraps around the year) or the slice
// ends.  group[t] is the same for the whole workgroup: read through the constant address space it is a scalar load.  Most pixels
// are never flagged (frequencies are a few percent), so most flushes issue nothing.  The slice length sets how many waves run: a
// 1-degree plane is only 16 290 quads (255 waves), so T is split to fill the chip (profiles/NOTES.md: the sweep).
#pragma once

typedef const __attribute__((address_space(4))) int32_t ctk_const_i32;      // a wave-uniform index into it is an s_load
typedef int32_t ctk_i32x4 __attribute__((ext_vector_type(4)));

constexpr int kFreqUnroll = 8;               // timesteps whose loads are in flight together

template <bool VEC, bool GROUPED, bool NT>
__global__ __launch_bounds__(256) void k_freq(const int32_t *__restrict__ flag, int64_t T, int64_t npix, const int32_t *__restrict__ group_ptr,
                                              int32_t above, int64_t slice, uint32_t *__restrict__ counts)
{
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;          // first pixel of this thread's quad (64-bit: > 2^32 elements)
    if (p0 >= npix) return;
    const int64_t t0 = (int64_t)blockIdx.y * slice, t1 = min(T, t0 + slice);
    ctk_const_i32 *group = (ctk_const_i32 *)group_ptr;
    auto load = [&](int64_t t) -> ctk_i32x4 {
        const int32_t *a = flag + t * npix + p0;
        if (VEC) return NT ? __builtin_nontemporal_load((const ctk_i32x4 *)a) : *(const ctk_i32x4 *)a;
        // general path (ny * nx % 4 != 0 or an unaligned pointer): pixels beyond the plane read as INT_MIN, which is never > above
        ctk_i32x4 v;
        v.x = a[0];
        v.y = p0 + 1 < npix ? a[1] : INT32_MIN;
        v.z = p0 + 2 < npix ? a[2] : INT32_MIN;
        v.w = p0 + 3 < npix ? a[3] : INT32_MIN;
        return v;
    };
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    int g = GROUPED ? group[t0] : 0;
    auto flush = [&]() {                                                        // (a counter of a pixel beyond the plane stays 0)
        uint32_t *dst = counts + (int64_t)g * npix + p0;
        if (c0) atomicAdd(dst, c0);
        if (c1) atomicAdd(dst + 1, c1);
        if (c2) atomicAdd(dst + 2, c2);
        if (c3) atomicAdd(dst + 3, c3);
        c0 = c1 = c2 = c3 = 0;
    };
    auto count = [&](int64_t t, const ctk_i32x4 &v) {
        if (GROUPED) {
            const int gt = group[t];
            if (gt != g) { flush(); g = gt; }
        }
        c0 += v.x > above; c1 += v.y > above; c2 += v.z > above; c3 += v.w > above;
    };
    int64_t t = t0;
    for (; t + kFreqUnroll <= t1; t += kFreqUnroll) {
        ctk_i32x4 v[kFreqUnroll];
#pragma unroll
        for (int u = 0; u < kFreqUnroll; u++) v[u] = load(t + u);
#pragma unroll
        for (int u = 0; u < kFreqUnroll; u++) count(t + u, v[u]);
    }
    for (; t < t1; t++) count(t, load(t));
    flush();
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
constexpr int64_t kSliceMax = 64;            // timesteps per slice of k_freq and k_spell once the chip is full (profiles/NOTES.md: the sweeps)
constexpr int64_t kSliceWaves = 16384;       // waves that fill 256 CUs several times over
constexpr int64_t kFreqSliceMin = 8;

// counts += k_freq(flag[0..T)) on the handle's stream; group_dev: T device ints (nullptr: one group)
static int launch_freq(ctk_handle *h, const int32_t *flag_dev, int64_t T, int64_t npix, const int32_t *group_dev, int32_t above, uint32_t *counts_dev)
{
    const int64_t slice = ctk_time_slice(h->fq_slice_dbg, T, npix, kFreqSliceMin, kSliceMax, kSliceWaves);
    const int64_t bx = ((npix + 3) / 4 + 255) / 256;
    if (bx > 0x7fffffffll) return ctk_set_error(CTK_E_RANGE, "ctk_frequency: a plane of %lld pixels is too large", (long long)npix);
    const dim3 grid((unsigned)bx, (unsigned)((T + slice - 1) / slice));
    const bool vec = npix % 4 == 0 && ((uintptr_t)flag_dev & 15) == 0, nt = h->fq_nt != 0;            // (-1: the default, nontemporal)
#define CTK_FREQ_LAUNCH(V, G, N) k_freq<V, G, N><<<grid, 256, 0, h->stream>>>(flag_dev, T, npix, group_dev, above, slice, counts_dev)
    if (vec) {
        if (group_dev) { if (nt) CTK_FREQ_LAUNCH(true, true, true); else CTK_FREQ_LAUNCH(true, true, false); }
        else           { if (nt) CTK_FREQ_LAUNCH(true, false, true); else CTK_FREQ_LAUNCH(true, false, false); }
    } else {
        if (group_dev) CTK_FREQ_LAUNCH(false, true, false);
        else           CTK_FREQ_LAUNCH(false, false, false);
    }
#undef CTK_FREQ_LAUNCH
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// the arguments every grouped map over a slab shares (frequency, composite, spells): handle, shape, T within the uint32 maps, group ids
// in [0, ngroups); the handle's device is current afterwards
static int group_args_check(ctk_handle *h, const char *name, int64_t T, int ny, int nx, const int32_t *group, int ngroups)
{
    if (!h) return ctk_set_error(CTK_E_INVALID, "%s: null handle", name);
    if (T < 1 || ny < 1 || nx < 1) return ctk_set_error(CTK_E_INVALID, "%s: bad shape (T=%lld ny=%d nx=%d)", name, (long long)T, ny, nx);
    if (T > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "%s: T=%lld timesteps do not fit the uint32 counts (at most 2^32 - 1)", name, (long long)T);
    if (ngroups < 1) return ctk_set_error(CTK_E_INVALID, "%s: ngroups=%d (at least 1)", name, ngroups);
    if (!group && ngroups != 1) return ctk_set_error(CTK_E_INVALID, "%s: group is NULL but ngroups=%d (NULL means one group)", name, ngroups);
    if (group)
        for (int64_t t = 0; t < T; t++)
            if (group[t] < 0 || group[t] >= ngroups) return ctk_set_error(CTK_E_INVALID, "%s: group[%lld] = %d is not in [0, %d)", name, (long long)t, group[t], ngroups);
    HIPCHK(hipSetDevice(h->device));
    return CTK_OK;
}

// ... and the group ids go to the device (fq_group) when there are several groups
static int freq_prepare(ctk_handle *h, const char *name, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int32_t **group_dev)
{
    CTKCHK(group_args_check(h, name, T, ny, nx, group, ngroups));
    *group_dev = nullptr;
    if (group && ngroups > 1) {                                     // (one group: every id is 0, the kernel needs none)
        CTKCHK(ensure(h, h->fq_group, (size_t)T * 4));
        HIPCHK(hipMemcpyAsync(h->fq_group.p, group, (size_t)T * 4, hipMemcpyHostToDevice, h->stream));
        *group_dev = P<int32_t>(h->fq_group);
    }
    return CTK_OK;
}

extern "C" int ctk_frequency_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                                 uint32_t *counts_dev, int accumulate)
{
    if (h && (!flag_dev || !counts_dev)) return ctk_set_error(CTK_E_INVALID, "ctk_frequency_dev: null buffer");
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, "ctk_frequency_dev", T, ny, nx, group, ngroups, &group_dev));
    const int64_t npix = (int64_t)ny * nx;
    if (!accumulate) HIPCHK(hipMemsetAsync(counts_dev, 0, (size_t)ngroups * npix * 4, h->stream));
    CTKCHK(launch_freq(h, flag_dev, T, npix, group_dev, above, counts_dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

// host array or reader callback: the flag passes through two chunk-sized device buffers (stream_in: chunk k+1 is read and copied
// while k_freq counts chunk k); the counts stay in HBM until the last chunk
static int freq_stream_impl(ctk_handle *h, StreamIO &io, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above, uint32_t *counts,
                            int64_t chunk_steps, const char *name)
{
    if (h && !counts) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    if (h && chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps=%lld", name, (long long)chunk_steps);
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, name, T, ny, nx, group, ngroups, &group_dev));
    const int64_t npix = (int64_t)ny * nx;
    const size_t plane = (size_t)npix * 4, cbytes = (size_t)ngroups * plane;
    io.esz = 4;
    io.chunk = ctk_stream_chunk(chunk_steps, T, plane);
    CTKCHK(ensure(h, h->fq_counts, cbytes));
    uint32_t *cdev = P<uint32_t>(h->fq_counts);
    HIPCHK(hipMemsetAsync(cdev, 0, cbytes, h->stream));
    const double t0 = now_ms();
    CTKCHK(stream_consume(h, io, false, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        return launch_freq(h, (const int32_t *)chunk, nt, npix, group_dev ? group_dev + c0 : nullptr, above, cdev);
    }));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(counts, cdev, cbytes, hipMemcpyDeviceToHost));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

extern "C" int ctk_frequency(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                             uint32_t *counts, int64_t chunk_steps)
{
    if (h && !flag) return ctk_set_error(CTK_E_INVALID, "ctk_frequency: null buffer");
    StreamIO io;
    io.host_in = flag;
    return freq_stream_impl(h, io, T, ny, nx, group, ngroups, above, counts, chunk_steps, "ctk_frequency");
}

extern "C" int ctk_frequency_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *group, int ngroups,
                                int32_t above, uint32_t *counts, int64_t chunk_steps)
{
    if (h && !reader) return ctk_set_error(CTK_E_INVALID, "ctk_frequency_cb: null reader");
    StreamIO io;
    io.read = reader; io.read_user = reader_user;
    return freq_stream_impl(h, io, T, ny, nx, group, ngroups, above, counts, chunk_steps, "ctk_frequency_cb");
}

// experiments (tools/freq_probe.py): timesteps per slice (0: the rule of ctk_time_slice) and the 16-byte loads (0 plain, 1 nontemporal,
// -1 the default: nontemporal)
extern "C" int ctk_debug_set_freq(ctk_handle *h, int64_t slice, int nt)
{
    if (!h || slice < 0 || nt < -1 || nt > 1) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_freq: null handle, negative slice or nt not -1 / 0 / 1");
    h->fq_slice_dbg = slice;
    h->fq_nt = nt;
    return CTK_OK;
}

// k_freq alone between HIP events on the handle's stream, `reps` launches that add to counts_dev after one that overwrites it
// (tools/freq_probe.py): ms2 = {best, mean} per launch
extern "C" int ctk_debug_time_freq(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, int32_t above,
                                   uint32_t *counts_dev, int reps, double *ms2)
{
    if (h && (!flag_dev || !counts_dev || !ms2 || reps < 1)) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_freq: null buffer or reps < 1");
    const int32_t *group_dev = nullptr;
    CTKCHK(freq_prepare(h, "ctk_debug_time_freq", T, ny, nx, group, ngroups, &group_dev));
    if ((int64_t)(reps + 1) * T > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_freq: (reps + 1) * T counts overflow uint32");
    const int64_t npix = (int64_t)ny * nx;
    HIPCHK(hipMemsetAsync(counts_dev, 0, (size_t)ngroups * npix * 4, h->stream));
    return time_launches(h, "ctk_debug_time_freq", reps, ms2, [&]() { return launch_freq(h, flag_dev, T, npix, group_dev, above, counts_dev); });
}
