// ctk_spell.hip -- blocked spells per grid point (included by ctk_api.hip): how many blocking events passed over a grid point and how
// long it stayed blocked each time, the pair of maps beside the frequency map of a blocking climatology.  At pixel p, step t CONTINUES
// step t-1 iff
//     t is not a segment start  and  flag[t-1][p] > above  and  flag[t][p] > above  and  (by_id: flag[t-1][p] == flag[t][p])
// A spell is a maximal chain of continuing steps that starts at a step with flag > above; its duration d is its number of steps, its
// group is group[onset].  Spells with d >= min_duration are counted:
//     events[g][p] = their number, steps[g][p] = the sum of their durations, longest[g][p] = the longest (0: none)
// The division steps / events is left to the caller, as the frequency's is.
//
// k_spell: k_freq's geometry -- one thread per 4 consecutive pixels and one slice of timesteps (blockIdx.y), nontemporal 16-byte loads
// when the plane and the pointer allow it, 4 int32 loads otherwise, the per-step word (group id, bit 31: segment start) read through
// the constant address space.  There are no per-slice summaries and no merge pass: A SPELL IS OWNED BY THE THREAD WHOSE SLICE HOLDS
// ITS ONSET.  A thread looks back one step (t0 - 1) to see whether the run at its slice start continues an older one -- then it
// skips that run -- and follows every spell that starts inside its slice forward until it ends, beyond its own slice end if need
// be (its four pixels together, with the slice's own loads).  Both decisions are the one predicate above, so neighbouring slices
// cannot disagree.  The spell is published with atomicAdd (events, steps) and atomicMax (longest) at group[onset]: integer atomics
// commute, so the result is exact whatever the slice length and the scheduling.  A permanently flagged pixel degenerates to one
// thread walking T: slow, but correct.
//
// Chunks (the streamed entries): a run that is open at the end of a chunk goes to a per-pixel carry record {length so far, last flag
// value, onset group} (12 bytes per pixel) with exactly one writer per pixel -- the owner of the spell that holds the chunk's last
// step or, if that step is unflagged, the last slice's thread, which writes "none" (length 0).  Slice 0 of the next chunk starts
// from the carry instead of looking back.  Within one launch a late slice writes the carry slice 0 reads, so carry-in and carry-out
// are two buffers, swapped per chunk.  After the last chunk k_spell_close publishes what the carry still holds.  The resident entry
// is the same code with one chunk.
#pragma once

constexpr int kSpellUnroll = 8;                  // timesteps whose loads are in flight together
constexpr uint32_t kSpellBreak = 0x80000000u;    // bit 31 of a step's word: the step starts a segment

struct SpellArgs {
    const int32_t *flag;                         // [nt][npix], this chunk
    const int32_t *words;                        // [nt] group id | kSpellBreak (nullptr: one group, no break inside the slab)
    const uint32_t *carry_in;                    // [3][npix]: length (0: none), last flag value, onset group
    uint32_t *carry_out;
    uint32_t *events, *steps, *longest;          // [G][npix]
    int64_t nt, npix, slice;
    int32_t above;
    uint32_t min_d;
    int by_id;
};

__device__ __forceinline__ void spell_publish(const SpellArgs &a, int64_t p, uint32_t len, uint32_t g)
{
    const int64_t i = (int64_t)g * a.npix + p;
    atomicAdd(a.events + i, 1u);
    atomicAdd(a.steps + i, len);
    atomicMax(a.longest + i, len);
}

template <bool VEC, bool WORDS, bool NT>
__global__ __launch_bounds__(256) CTK_SGPR_8WAVES void k_spell(const SpellArgs a)
{
    const int64_t npix = a.npix;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;          // first pixel of this thread's quad (64-bit: > 2^32 elements)
    if (p0 >= npix) return;
    const int64_t t0 = (int64_t)blockIdx.y * a.slice, t1 = min(a.nt, t0 + a.slice);
    const int32_t above = a.above;
    const bool by_id = a.by_id != 0;
    ctk_const_i32 *words = (ctk_const_i32 *)a.words;
    auto load = [&](int64_t t) __attribute__((always_inline)) -> ctk_i32x4 {
        const int32_t *q = a.flag + t * npix + p0;
        if (VEC) return NT ? __builtin_nontemporal_load((const ctk_i32x4 *)q) : *(const ctk_i32x4 *)q;
        // general path (ny * nx % 4 != 0 or an unaligned pointer): pixels beyond the plane read as INT_MIN, which is never > above
        ctk_i32x4 v;
        v.x = q[0];
        v.y = p0 + 1 < npix ? q[1] : INT32_MIN;
        v.z = p0 + 2 < npix ? q[2] : INT32_MIN;
        v.w = p0 + 3 < npix ? q[3] : INT32_MIN;
        return v;
    };
    // per pixel: the flag of the step before, the length of the open run this thread owns (0 with pv > above: a run an earlier
    // slice owns, skipped), its onset group -- and one finished spell waiting to be published (plen 0: none).  The atomics of a wave
    // are few lanes wide, and an instruction costs the memory pipeline the same whatever its lanes: a spell that ends is parked
    // here and the four slots are flushed once per kSpellUnroll steps instead of wherever a lane happens to close (measured:
    // profiles/NOTES.md)
    struct Px { int32_t pv; uint32_t len, og, plen, pog; } x0, x1, x2, x3;
    const uint32_t min_d = a.min_d;
    auto close = [&](Px &x, int64_t p) __attribute__((always_inline)) {         // the open run of x has ended
        if (x.len >= min_d) {
            if (x.plen) spell_publish(a, p, x.plen, x.pog);                      // (two ends within one batch of steps: rare)
            x.plen = x.len;
            x.pog = x.og;
        }
    };
    auto flush = [&](Px &x, int64_t p) __attribute__((always_inline)) {
        if (x.plen) { spell_publish(a, p, x.plen, x.pog); x.plen = 0; }
    };
    auto flush4 = [&]() __attribute__((always_inline)) { flush(x0, p0); flush(x1, p0 + 1); flush(x2, p0 + 2); flush(x3, p0 + 3); };
    if (blockIdx.y == 0) {                                                      // the chunk's first slice: from the carry
        auto from_carry = [&](Px &x, int64_t p) __attribute__((always_inline)) {
            const uint32_t l = p < npix ? a.carry_in[p] : 0u;
            x.len = l;
            x.pv = l ? (int32_t)a.carry_in[npix + p] : INT32_MIN;
            x.og = l ? a.carry_in[2 * npix + p] : 0u;
            x.plen = x.pog = 0;
        };
        from_carry(x0, p0); from_carry(x1, p0 + 1); from_carry(x2, p0 + 2); from_carry(x3, p0 + 3);
    } else {                                                                    // look back one step
        const ctk_i32x4 v = load(t0 - 1);
        x0 = {v.x, 0u, 0u, 0u, 0u}; x1 = {v.y, 0u, 0u, 0u, 0u}; x2 = {v.z, 0u, 0u, 0u, 0u}; x3 = {v.w, 0u, 0u, 0u, 0u};
    }
    auto step = [&](Px &x, int64_t p, int32_t v, bool brk, uint32_t g) __attribute__((always_inline)) {
        const bool on = v > above;
        const bool cont = !brk && on && x.pv > above && (!by_id || x.pv == v);
        if (cont) {
            x.len += x.len != 0;                                                // (a skipped run stays at 0)
        } else {
            if (x.len) close(x, p);
            x.len = on;
            x.og = g;
        }
        x.pv = v;
    };
    auto advance = [&](int64_t tt, const ctk_i32x4 &v) __attribute__((always_inline)) {
        const uint32_t w = WORDS ? (uint32_t)words[tt] : 0u;
        const bool brk = (w & kSpellBreak) != 0;
        const uint32_t g = w & ~kSpellBreak;
        step(x0, p0, v.x, brk, g); step(x1, p0 + 1, v.y, brk, g); step(x2, p0 + 2, v.z, brk, g); step(x3, p0 + 3, v.w, brk, g);
    };
    int64_t t = t0;
    for (; t + kSpellUnroll <= t1; t += kSpellUnroll) {
        ctk_i32x4 v[kSpellUnroll];
#pragma unroll
        for (int u = 0; u < kSpellUnroll; u++) v[u] = load(t + u);
#pragma unroll
        for (int u = 0; u < kSpellUnroll; u++) advance(t + u, v[u]);
        flush4();
    }
    for (; t < t1; t++) advance(t, load(t));
    // the chunk's last slice: a pixel whose last step is unflagged has no open run -- this thread says so (a flagged one the thread
    // does not own is its owner's to write)
    if (t1 == a.nt) {
        auto none = [&](const Px &x, int64_t p) __attribute__((always_inline)) {
            if (!x.len && p < npix && !(x.pv > above)) a.carry_out[p] = 0;
        };
        none(x0, p0); none(x1, p0 + 1); none(x2, p0 + 2); none(x3, p0 + 3);
    }
    // the runs still open at the slice end: their owner follows them until they end or the chunk does -- the four pixels together,
    // kSpellUnroll steps in flight as in the slice itself (a pixel whose run has ended only waits for the others: len 0)
    auto follow = [&](Px &x, int64_t p, int32_t v, bool brk) __attribute__((always_inline)) {
        if (!x.len) return;
        if (!brk && v > above && (!by_id || x.pv == v)) {
            x.len++;
            x.pv = v;
        } else {
            close(x, p);
            x.len = 0;
        }
    };
    auto follow4 = [&](int64_t tt, const ctk_i32x4 &v) __attribute__((always_inline)) {
        const bool brk = WORDS && ((uint32_t)words[tt] & kSpellBreak) != 0;
        follow(x0, p0, v.x, brk); follow(x1, p0 + 1, v.y, brk); follow(x2, p0 + 2, v.z, brk); follow(x3, p0 + 3, v.w, brk);
    };
    for (; t + kSpellUnroll <= a.nt && (x0.len | x1.len | x2.len | x3.len); t += kSpellUnroll) {
        ctk_i32x4 v[kSpellUnroll];
#pragma unroll
        for (int u = 0; u < kSpellUnroll; u++) v[u] = load(t + u);
#pragma unroll
        for (int u = 0; u < kSpellUnroll; u++) follow4(t + u, v[u]);
    }
    for (; t < a.nt && (x0.len | x1.len | x2.len | x3.len); t++) follow4(t, load(t));
    flush4();
    // open at the chunk end: the one writer of this pixel's carry
    auto to_carry = [&](const Px &x, int64_t p) __attribute__((always_inline)) {
        if (!x.len) return;
        a.carry_out[p] = x.len;
        a.carry_out[npix + p] = (uint32_t)x.pv;
        a.carry_out[2 * npix + p] = x.og;
    };
    to_carry(x0, p0); to_carry(x1, p0 + 1); to_carry(x2, p0 + 2); to_carry(x3, p0 + 3);
}

// what the carry holds after the last chunk: the spells the end of the slab cuts
__global__ __launch_bounds__(256) void k_spell_close(const SpellArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.npix) return;
    const uint32_t l = a.carry_in[p];
    if (l >= a.min_d) spell_publish(a, p, l, a.carry_in[2 * a.npix + p]);                // (0: none; min_d >= 1)
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// The look-back costs one plane per slice and a follow-up reads single pixels, so short slices are dearer than in k_freq
// (profiles/NOTES.md: the sweep)
constexpr int64_t kSpellSliceMin = 16;       // (the other two numbers of the rule: k_freq's, ctk_freq.hip)

// one chunk: a.flag[0..a.nt) with the carry of the chunk before (a.carry_in) -> publishes, a.carry_out
static int launch_spell(ctk_handle *h, SpellArgs a)
{
    a.slice = ctk_time_slice(h->sp_slice_dbg, a.nt, a.npix, kSpellSliceMin, kSliceMax, kSliceWaves);
    const int64_t bx = ((a.npix + 3) / 4 + 255) / 256;
    if (bx > 0x7fffffffll) return ctk_set_error(CTK_E_RANGE, "ctk_spells: a plane of %lld pixels is too large", (long long)a.npix);
    const dim3 grid((unsigned)bx, (unsigned)((a.nt + a.slice - 1) / a.slice));
    const bool vec = a.npix % 4 == 0 && ((uintptr_t)a.flag & 15) == 0;
    if (vec) {
        if (a.words) k_spell<true, true, true><<<grid, 256, 0, h->stream>>>(a);
        else         k_spell<true, false, true><<<grid, 256, 0, h->stream>>>(a);
    } else {
        if (a.words) k_spell<false, true, false><<<grid, 256, 0, h->stream>>>(a);
        else         k_spell<false, false, false><<<grid, 256, 0, h->stream>>>(a);
    }
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

static int launch_spell_close(ctk_handle *h, const SpellArgs &a)
{
    k_spell_close<<<(unsigned)((a.npix + 255) / 256), 256, 0, h->stream>>>(a);
    HIPCHK(hipGetLastError());
    return CTK_OK;
}

// arguments shared by the entries; the per-step words (group id, bit 31: segment start) go to the device (sp_words) when there are
// several groups or a break inside the slab; both carries are allocated and the first one is set to "none"
static int spell_prepare(ctk_handle *h, const char *name, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts,
                         int64_t nseg, int by_id, int64_t min_duration, SpellArgs *a)
{
    CTKCHK(group_args_check(h, name, T, ny, nx, group, ngroups));
    if (by_id != 0 && by_id != 1) return ctk_set_error(CTK_E_INVALID, "%s: by_id=%d (0 or 1)", name, by_id);
    if (min_duration < 1) return ctk_set_error(CTK_E_INVALID, "%s: min_duration=%lld (at least 1)", name, (long long)min_duration);
    CTKCHK(segment_starts_check(name, seg_starts, nseg, T));
    const int64_t npix = (int64_t)ny * nx;
    *a = SpellArgs();
    a->npix = npix;
    a->by_id = by_id;
    a->min_d = (uint32_t)std::min<int64_t>(min_duration, 0xffffffffll);
    if ((group && ngroups > 1) || nseg > 1) {                       // (one group and no break: every word is 0, the kernel needs none)
        std::vector<uint32_t> &w = h->sp_words_host;                // (kept: the copy below may still read it when this returns)
        w.assign((size_t)T, 0u);
        if (group && ngroups > 1)
            for (int64_t t = 0; t < T; t++) w[(size_t)t] = (uint32_t)group[t];
        for (int64_t k = 0; k < nseg; k++) w[(size_t)seg_starts[k]] |= kSpellBreak;
        CTKCHK(ensure(h, h->sp_words, (size_t)T * 4));
        HIPCHK(hipMemcpyAsync(h->sp_words.p, w.data(), (size_t)T * 4, hipMemcpyHostToDevice, h->stream));
        a->words = P<int32_t>(h->sp_words);
    }
    CTKCHK(ensure(h, h->sp_carry, (size_t)npix * 24));
    HIPCHK(hipMemsetAsync(h->sp_carry.p, 0, (size_t)npix * 4, h->stream));                 // lengths of carry 0: none
    return CTK_OK;
}

// the carry chunk k reads (k & 1) and the one it writes
static void spell_carries(ctk_handle *h, SpellArgs *a, int64_t k)
{
    uint32_t *c = P<uint32_t>(h->sp_carry);
    a->carry_in = c + (size_t)(k & 1) * 3 * a->npix;
    a->carry_out = c + (size_t)((k + 1) & 1) * 3 * a->npix;
}

extern "C" int ctk_spells_dev(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts,
                              int64_t nseg, int32_t above, int by_id, int64_t min_duration, uint32_t *events_dev, uint32_t *steps_dev, uint32_t *longest_dev)
{
    if (h && (!flag_dev || !events_dev || !steps_dev || !longest_dev)) return ctk_set_error(CTK_E_INVALID, "ctk_spells_dev: null buffer");
    SpellArgs a;
    CTKCHK(spell_prepare(h, "ctk_spells_dev", T, ny, nx, group, ngroups, seg_starts, nseg, by_id, min_duration, &a));
    const size_t obytes = (size_t)ngroups * a.npix * 4;
    HIPCHK(hipMemsetAsync(events_dev, 0, obytes, h->stream));
    HIPCHK(hipMemsetAsync(steps_dev, 0, obytes, h->stream));
    HIPCHK(hipMemsetAsync(longest_dev, 0, obytes, h->stream));
    if (min_duration <= T) {                                        // (no spell is longer than the slab)
        a.flag = flag_dev; a.nt = T; a.above = above;
        a.events = events_dev; a.steps = steps_dev; a.longest = longest_dev;
        spell_carries(h, &a, 0);
        CTKCHK(launch_spell(h, a));
        spell_carries(h, &a, 1);
        CTKCHK(launch_spell_close(h, a));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTK_OK;
}

// host array or reader callback: the flag passes through two chunk-sized device buffers (stream_in: chunk k+1 is read and copied
// while k_spell scans chunk k); the three maps and the carries stay in HBM until the last chunk
static int spell_stream_impl(ctk_handle *h, StreamIO &io, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts, int64_t nseg,
                             int32_t above, int by_id, int64_t min_duration, uint32_t *events, uint32_t *steps, uint32_t *longest, int64_t chunk_steps,
                             const char *name)
{
    if (h && (!events || !steps || !longest)) return ctk_set_error(CTK_E_INVALID, "%s: null buffer", name);
    if (h && chunk_steps < 0) return ctk_set_error(CTK_E_INVALID, "%s: chunk_steps=%lld", name, (long long)chunk_steps);
    SpellArgs a;
    CTKCHK(spell_prepare(h, name, T, ny, nx, group, ngroups, seg_starts, nseg, by_id, min_duration, &a));
    const int64_t npix = a.npix;
    const size_t plane = (size_t)npix * 4, obytes = (size_t)ngroups * plane;
    io.esz = 4;
    io.chunk = ctk_stream_chunk(chunk_steps, T, plane);
    CTKCHK(ensure(h, h->sp_out, 3 * obytes));
    uint32_t *odev = P<uint32_t>(h->sp_out);
    HIPCHK(hipMemsetAsync(odev, 0, 3 * obytes, h->stream));
    a.above = above;
    a.events = odev; a.steps = odev + (size_t)ngroups * npix; a.longest = odev + 2 * (size_t)ngroups * npix;
    const uint32_t *words = (const uint32_t *)a.words;
    const bool none = min_duration > T;                             // (no spell is longer than the slab; the slab is still read)
    const double t0 = now_ms();
    int64_t k = 0;
    CTKCHK(stream_consume(h, io, false, T, ny, nx, [&](const void *chunk, int64_t c0, int64_t nt) -> int {
        if (none) return CTK_OK;
        a.flag = (const int32_t *)chunk; a.nt = nt;
        a.words = words ? (const int32_t *)(words + c0) : nullptr;
        spell_carries(h, &a, k++);
        return launch_spell(h, a);
    }));
    if (!none) {
        spell_carries(h, &a, k);
        CTKCHK(launch_spell_close(h, a));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(events, a.events, obytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(steps, a.steps, obytes, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(longest, a.longest, obytes, hipMemcpyDeviceToHost));
    h->ms[CTK_T_H2D] = io.ms_in; h->ms[CTK_T_TOTAL] = now_ms() - t0;
    return CTK_OK;
}

extern "C" int ctk_spells(ctk_handle *h, const int32_t *flag, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts, int64_t nseg,
                          int32_t above, int by_id, int64_t min_duration, uint32_t *events, uint32_t *steps, uint32_t *longest, int64_t chunk_steps)
{
    if (h && !flag) return ctk_set_error(CTK_E_INVALID, "ctk_spells: null buffer");
    StreamIO io;
    io.host_in = flag;
    return spell_stream_impl(h, io, T, ny, nx, group, ngroups, seg_starts, nseg, above, by_id, min_duration, events, steps, longest, chunk_steps, "ctk_spells");
}

extern "C" int ctk_spells_cb(ctk_handle *h, int64_t T, int ny, int nx, ctk_read_chunk_fn reader, void *reader_user, const int32_t *group, int ngroups,
                             const int64_t *seg_starts, int64_t nseg, int32_t above, int by_id, int64_t min_duration, uint32_t *events, uint32_t *steps,
                             uint32_t *longest, int64_t chunk_steps)
{
    if (h && !reader) return ctk_set_error(CTK_E_INVALID, "ctk_spells_cb: null reader");
    StreamIO io;
    io.read = reader; io.read_user = reader_user;
    return spell_stream_impl(h, io, T, ny, nx, group, ngroups, seg_starts, nseg, above, by_id, min_duration, events, steps, longest, chunk_steps, "ctk_spells_cb");
}

// experiments and tests (tools/spell_probe.py): timesteps per slice (0: the rule of ctk_time_slice)
extern "C" int ctk_debug_set_spell(ctk_handle *h, int64_t slice)
{
    if (!h || slice < 0) return ctk_set_error(CTK_E_INVALID, "ctk_debug_set_spell: null handle or negative slice");
    h->sp_slice_dbg = slice;
    return CTK_OK;
}

// k_spell alone (one chunk of T steps, no k_spell_close) between HIP events on the handle's stream, `reps` launches that add to the
// three maps after one on zeroed maps (tools/spell_probe.py): ms2 = {best, mean} per launch
extern "C" int ctk_debug_time_spell(ctk_handle *h, const int32_t *flag_dev, int64_t T, int ny, int nx, const int32_t *group, int ngroups, const int64_t *seg_starts,
                                    int64_t nseg, int32_t above, int by_id, int64_t min_duration, uint32_t *events_dev, uint32_t *steps_dev, uint32_t *longest_dev,
                                    int reps, double *ms2)
{
    if (h && (!flag_dev || !events_dev || !steps_dev || !longest_dev || !ms2 || reps < 1)) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_spell: null buffer or reps < 1");
    SpellArgs a;
    CTKCHK(spell_prepare(h, "ctk_debug_time_spell", T, ny, nx, group, ngroups, seg_starts, nseg, by_id, min_duration, &a));
    if ((int64_t)(reps + 1) * T > 0xffffffffll) return ctk_set_error(CTK_E_INVALID, "ctk_debug_time_spell: (reps + 1) * T steps overflow uint32");
    const size_t obytes = (size_t)ngroups * a.npix * 4;
    a.flag = flag_dev; a.nt = T; a.above = above;
    a.events = events_dev; a.steps = steps_dev; a.longest = longest_dev;
    spell_carries(h, &a, 0);
    HIPCHK(hipMemsetAsync(events_dev, 0, obytes, h->stream));
    HIPCHK(hipMemsetAsync(steps_dev, 0, obytes, h->stream));
    HIPCHK(hipMemsetAsync(longest_dev, 0, obytes, h->stream));
    return time_launches(h, "ctk_debug_time_spell", reps, ms2, [&]() { return launch_spell(h, a); });
}
