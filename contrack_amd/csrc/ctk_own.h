// ctk_own.h -- owners of the GPU resources a ctk_handle and its helpers hold: device buffers, pinned host buffers, events, streams.
// Each is move-only and frees what it holds in its destructor, so nothing is released by name anywhere; each counts its live
// instances (ctk_debug_live).  Host code only.  The includer brings the HIP runtime's declarations (hipcc does; tests/own_host.cpp
// brings a stub of them); the policies -- head room, retries, error texts, the wait for a collective -- are ensure() / ensure_host()
// in ctk_api.hip.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

enum CtkLive { CTK_LIVE_DEV = 0, CTK_LIVE_PIN, CTK_LIVE_EVENT, CTK_LIVE_STREAM, CTK_LIVE_KINDS };
inline std::atomic<int64_t> g_ctk_live[CTK_LIVE_KINDS];        // device buffers, pinned buffers, events, streams alive in this process

// hipMalloc (DevBuf) or hipHostMalloc (PinBuf) memory.  p and cap are public: the launches read them, only the members write them.
template <CtkLive KIND>
struct OwnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept { swap(o); }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    ~OwnedBuf() { release(); }
    void swap(OwnedBuf &o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    void release()                                          // free now; empty afterwards
    {
        if (p) { (void)(KIND == CTK_LIVE_DEV ? hipFree(p) : hipHostFree(p)); g_ctk_live[KIND]--; }
        p = nullptr; cap = 0;
    }
    // exactly `bytes` into an EMPTY buffer (flags: hipHostMalloc's, pinned memory only); a failure leaves it empty
    hipError_t alloc(size_t bytes, unsigned flags = 0)
    {
        const hipError_t e = KIND == CTK_LIVE_DEV ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes; g_ctk_live[KIND]++;
        return hipSuccess;
    }
};
using DevBuf = OwnedBuf<CTK_LIVE_DEV>;
using PinBuf = OwnedBuf<CTK_LIVE_PIN>;

// Two pinned buffers of one size that grow together (the chunk buffers of the streaming entries, the table twins of ctk_band_*):
// exactly the bytes asked for, no head room.  cap() is 0 until BOTH exist, so a pair whose second allocation failed is built anew.
struct PinPair {
    PinBuf b[2];
    void *operator[](int i) const { return b[i].p; }
    size_t cap() const { return b[1].cap; }
    void release() { b[0].release(); b[1].release(); }
    hipError_t grow(size_t bytes, unsigned flags)
    {
        if (bytes <= cap()) return hipSuccess;
        release();
        for (PinBuf &x : b) { const hipError_t e = x.alloc(bytes, flags); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
};

// A HIP event (Event) or stream (Stream); converts to the raw handle, so launches and hipEventRecord take it as it is.
template <typename Raw, CtkLive KIND>
struct OwnedHandle {
    Raw raw = nullptr;
    OwnedHandle() = default;
    OwnedHandle(const OwnedHandle &) = delete;
    OwnedHandle &operator=(const OwnedHandle &) = delete;
    OwnedHandle(OwnedHandle &&o) noexcept { std::swap(raw, o.raw); }
    OwnedHandle &operator=(OwnedHandle &&o) noexcept { if (this != &o) { release(); std::swap(raw, o.raw); } return *this; }
    ~OwnedHandle() { release(); }
    operator Raw() const { return raw; }
    void release()
    {
        if (raw) { if constexpr (KIND == CTK_LIVE_EVENT) (void)hipEventDestroy(raw); else (void)hipStreamDestroy(raw); g_ctk_live[KIND]--; }
        raw = nullptr;
    }
    // one that exists is kept.  flags: hipEventCreateWithFlags' (0: a timing event, as hipEventCreate makes it) / hipStreamCreateWithFlags'
    hipError_t create(unsigned flags = 0)
    {
        if (raw) return hipSuccess;
        hipError_t e;
        if constexpr (KIND == CTK_LIVE_EVENT) e = hipEventCreateWithFlags(&raw, flags); else e = hipStreamCreateWithFlags(&raw, flags);
        if (e != hipSuccess) { raw = nullptr; return e; }
        g_ctk_live[KIND]++;
        return hipSuccess;
    }
};
using Event = OwnedHandle<hipEvent_t, CTK_LIVE_EVENT>;
using Stream = OwnedHandle<hipStream_t, CTK_LIVE_STREAM>;
