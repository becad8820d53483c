// The owning types of contrack_amd/csrc/ctk_own.h against a stub of the HIP calls they make: after move construction, move assignment
// over a live buffer, swap, release() and scope exit every allocation was freed exactly once and the live counters are back at zero.
// tests/test_own_host.py builds this with -fsanitize=address,undefined and runs it; no GPU, nothing of HIP is linked.
#include <cstdio>
#include <cstdlib>
#include <map>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct StubEvent *hipEvent_t;
typedef struct StubStream *hipStream_t;

static std::map<void *, int> g_freed;                   // every pointer the stub handed out -> how often it came back (the memory
                                                        // itself is kept until main ends, so that no address comes twice)
static int g_fail_next = 0;                             // the next allocation fails
static int g_bad = 0;
static void *stub_new(size_t n) { void *p = malloc(n ? n : 1); g_freed[p] = 0; return p; }
static hipError_t stub_free(void *p)
{
    auto it = g_freed.find(p);
    if (it == g_freed.end() || it->second++) { printf("freed twice or never allocated: %p\n", p); g_bad++; return 1; }
    return hipSuccess;
}
static hipError_t stub_alloc(void **p, size_t n) { if (g_fail_next) { g_fail_next = 0; return hipErrorOutOfMemory; } *p = stub_new(n); return hipSuccess; }
static hipError_t hipMalloc(void **p, size_t n) { return stub_alloc(p, n); }
static hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return stub_alloc(p, n); }
static hipError_t hipFree(void *p) { return stub_free(p); }
static hipError_t hipHostFree(void *p) { return stub_free(p); }
static hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return stub_alloc((void **)e, 1); }
static hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return stub_alloc((void **)s, 1); }
static hipError_t hipEventDestroy(hipEvent_t e) { return stub_free(e); }
static hipError_t hipStreamDestroy(hipStream_t s) { return stub_free(s); }

#include "../contrack_amd/csrc/ctk_own.h"

#define CHECK(c) do { if (!(c)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #c); g_bad++; } } while (0)
static long live(int k) { return (long)g_ctk_live[k].load(); }

template <typename Buf>
static void buffers(CtkLive kind)
{
    {
        Buf a, b;
        CHECK(a.alloc(100) == hipSuccess && a.cap == 100 && a.p && live(kind) == 1);
        Buf c(std::move(a));                                                    // move construction: the source is empty
        CHECK(!a.p && a.cap == 0 && c.cap == 100 && live(kind) == 1);
        CHECK(b.alloc(200) == hipSuccess && live(kind) == 2);
        void *const was_b = b.p;
        b = std::move(c);                                                       // move assignment over a live buffer frees it
        CHECK(g_freed[was_b] == 1 && b.cap == 100 && !c.p && live(kind) == 1);
        CHECK(c.alloc(300) == hipSuccess);
        void *const pb = b.p, *const pc = c.p;
        b.swap(c);
        CHECK(b.p == pc && b.cap == 300 && c.p == pb && c.cap == 100 && live(kind) == 2);
        c.release();
        CHECK(!c.p && c.cap == 0 && g_freed[pb] == 1 && live(kind) == 1);
        c.release();                                                            // (an empty one: nothing happens)
        g_fail_next = 1;
        CHECK(a.alloc(50) != hipSuccess && !a.p && a.cap == 0 && live(kind) == 1);
    }                                                                           // scope exit frees b
    CHECK(live(kind) == 0);
}

int main()
{
    buffers<DevBuf>(CTK_LIVE_DEV);
    buffers<PinBuf>(CTK_LIVE_PIN);
    {
        PinPair pr;
        CHECK(pr.grow(64, 0) == hipSuccess && pr.cap() == 64 && pr[0] && pr[1] && live(CTK_LIVE_PIN) == 2);
        void *const p0 = pr[0];
        CHECK(pr.grow(32, 0) == hipSuccess && pr[0] == p0);                     // (large enough: kept)
        CHECK(pr.grow(128, 0) == hipSuccess && pr.cap() == 128 && g_freed[p0] == 1 && live(CTK_LIVE_PIN) == 2);
    }
    CHECK(live(CTK_LIVE_PIN) == 0);
    {
        Event e, f;
        Stream s;
        CHECK(e.create() == hipSuccess && s.create(1) == hipSuccess && live(CTK_LIVE_EVENT) == 1 && live(CTK_LIVE_STREAM) == 1);
        const hipEvent_t raw = e;
        CHECK(e.create() == hipSuccess && (hipEvent_t)e == raw);                // (one that exists is kept)
        f = std::move(e);
        CHECK(!(hipEvent_t)e && (hipEvent_t)f == raw && live(CTK_LIVE_EVENT) == 1);
        Event g(std::move(f));
        CHECK(e.create() == hipSuccess && live(CTK_LIVE_EVENT) == 2);
        g = std::move(e);                                                       // over a live event
        CHECK(g_freed[(void *)raw] == 1 && live(CTK_LIVE_EVENT) == 1);
        s.release();
        CHECK(!(hipStream_t)s && live(CTK_LIVE_STREAM) == 0);
    }
    for (int k = 0; k < CTK_LIVE_KINDS; k++) CHECK(live(k) == 0);
    for (const auto &kv : g_freed) {
        if (kv.second != 1) { printf("%p was freed %d times\n", kv.first, kv.second); g_bad++; }
        free(kv.first);
    }
    if (g_bad) printf("own_host: %d failure(s)\n", g_bad);
    else printf("own_host: ok, %zu allocations each freed once\n", g_freed.size());
    return g_bad ? 1 : 0;
}
