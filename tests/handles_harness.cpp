// handles_harness.cpp -- csrc/gs_handles.h against a fake HIP runtime: every allocation / event the handles make is tracked, a release of
// something that is not live aborts, and the k-th creation can be made to fail.  A stand-alone program (tests/test_handles.py builds it with
// -fsanitize=address,undefined and runs it); it is NOT linked against the HIP runtime: the few hip* functions the header calls are defined here.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "../unitygaussiansplatting_amd/csrc/gs_handles.h"

// ---- the fake runtime -------------------------------------------------------------------------------------
static std::set<void*> g_live;          // device + pinned allocations and events
static long g_created = 0;              // creations attempted so far
static long g_failAt = -1;              // the creation (counted from g_created) that fails, -1 = none
static long g_released = 0;

static void die(const char* what) { fprintf(stderr, "FAIL: %s\n", what); abort(); }
static bool inject() { return g_created++ == g_failAt; }
static void* make(size_t bytes) { void* p = malloc(bytes ? bytes : 1); if (!p) die("malloc"); g_live.insert(p); return p; }
static void release(void* p, const char* what) {
    if (!g_live.erase(p)) die(what);
    g_released++;
    free(p);
}
static void fail_next(long k) { g_failAt = g_created + k; }          // k = 0: the next creation

hipError_t hipMalloc(void** p, size_t bytes) { if (inject()) { *p = (void*)0x1; return hipErrorOutOfMemory; } *p = make(bytes); return hipSuccess; }   // (a failed call may leave garbage)
hipError_t hipFree(void* p) { release(p, "hipFree of a pointer that is not live"); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { if (inject()) { *p = (void*)0x1; return hipErrorOutOfMemory; } *p = make(bytes); return hipSuccess; }
hipError_t hipHostFree(void* p) { release(p, "hipHostFree of a pointer that is not live"); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** dev, void* host, unsigned int) {
    if (!g_live.count(host)) die("hipHostGetDevicePointer of a pointer that is not live");
    *dev = host;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { if (inject()) { *e = (hipEvent_t)0x1; return hipErrorOutOfMemory; } *e = (hipEvent_t)make(8); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e) { release((void*)e, "hipEventDestroy of an event that is not live"); return hipSuccess; }

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// ---- one uniform face over the three types ------------------------------------------------------------------
using gs::DevBuf; using gs::PinnedBuf; using gs::Event;
static hipError_t make_one(DevBuf<int>& h) { return h.alloc(64); }
static hipError_t make_one(PinnedBuf<int>& h) { return h.alloc(64, hipHostMallocMapped); }
static hipError_t make_one(Event& h) { return h.create(hipEventDisableTiming); }
static void* raw(const DevBuf<int>& h) { return (int*)h; }
static void* raw(const PinnedBuf<int>& h) { return (int*)h; }
static void* raw(const Event& h) { return (hipEvent_t)h; }

template <class H>
static void lifecycle() {
    const size_t base = g_live.size();
    {   // alloc and scope exit
        H a;
        CHECK(!raw(a));
        CHECK(make_one(a) == hipSuccess && raw(a) && g_live.size() == base + 1 && g_live.count(raw(a)));
    }
    CHECK(g_live.size() == base);
    {   // move construction
        H a; CHECK(make_one(a) == hipSuccess);
        void* p = raw(a);
        H b(std::move(a));
        CHECK(!raw(a) && raw(b) == p && g_live.size() == base + 1);
    }
    CHECK(g_live.size() == base);
    {   // move assignment onto a non-empty handle: the old allocation goes, exactly once
        H a, b; CHECK(make_one(a) == hipSuccess && make_one(b) == hipSuccess);
        void* pa = raw(a); void* pb = raw(b);
        const long rel = g_released;
        b = std::move(a);
        CHECK(g_released == rel + 1 && !g_live.count(pb) && g_live.count(pa) && raw(b) == pa && !raw(a));
        H& self = b;                     // self-move: nothing changes
        b = std::move(self);
        CHECK(raw(b) == pa && g_live.count(pa) && g_released == rel + 1);
    }
    CHECK(g_live.size() == base);
    {   // std::swap
        H a, b; CHECK(make_one(a) == hipSuccess);
        void* pa = raw(a);
        const long rel = g_released;
        std::swap(a, b);
        CHECK(!raw(a) && raw(b) == pa && g_released == rel);
        CHECK(make_one(a) == hipSuccess);
        void* pa2 = raw(a);
        std::swap(a, b);
        CHECK(raw(a) == pa && raw(b) == pa2 && g_released == rel && g_live.size() == base + 2);
    }
    CHECK(g_live.size() == base);
    {   // alloc on a non-empty handle; reset twice
        H a; CHECK(make_one(a) == hipSuccess);
        void* p = raw(a);
        const long rel = g_released;
        CHECK(make_one(a) == hipSuccess);
        CHECK(g_released == rel + 1 && !g_live.count(p) && g_live.count(raw(a)) && g_live.size() == base + 1);
        a.reset(); CHECK(!raw(a) && g_live.size() == base);
        a.reset(); CHECK(!raw(a) && g_live.size() == base);
    }
    {   // a failed alloc leaves the handle null and releases what it held
        H a; CHECK(make_one(a) == hipSuccess);
        fail_next(0);
        CHECK(make_one(a) != hipSuccess);
        CHECK(!raw(a) && g_live.size() == base);
        fail_next(0);
        CHECK(make_one(a) != hipSuccess && !raw(a));      // ... also from empty
        CHECK(make_one(a) == hipSuccess && raw(a));
    }
    CHECK(g_live.size() == base);
}

static void pinned_device_address() {
    PinnedBuf<int> m, d;
    CHECK(m.alloc(16, hipHostMallocMapped) == hipSuccess && m.device() == m.get() && m.get());     // (the fake maps a host address onto itself)
    CHECK(d.alloc(16, hipHostMallocDefault) == hipSuccess && d.get() && !d.device());
    PinnedBuf<int> n(std::move(m));
    CHECK(n.device() == n.get() && !m.device() && !m.get());
    d = std::move(n);
    CHECK(d.device() == d.get() && d.get() && !n.device());
    d.reset();
    CHECK(!d.device() && !d.get());
}

static void event_ring() {
    const size_t base = g_live.size();
    {
        std::vector<Event> ring;
        std::vector<void*> seen;
        for (int k = 0; k < 100; ++k) {          // growth relocates the handles: by move, never by a second destroy
            ring.emplace_back();
            CHECK(ring.back().create(0) == hipSuccess);
            seen.push_back(raw(ring.back()));
        }
        CHECK(g_live.size() == base + 100);
        for (int k = 0; k < 100; ++k) CHECK(raw(ring[(size_t)k]) == seen[(size_t)k]);
        std::vector<Event> bigger(200);           // the library's ring growth: a new vector, committed by move
        for (Event& e : bigger) CHECK(e.create(0) == hipSuccess);
        ring = std::move(bigger);
        CHECK(ring.size() == 200 && g_live.size() == base + 200);
        for (void* p : seen) CHECK(!g_live.count(p));
    }
    CHECK(g_live.size() == base);
}

// ---- commit by move, as the library grows several buffers together -------------------------------------------
struct Triple { DevBuf<int> a, b, c; int size = 0; };

static hipError_t grow(Triple& t, int size) {
    DevBuf<int> a, b, c;
    hipError_t e = a.alloc((size_t)size);
    if (e == hipSuccess) e = b.alloc((size_t)size);
    if (e == hipSuccess) e = c.alloc((size_t)size);
    if (e != hipSuccess) return e;                // the locals release what was made
    t.a = std::move(a); t.b = std::move(b); t.c = std::move(c); t.size = size;
    return hipSuccess;
}

static void commit_by_move() {
    const size_t base = g_live.size();
    {
        Triple t;
        for (int k = 0; k < 3; ++k) {            // from empty: nothing is left behind
            fail_next(k);
            CHECK(grow(t, 32) != hipSuccess);
            CHECK(!t.a && !t.b && !t.c && t.size == 0 && g_live.size() == base);
        }
        CHECK(grow(t, 32) == hipSuccess && g_live.size() == base + 3);
        int* const pa = t.a; int* const pb = t.b; int* const pc = t.c;
        for (int k = 0; k < 3; ++k) {            // the first, second, third creation fails: exactly the old three stay
            fail_next(k);
            CHECK(grow(t, 64) != hipSuccess);
            CHECK(t.a == pa && t.b == pb && t.c == pc && t.size == 32);
            CHECK(g_live.size() == base + 3 && g_live.count(pa) && g_live.count(pb) && g_live.count(pc));
        }
        CHECK(grow(t, 64) == hipSuccess && t.size == 64);
        CHECK(g_live.size() == base + 3 && !g_live.count(pa) && !g_live.count(pb) && !g_live.count(pc));
    }
    CHECK(g_live.size() == base);
}

int main() {
    lifecycle<DevBuf<int>>();
    lifecycle<PinnedBuf<int>>();
    lifecycle<Event>();
    pinned_device_address();
    event_ring();
    commit_by_move();
    if (!g_live.empty()) { fprintf(stderr, "FAIL: %zu handles still live at exit\n", g_live.size()); return 1; }
    printf("handles ok: %ld created, %ld released\n", g_created, g_released);
    return 0;
}
