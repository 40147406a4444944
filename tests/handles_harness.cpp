// handles_harness.cpp -- csrc/gs_handles.h against a fake HIP runtime: every allocation / event the handles make is tracked, a release of
// something that is not live aborts, and the k-th creation can be made to fail.  The fake also has streams, each with a vector clock, so that
// what gs::order_after promises -- and the sequences the library builds from it -- are checked as happens-before.  A stand-alone program (tests/test_handles.py builds it with
// -fsanitize=address,undefined and runs it); it is NOT linked against the HIP runtime: the few hip* functions the header calls are defined here.
#include <stdio.h>
#include <stdlib.h>

#include <map>
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
static void forget_event(void* e);      // (the ordering model below)
hipError_t hipEventDestroy(hipEvent_t e) { forget_event((void*)e); release((void*)e, "hipEventDestroy of an event that is not live"); return hipSuccess; }

// Streams and ordering: a MODEL of what the library relies on, not a claim about HIP beyond it.  A stream is an in-order queue with a vector clock
// (one component per stream); hipEventRecord snapshots the stream's clock into the event, hipStreamWaitEvent merges the event's snapshot AS IT IS AT
// THAT CALL into the waiter's clock -- a wait refers to the record that preceded it, a later record does not move it.  An event recorded on a second
// stream aborts: the rule csrc/gs_common.h's signal_to keeps by construction.
using Clock = std::vector<long>;
struct FakeStream { int id; Clock clock; };
struct FakeEvent { const FakeStream* home = nullptr; Clock snap; };
static std::vector<FakeStream*> g_streams;
static std::map<void*, FakeEvent> g_events;     // by event handle, while the event is live
static long g_records = 0, g_waits = 0;
static void forget_event(void* e) { g_events.erase(e); }

static void merge(Clock& into, const Clock& from) {
    if (into.size() < from.size()) into.resize(from.size(), 0);
    for (size_t k = 0; k < from.size(); ++k) if (from[k] > into[k]) into[k] = from[k];
}
static hipStream_t stream_create() {
    FakeStream* s = new FakeStream{ (int)g_streams.size(), Clock() };
    g_streams.push_back(s);
    for (FakeStream* t : g_streams) t->clock.resize(g_streams.size(), 0);
    return (hipStream_t)s;
}
static void streams_destroy() { for (FakeStream* s : g_streams) delete s; g_streams.clear(); }
// a piece of work enqueued on a stream: the stamp it gets is what it has behind it
struct Op { int stream; Clock at; };
static Op op(hipStream_t st) {
    FakeStream* s = (FakeStream*)st;
    s->clock[(size_t)s->id]++;
    return Op{ s->id, s->clock };
}
static bool before(const Op& a, const Op& b) {      // a happens-before b
    return b.at.size() > (size_t)a.stream && b.at[(size_t)a.stream] >= a.at[(size_t)a.stream] && !(a.stream == b.stream && a.at == b.at);
}

hipError_t hipEventRecord(hipEvent_t e, hipStream_t st) {
    if (!g_live.count((void*)e)) die("hipEventRecord on an event that is not live");
    FakeEvent& ev = g_events[(void*)e];
    if (ev.home && ev.home != (FakeStream*)st) die("an event was recorded on a second stream");
    ev.home = (FakeStream*)st;
    ev.snap = ev.home->clock;
    g_records++;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned int) {
    if (!g_live.count((void*)e)) die("hipStreamWaitEvent on an event that is not live");
    merge(((FakeStream*)st)->clock, g_events[(void*)e].snap);      // (never recorded: an empty snapshot, no ordering -- as in HIP)
    g_waits++;
    return hipSuccess;
}

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

// ---- gs::order_after and the sequences the library builds from it ----------------------------------------------------------------------------
// A context of the library: a stream and the one event that is recorded on it and nowhere else (gs_context::evOrder; gs::signal_to)
struct Ctx {
    hipStream_t stream = stream_create();
    Event evOrder;
    Ctx() { CHECK(evOrder.create(hipEventDisableTiming) == hipSuccess); }
};
static void signal_to(Ctx& from, hipStream_t waiter) { CHECK(gs::order_after(waiter, from.stream, from.evOrder) == hipSuccess); }

static void basic_ordering() {
    Ctx a, b;
    const Op early = op(a.stream), lone = op(b.stream);
    CHECK(before(early, op(a.stream)) && !before(early, lone) && !before(lone, early));      // (the model: in-order streams, unordered against each other)
    const long rec = g_records, waits = g_waits;
    signal_to(a, b.stream);
    CHECK(g_records == rec + 1 && g_waits == waits + 1);       // one record, one wait: nothing is created, nothing else is called
    const Op late = op(a.stream);                              // put on the signaller AFTER the call
    const Op after = op(b.stream);
    CHECK(before(early, after));
    CHECK(!before(late, after));
    CHECK(!before(lone, early) && !before(after, late));       // one direction only
    CHECK(before(lone, after));
}

// mirror_bits_to_lanes (gs_edit.hip) with two lanes: per lane, the lane waits for the owner, copies, the owner waits for the lane
static void mirror_sequence() {
    Ctx owner, lane[2];
    const Op frame[2] = { op(lane[0].stream), op(lane[1].stream) };    // a frame dealt to each lane before the delete
    const Op write = op(owner.stream);                                   // the delete's kernel
    Op copy[2];
    for (int k = 0; k < 2; ++k) {
        signal_to(owner, lane[k].stream);
        copy[k] = op(lane[k].stream);
        signal_to(lane[k], owner.stream);
    }
    const Op next = op(owner.stream);                                    // the owner's next write of the buffer
    const Op later[2] = { op(lane[0].stream), op(lane[1].stream) };    // frames dealt afterwards read the copies
    for (int k = 0; k < 2; ++k) {
        CHECK(before(write, copy[k]));
        CHECK(before(copy[k], next));
        CHECK(before(frame[k], copy[k]) && !before(copy[k], frame[k]));  // the frame keeps the bits of the time it was dealt
        CHECK(before(copy[k], later[k]) && before(write, later[k]));
        CHECK(!before(next, later[k]));                                  // (the lanes do not wait for what the owner does afterwards)
    }
}

// edit_before_move / edit_after_move (gs_edit.hip): the owner waits for every lane, the kernel runs, every lane waits for the owner
static void move_sequence() {
    Ctx owner, lane[3];
    Op earlier[3], later[3];
    for (int k = 0; k < 3; ++k) earlier[k] = op(lane[k].stream);
    for (int k = 0; k < 3; ++k) signal_to(lane[k], owner.stream);
    const Op kernel = op(owner.stream);
    for (int k = 0; k < 3; ++k) signal_to(owner, lane[k].stream);       // the owner's event, recorded once per lane
    const Op ownerNext = op(owner.stream);
    for (int k = 0; k < 3; ++k) later[k] = op(lane[k].stream);
    for (int k = 0; k < 3; ++k) {
        CHECK(before(earlier[k], kernel));
        CHECK(before(kernel, later[k]));
        CHECK(!before(ownerNext, later[k]));
        for (int j = 0; j < 3; ++j) CHECK(before(earlier[j], later[k]));  // through the kernel
    }
}

// The assumption the library relies on, written down as the model: a wait enqueued earlier keeps the snapshot of ITS record when the event is
// recorded again (a lane's evOrder every frame, the owner's once per lane in a fan-out).
static void re_recording() {
    Ctx a, b, c;
    const Op first = op(a.stream);
    signal_to(a, b.stream);
    const Op second = op(a.stream);
    signal_to(a, c.stream);                                    // the same event, recorded again on the same stream
    const Op third = op(a.stream);
    const Op onB = op(b.stream), onC = op(c.stream);
    CHECK(before(first, onB) && !before(second, onB) && !before(third, onB));       // b's wait was not moved by the second record
    CHECK(before(first, onC) && before(second, onC) && !before(third, onC));
    signal_to(a, b.stream);                                    // ... and a new wait sees the new record
    CHECK(before(third, op(b.stream)));
}

int main() {
    lifecycle<DevBuf<int>>();
    lifecycle<PinnedBuf<int>>();
    lifecycle<Event>();
    pinned_device_address();
    event_ring();
    commit_by_move();
    basic_ordering();
    mirror_sequence();
    move_sequence();
    re_recording();
    streams_destroy();
    if (!g_live.empty()) { fprintf(stderr, "FAIL: %zu handles still live at exit\n", g_live.size()); return 1; }
    printf("handles ok: %ld created, %ld released\n", g_created, g_released);
    printf("ordering ok: %ld records, %ld waits, none on a second stream\n", g_records, g_waits);
    return 0;
}
