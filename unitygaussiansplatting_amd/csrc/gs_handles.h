// gs_handles.h -- move-only owners of one device allocation, one pinned host allocation, one event.  Host-only, header-only (HIP runtime API
// + the standard library), so that it also compiles with a plain host compiler (tests/handles_harness.cpp).
// A handle converts to the raw pointer / event it owns, so kernel launches, copies and pointer arithmetic read as they would with the raw pointer.
// No destructor synchronises: whoever destroys an object that work in flight may still use waits for its streams first (the gs_*_destroy functions).
// Several resources that are made or grown together are built in local handles and moved into their owner after the last step has succeeded.
// order_after(), at the end, puts one stream behind another through an Event: the record and the wait in one step.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace gs {

template <class T>
class DevBuf {                                   // one hipMalloc allocation
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t bytes) {             // frees what it held; null on failure
        reset();
        const hipError_t e = hipMalloc((void**)&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() { if (p_) { (void)hipFree(p_); p_ = nullptr; } }
    T* get() const { return p_; }
    operator T*() const { return p_; }
private:
    T* p_ = nullptr;
};

template <class T>
class PinnedBuf {                                // one hipHostMalloc allocation (+ its device-side address when it is mapped)
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), dev_(o.dev_) { o.p_ = o.dev_ = nullptr; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; dev_ = o.dev_; o.p_ = o.dev_ = nullptr; }
        return *this;
    }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t bytes, unsigned flags) {
        reset();
        hipError_t e = hipHostMalloc((void**)&p_, bytes, flags);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        if (flags & hipHostMallocMapped) {
            e = hipHostGetDevicePointer((void**)&dev_, p_, 0);
            if (e != hipSuccess) reset();
        }
        return e;
    }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = dev_ = nullptr; }
    T* get() const { return p_; }
    T* device() const { return dev_; }           // null unless allocated with hipHostMallocMapped
    operator T*() const { return p_; }
private:
    T* p_ = nullptr;
    T* dev_ = nullptr;
};

class Event {                                    // one hipEvent_t
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
        return *this;
    }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { reset(); }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&e_, flags);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    void reset() { if (e_) { (void)hipEventDestroy(e_); e_ = nullptr; } }
    operator hipEvent_t() const { return e_; }
private:
    hipEvent_t e_ = nullptr;
};

// Everything enqueued on `waiter` after this call starts only after everything enqueued on `signaller` before it has finished.
// ev must exist.  The wait refers to THIS record: a later record of ev (on the same stream) does not move it.
inline hipError_t order_after(hipStream_t waiter, hipStream_t signaller, Event& ev) {
    const hipError_t e = hipEventRecord(ev, signaller);
    return e != hipSuccess ? e : hipStreamWaitEvent(waiter, ev, 0);
}

} // namespace gs
