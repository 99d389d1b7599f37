// engine_internal.h — helpers shared by the Engine's translation units (engine.cpp, engine_queue.cpp).
#pragma once
#include <algorithm>
#include <utility>

#include "engine.h"

namespace q3t {

// a HIP event for the length of a scope
struct Event {
    hipEvent_t ev = nullptr;
    explicit Event(unsigned flags = hipEventDefault) { hipEventCreateWithFlags(&ev, flags); }
    ~Event() { if (ev) hipEventDestroy(ev); }
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    operator hipEvent_t() const { return ev; }   // null if the creation failed: the first use reports it
};
// runs f on every exit of the scope
template <class F>
struct ScopeExit {
    F f;
    explicit ScopeExit(F fn) : f(std::move(fn)) {}
    ~ScopeExit() { f(); }
    ScopeExit(const ScopeExit &) = delete;
    ScopeExit &operator=(const ScopeExit &) = delete;
};

template <class T>
T *Engine::dalloc(size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
    allocs_.push_back(p);
    // zeroed on the context's own stream, and drained before any other stream (the admission stream, or a
    // synchronous null-stream copy into the buffer right after this call) can touch it: without the ordering a first
    // launch could read what a previous context freed in the same process left in this memory (DESIGN §2e').  Only
    // this context's stream is waited for, never the device.
    if (hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess) {
        set_error("dalloc: zeroing failed");
        return nullptr;
    }
    return static_cast<T *>(p);
}

}  // namespace q3t
