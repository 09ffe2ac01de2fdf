// engine_impl.h - internal to the host runtime (engine.cpp and engine_tick.cpp, through engine_state.h): owning device /
// page-locked scratch and the small scoped helpers of its entry points.  Everything here stays out of the dynamic
// symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "../../include/kwok_engine.h"

// (the engine's sub-structs own device memory, so they have constructors and destructors)
#define KWOK_LOCAL __attribute__((visibility("hidden")))

#pragma GCC visibility push(hidden)
namespace kwok {

// An owning device pointer: freed by release() or the destructor, move-only; reads as a plain T*.
template <class T>
struct DevArr {
    T* p = nullptr;
    DevArr() = default;
    DevArr(const DevArr&) = delete;
    DevArr& operator=(const DevArr&) = delete;
    DevArr(DevArr&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevArr& operator=(DevArr&& o) noexcept {
        if (this != &o) reset(o.p), o.p = nullptr;
        return *this;
    }
    ~DevArr() { release(); }
    void release() { reset(nullptr); }
    void reset(T* q) {  // takes ownership of q
        if (p) (void)hipFree(p);
        p = q;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
// Its twin for the page-locked staging words (hipHostMalloc) the device's counters are copied into.
template <class T>
struct Pinned {
    T* p = nullptr;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// the headroom of a scratch group that grows, and the claim table of a batch of n records
// (a power of two >= 2n, so that it is at most half full)
inline size_t grown(size_t n) { return n + n / 4; }
inline size_t claim_size(size_t n) {
    size_t c = 64;
    while (c < 2 * n) c <<= 1;
    return c;
}

// Scratch arrays of one subsystem that share a capacity and grow together.  The arrays are DevArr
// members of the same struct, named once, where the group is declared; an array may hold a multiple
// or another function of the capacity (`count`).  A reserve past the capacity frees every array and
// allocates them again, zero-filled on the engine stream, with headroom: the contents are discarded
// and every pointer changes, so callers reserve before they hand a pointer to anything.
class DevGroup {
  public:
    struct Member {
        void** p;
        size_t elem;
        size_t (*count)(size_t cap);
        template <class T>
        Member(DevArr<T>& a, size_t (*c)(size_t) = nullptr) : p((void**)&a.p), elem(sizeof(std::conditional_t<std::is_void<T>::value, char, T>)), count(c) {}
    };
    DevGroup(size_t floor, std::initializer_list<Member> m) : floor_(floor), m_(m) {}
    DevGroup(const DevGroup&) = delete;
    DevGroup& operator=(const DevGroup&) = delete;
    size_t cap = 0;  // elements every array holds (times its factor); 0: nothing allocated, or a failed reserve
    // room for n elements: nothing if they fit, else max(n + n / 4, floor)
    int reserve(kwok_engine* e, size_t n) { return reserve(e, n, grown(n)); }
    // ... else max(want, floor), for the groups with a headroom of their own
    int reserve(kwok_engine* e, size_t need, size_t want);
    void release() {
        for (auto& m : m_) {
            if (*m.p) (void)hipFree(*m.p);
            *m.p = nullptr;
        }
        cap = 0;
    }

  private:
    size_t floor_;
    std::vector<Member> m_;
};
// array sizes that are not the capacity itself
inline size_t per_tile256(size_t cap) { return cap / 256 + 2; }
inline size_t twice(size_t cap) { return 2 * cap; }

// KWOK_INGEST_PROF: N device-side stamps of one call on the engine stream.  The events exist only
// while the engine profiles its ingests; stamp and elapsed are no-ops (0 ms) otherwise.
template <int N>
struct ProfEvents {
    hipEvent_t ev[N] = {};
    hipStream_t st;
    ProfEvents(bool on, hipStream_t s) : st(s) {  // (on: kwok_engine::iprof; s: the engine stream)
        if (on)
            for (auto& x : ev) (void)hipEventCreate(&x);
    }
    ProfEvents(const ProfEvents&) = delete;
    ProfEvents& operator=(const ProfEvents&) = delete;
    ~ProfEvents() {
        for (auto& x : ev)
            if (x) (void)hipEventDestroy(x);
    }
    bool on() const { return ev[0] != nullptr; }
    void stamp(int k) {
        if (ev[k]) (void)hipEventRecord(ev[k], st);
    }
    float elapsed(int a, int b) const {
        float ms = 0;
        if (ev[a] && ev[b]) (void)hipEventElapsedTime(&ms, ev[a], ev[b]);
        return ms;
    }
};

// a pointer of the engine set for a scope (what the ingest reads a framed batch's strings, uids or
// names from) and null again on every way out of it
template <class T>
struct ScopedPtr {
    const T*& slot;
    ScopedPtr(const T*& s, const T* p) : slot(s) { slot = p; }
    ScopedPtr(const ScopedPtr&) = delete;
    ScopedPtr& operator=(const ScopedPtr&) = delete;
    ~ScopedPtr() { slot = nullptr; }
};

}  // namespace kwok
#pragma GCC visibility pop
