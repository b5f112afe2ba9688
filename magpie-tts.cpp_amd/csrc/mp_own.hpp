// Owners of the GPU resources the host side holds (mp_runtime.hip, mp_model.hip,
// mp_codec.hip): device blocks, a pinned host buffer, an event, a stream. Each is move-only
// and releases in its destructor, so an early return releases what it made and a struct
// that holds owners needs no hand-written free list. Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

// `expr` (a hipError_t) failed: its text into `errstr`, MP_ERR_HIP to the caller
#define MP_HIPCHK_TO(errstr, expr)                                               \
    do {                                                                         \
        hipError_t e_ = (expr);                                                  \
        if (e_ != hipSuccess) {                                                  \
            (errstr) = std::string(#expr) + " failed: " + hipGetErrorString(e_); \
            return MP_ERR_HIP;                                                   \
        }                                                                        \
    } while (0)

namespace mp {

// Device blocks, one hipMalloc each, released together (clear or destruction).
class DevBlocks {
    std::vector<void *> v_;
  public:
    DevBlocks() = default;
    DevBlocks(DevBlocks &&o) noexcept { v_.swap(o.v_); }
    DevBlocks &operator=(DevBlocks &&o) noexcept { v_.swap(o.v_); return *this; }  // o's destructor releases ours
    ~DevBlocks() { clear(); }
    void clear() {
        for (void *p : v_) hipFree(p);
        v_.clear();
    }
    bool empty() const { return v_.empty(); }
    // a block of exactly `nbytes`
    template <class T> hipError_t bytes(T **p, size_t nbytes) {
        const hipError_t e = hipMalloc((void **)p, nbytes);
        if (e == hipSuccess) v_.push_back((void *)*p);
        return e;
    }
    // `count` elements and a 256-byte tail (kernels' vector loads may run past the last row)
    template <class T> hipError_t get(T **p, size_t count) { return bytes(p, count * sizeof(T) + 256); }
    // the same, zero-filled on stream s (hand-off granules start without a tag)
    template <class T> hipError_t get_zeroed(T **p, size_t count, hipStream_t s) {
        const hipError_t e = get(p, count);
        return e != hipSuccess ? e : hipMemsetAsync(*p, 0, count * sizeof(T) + 256, s);
    }
};

// A pinned host buffer that grows on demand.
struct Pinned {
    void *p = nullptr;
    size_t cap = 0;  // bytes
    Pinned() = default;
    Pinned(Pinned &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Pinned &operator=(Pinned &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~Pinned() { if (p) hipHostFree(p); }
    hipError_t reserve(size_t nbytes) {  // at least nbytes; a larger buffer replaces the old one (contents dropped)
        if (nbytes <= cap) return hipSuccess;
        *this = Pinned{};
        const hipError_t e = hipHostMalloc(&p, nbytes, hipHostMallocDefault);
        if (e == hipSuccess) cap = nbytes;
        return e;
    }
    template <class T> T *as() const { return (T *)p; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) hipStreamDestroy(s); }
    hipError_t create(int priority = 0) {  // non-blocking; 0: the default priority
        return s ? hipSuccess : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority);
    }
    operator hipStream_t() const { return s; }
};

}  // namespace mp
