// Move-only owners of the Device class's GPU resources: device and pinned memory, events,
// streams, and the pinned staging ring.  No HIP header: device.h is compiled by g++ too, so the
// calls that release and allocate are defined in device.hip.  Every destructor releases and
// ignores the error; every allocation that fails throws Error(FR_ERR_HIP) and leaves its
// holder empty.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>

// the runtime's handle types, as hip/hip_runtime_api.h declares them
typedef struct ihipStream_t* hipStream_t;
typedef struct ihipEvent_t* hipEvent_t;

namespace fr {
namespace gpu {

// device.hip
void* dev_alloc(size_t bytes);
void dev_free(void* p) noexcept;
void* pinned_alloc(size_t bytes);
void pinned_free(void* p) noexcept;
hipEvent_t event_create(unsigned flags);
void event_destroy(hipEvent_t e) noexcept;
hipStream_t stream_create();  // non-blocking
void stream_destroy(hipStream_t s) noexcept;

// n elements of T from Alloc, given back to Free
template <class T, void* (*Alloc)(size_t), void (*Free)(void*) noexcept>
class Buf {
  public:
    Buf() = default;
    explicit Buf(size_t n) { alloc(n); }
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~Buf() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }  // elements
    explicit operator bool() const { return p_ != nullptr; }
    void alloc(size_t n) {  // the previous contents go first; empty after a failed allocation
        reset();
        p_ = static_cast<T*>(Alloc(n * sizeof(T)));
        n_ = n;
    }
    void reset() {
        if (p_) Free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* release() {
        n_ = 0;
        return std::exchange(p_, nullptr);
    }
    // at least n elements: `first` to begin with, then doubled; true if it reallocated (the
    // contents are lost, and the caller has made sure nothing in flight reads them)
    bool grow(size_t n, size_t first) {
        if (n <= n_) return false;
        size_t cap = n_ ? n_ : first;
        while (cap < n) cap *= 2;
        alloc(cap);
        return true;
    }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T>
using DevBuf = Buf<T, dev_alloc, dev_free>;
template <class T>
using PinnedBuf = Buf<T, pinned_alloc, pinned_free>;

template <class H, void (*Destroy)(H) noexcept>
class Handle {
  public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() {
        if (h_) Destroy(h_);
        h_ = nullptr;
    }

  protected:
    H h_ = nullptr;
};
struct Event : Handle<hipEvent_t, event_destroy> {
    Event() = default;
    explicit Event(unsigned flags) { h_ = event_create(flags); }
};
struct Stream : Handle<hipStream_t, stream_destroy> {
    void create() {  // non-blocking
        reset();
        h_ = stream_create();
    }
};

// Pinned staging ring: a device buffer rewritten in stream order from two pinned buffers that
// take turns, so the host never waits for the stream -- a pinned side is rewritten only after
// the event behind its previous copy completed.  The events are created at the first reserve
// and start out never recorded, which HIP counts as complete.
class StagingBytes {
  public:
    // at least `bytes` (`first` to begin with, then doubled); a reallocation first waits for
    // the stream, and leaves all three buffers empty if any allocation fails
    void reserve(size_t bytes, size_t first, hipStream_t s);
    void* acquire();  // the other pinned side, free to write
    void commit(size_t bytes, hipStream_t s);  // the acquired side -> device(), stream-ordered
    uint8_t* device() const { return d_.get(); }
    const void* last() const { return h_[side_].get(); }  // the pinned side committed last

  private:
    DevBuf<uint8_t> d_;
    PinnedBuf<uint8_t> h_[2];
    Event ev_[2];
    int side_ = 0;
};
template <class T>
class StagingRing {
  public:
    void reserve(size_t n, size_t first, hipStream_t s) { b_.reserve(n * sizeof(T), first * sizeof(T), s); }
    T* acquire() { return static_cast<T*>(b_.acquire()); }
    void commit(size_t n, hipStream_t s) { b_.commit(n * sizeof(T), s); }
    T* device() const { return reinterpret_cast<T*>(b_.device()); }
    const T* last() const { return static_cast<const T*>(b_.last()); }

  private:
    StagingBytes b_;
};

}  // namespace gpu
}  // namespace fr
