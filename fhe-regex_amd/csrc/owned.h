// Move-only owners of the Device class's GPU resources: device and pinned memory, events,
// streams, and the pinned staging ring.  No HIP header: device.h is compiled by g++ too, so the
// calls that release and allocate are defined in device.hip.  Every destructor releases and
// ignores the error; every allocation that fails throws Error(FR_ERR_HIP) and leaves its
// holder empty.  SlotsOf owns arena slots the same way, for the layer above Device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

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

// Arena slots of a call or of a plan, given back when the owner goes.  Arena is anything with
// int alloc_slot() and void free_slot(int): Device in the library (device.h: Slots), a counting
// fake in tests/slot_owner_check.cpp.  Slots are taken and given back in ascending index; an
// entry of -1 is a slot handed on (take) and is skipped.
template <class Arena>
class SlotsOf {
  public:
    SlotsOf() = default;
    explicit SlotsOf(Arena& a, size_t n = 0) : a_(&a) { alloc(n); }
    SlotsOf(SlotsOf&& o) noexcept : a_(o.a_), s_(std::move(o.s_)) { o.s_.clear(); }
    SlotsOf& operator=(SlotsOf&& o) noexcept {
        if (this != &o) {
            drop();
            a_ = o.a_;
            s_ = std::move(o.s_);
            o.s_.clear();
        }
        return *this;
    }
    ~SlotsOf() { drop(); }
    Arena* arena() const { return a_; }
    size_t size() const { return s_.size(); }
    const int* data() const { return s_.data(); }
    int operator[](size_t i) const { return s_[i]; }
    // n fresh slots in place of the previous ones, all or nothing: empty after a throw
    void alloc(size_t n) {
        reset();
        try {
            s_.reserve(n);
            while (s_.size() < n) s_.push_back(a_->alloc_slot());
        } catch (...) {
            drop();
            throw;
        }
    }
    void reset() {
        for (int& s : s_)
            if (s >= 0) a_->free_slot(std::exchange(s, -1));
        s_.clear();
    }
    // slot i becomes the caller's
    int take(size_t i) { return std::exchange(s_[i], -1); }
    // every slot becomes the caller's (handles)
    std::vector<int> release() {
        std::vector<int> v = std::move(s_);
        s_.clear();
        return v;
    }

  private:
    void drop() noexcept {  // reset for destructors: an error of free_slot is ignored
        try {
            reset();
        } catch (...) {
            s_.clear();
        }
    }
    Arena* a_ = nullptr;
    std::vector<int> s_;
};

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
