// Device memory of the host layers (moshii_api.hip, lbs_forward.hip, stagei.hip): who owns an allocation and how a call's buffers get
// to the device and back.  Host code only; compiles against the HIP headers and against tests/emu/fakehip.
//
//   DevArena  owns every pointer it hands out: a handle's arrays, a table that is replaced as a whole, the temporaries of one call.
//   Staging   the host-buffer / device-buffer choice of an entry (MOSHII_BUFFERS_DEVICE): in(), out(), finish().
//   Scratch   a grow-only buffer kept with a handle between calls; a different thing, it waits for its stream before it is reused.
//
// The rule they serve: a call that fails leaves no allocation of its own behind and no half-built table in a handle.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/moshii.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

extern "C" int moshii_internal_fail(int code, const char* msg);   // moshii_api.hip: sets moshii_last_error(), returns code

class DevArena {   // move-only; the destructor frees everything
  public:
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    DevArena(DevArena&& o) noexcept { swap(o); }
    DevArena& operator=(DevArena&& o) noexcept { DevArena old(std::move(*this)); swap(o); return *this; }   // `old` frees the old contents: how a table is replaced
    void swap(DevArena& o) noexcept { ptrs_.swap(o.ptrs_); std::swap(err_, o.err_); }
    ~DevArena() { clear(); }

    // Sticky: false once an allocation or copy has failed (err() says how); the calls after it return null without trying.
    bool ok() const { return err_ == hipSuccess; }
    hipError_t err() const { return err_; }
    size_t count() const { return ptrs_.size(); }
    void clear() {
        for (void* p : ptrs_) hipFree(p);
        ptrs_.clear();
        err_ = hipSuccess;
    }

    // n elements, uninitialised; never null on success (n == 0 gets one element, so that null always means failure)
    template <class T> T* alloc(size_t n) {
        if (!ok()) return nullptr;
        void* q = nullptr;
        err_ = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
        if (err_ != hipSuccess) return nullptr;
        ptrs_.push_back(q);
        return static_cast<T*>(q);
    }
    // a copy of host[0 .. n), made before the call returns; n == 0: null and no allocation (ok() tells that from a failure)
    template <class T> T* upload(const T* host, size_t n) {
        if (n == 0) return nullptr;
        T* q = alloc<T>(n);
        if (q && !note(hipMemcpy(q, host, n * sizeof(T), hipMemcpyHostToDevice))) return nullptr;
        return q;
    }
    // alloc(n) and a copy in stream order (the host array must live until the stream has passed it)
    template <class T> T* upload_async(const T* host, size_t n, hipStream_t stream) {
        T* q = alloc<T>(n);
        if (q && n && !note(hipMemcpyAsync(q, host, n * sizeof(T), hipMemcpyHostToDevice, stream))) return nullptr;
        return q;
    }
    // alloc(n), cleared in stream order
    template <class T> T* zeros(size_t n, hipStream_t stream) {
        T* q = alloc<T>(n);
        if (q && !note(hipMemsetAsync(q, 0, std::max<size_t>(n, 1) * sizeof(T), stream))) return nullptr;
        return q;
    }

  private:
    bool note(hipError_t e) { if (e != hipSuccess) err_ = e; return e == hipSuccess; }
    std::vector<void*> ptrs_;
    hipError_t err_ = hipSuccess;
};

// The buffers of one call of an entry that takes host or device pointers.  Host mode (no MOSHII_BUFFERS_DEVICE in flags): inputs are
// copied into temporaries, outputs get temporaries and are copied back by finish(); the temporaries go with the object.  Device mode:
// every pointer passes through untouched and nothing is allocated.  A null pointer (an optional array) stays null in both modes.
class Staging {
  public:
    Staging(uint32_t flags, hipStream_t stream) : dev_((flags & MOSHII_BUFFERS_DEVICE) != 0), stream_(stream) {}
    bool device() const { return dev_; }
    bool ok() const { return mem_.ok(); }
    hipError_t err() const { return mem_.err(); }
    DevArena& mem() { return mem_; }   // further temporaries of the call

    template <class T> const T* in(const T* p, size_t n) { return (dev_ || !p) ? p : mem_.upload(p, n); }
    template <class T> T* out(T* p, size_t n) {
        if (dev_ || !p) return p;
        T* d = mem_.alloc<T>(n);
        if (d) back_.push_back(Back{p, d, n * sizeof(T)});
        return d;
    }
    // host mode: waits for the stream, then copies every out() back, once; device mode: nothing
    hipError_t finish() {
        if (dev_) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream_);
        for (size_t i = 0; e == hipSuccess && i < back_.size(); ++i) e = hipMemcpy(back_[i].host, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost);
        back_.clear();
        return e;
    }

  private:
    struct Back { void* host; const void* dev; size_t bytes; };
    bool dev_;
    hipStream_t stream_;
    DevArena mem_;
    std::vector<Back> back_;
};

struct Scratch {   // growable device buffer reused across calls (small control data)
    char* ptr = nullptr;
    size_t cap = 0;
    hipStream_t last_stream = nullptr;
    bool used = false;
    int reserve(size_t bytes) {
        if (used) { hipStreamSynchronize(last_stream); used = false; }
        if (bytes <= cap) return MOSHII_OK;
        if (ptr) hipFree(ptr);
        ptr = nullptr; cap = 0;
        size_t want = std::max<size_t>(bytes, 1 << 16);
        if (hipMalloc((void**)&ptr, want) != hipSuccess) return moshii_internal_fail(MOSHII_ERR_HIP, "scratch hipMalloc failed");
        cap = want;
        return MOSHII_OK;
    }
    int reserve(size_t bytes, hipStream_t stream) {   // ... and the buffer is in use on `stream` until the next reserve
        const int rc = reserve(bytes);
        if (rc == MOSHII_OK) { used = true; last_stream = stream; }
        return rc;
    }
    ~Scratch() { if (ptr) hipFree(ptr); }
};
