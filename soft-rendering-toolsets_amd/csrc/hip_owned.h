// The owners of what the host code gets from HIP: device memory, pinned host memory, events and streams.  Move-only; a member of one
// of these types is all a struct needs to say about a resource - no free list mirrors it.  An empty owner makes no HIP call, in its
// destructor, reset() and moves alike (host-only contexts live on machines without a GPU), and no owner sets the device: the
// entry points have done so before they touch anything.  A struct whose owners live on several devices (the group of pt_group.cpp)
// therefore resets each of them under its own device before it is deleted, and leaves its destructor nothing to free.
#ifndef SRT_HIP_OWNED_H
#define SRT_HIP_OWNED_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "srt_raster.h"

namespace srt {

int fail(int status, const char* fmt, ...);   // srt_common.h

// Live objects that hold a resource, per type (srt_pt_live_resources): what a test compares before and after.
enum OwnedKind { OWNED_DEVICE = 0, OWNED_PINNED = 1, OWNED_EVENT = 2, OWNED_STREAM = 3, OWNED_KINDS = 4 };
inline std::atomic<uint64_t>& owned_live(OwnedKind k) {
  static std::atomic<uint64_t> live[OWNED_KINDS];
  return live[k];
}
inline void owned_count(OwnedKind k, bool born) {
  if (born) owned_live(k).fetch_add(1, std::memory_order_relaxed);
  else owned_live(k).fetch_sub(1, std::memory_order_relaxed);
}

template <typename T> struct OwnedElem { static constexpr size_t size = sizeof(T); };
template <> struct OwnedElem<void> { static constexpr size_t size = 1; };   // DeviceBuffer<void>: bytes, typed where a kernel is launched

// A device array and its capacity in elements.
template <typename T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) { (void)hipFree(p_); owned_count(OWNED_DEVICE, false); }
    p_ = nullptr; cap_ = 0;
  }
  // At least `need` elements: grown (never shrunk) by freeing and allocating anew; what it held is gone then.
  int ensure(size_t need) {
    if (cap_ >= need && p_) return SRT_OK;
    reset();
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, need * OwnedElem<T>::size);
    if (e != hipSuccess) return srt::fail(SRT_ERR_HIP, "hipMalloc of %zu bytes: %s", need * OwnedElem<T>::size, hipGetErrorString(e));
    if (p) { p_ = static_cast<T*>(p); cap_ = need; owned_count(OWNED_DEVICE, true); }
    return SRT_OK;
  }
  // A fresh array holding src[0, n) (one element of room for an empty source), copied before the call returns.
  int upload(const T* src, size_t n) {
    reset();
    const int st = ensure(n ? n : 1);
    if (st != SRT_OK || !n) return st;
    const hipError_t e = hipMemcpy(p_, src, n * OwnedElem<T>::size, hipMemcpyHostToDevice);
    if (e == hipSuccess) return SRT_OK;
    reset();
    return srt::fail(SRT_ERR_HIP, "hipMemcpy of %zu bytes to the device: %s", n * OwnedElem<T>::size, hipGetErrorString(e));
  }
  template <typename U>
  int upload(const std::vector<U>& src) {
    static_assert(sizeof(U) == OwnedElem<T>::size, "element type");
    return upload(static_cast<const T*>(src.data()), src.size());
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// Pinned host memory (hipHostMalloc) and, for a mapped allocation, the address the device sees it under.
template <typename T>
class PinnedBuffer {
 public:
  PinnedBuffer() = default;
  PinnedBuffer(const PinnedBuffer&) = delete;
  PinnedBuffer& operator=(const PinnedBuffer&) = delete;
  PinnedBuffer(PinnedBuffer&& o) noexcept : p_(o.p_), dev_(o.dev_), cap_(o.cap_) { o.p_ = o.dev_ = nullptr; o.cap_ = 0; }
  PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; dev_ = o.dev_; cap_ = o.cap_; o.p_ = o.dev_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~PinnedBuffer() { reset(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  T* device() const { return dev_; }          // NULL unless made with hipHostMallocMapped
  size_t capacity() const { return cap_; }
  void reset() {
    if (p_) { (void)hipHostFree(p_); owned_count(OWNED_PINNED, false); }
    p_ = dev_ = nullptr; cap_ = 0;
  }
  // As DeviceBuffer::ensure; `flags` are hipHostMalloc's.
  int ensure(size_t need, unsigned flags = hipHostMallocDefault) {
    if (cap_ >= need && p_) return SRT_OK;
    reset();
    void* p = nullptr;
    hipError_t e = hipHostMalloc(&p, need * sizeof(T), flags);
    if (e != hipSuccess) return srt::fail(SRT_ERR_HIP, "hipHostMalloc of %zu bytes: %s", need * sizeof(T), hipGetErrorString(e));
    if (!p) return SRT_OK;
    p_ = static_cast<T*>(p); cap_ = need; owned_count(OWNED_PINNED, true);
    if (flags & hipHostMallocMapped) {
      void* d = nullptr;
      if ((e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) {
        reset();
        return srt::fail(SRT_ERR_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
      }
      dev_ = static_cast<T*>(d);
    }
    return SRT_OK;
  }

 private:
  T *p_ = nullptr, *dev_ = nullptr;
  size_t cap_ = 0;
};

// One hipEvent_t.
class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
    return *this;
  }
  ~Event() { reset(); }

  operator hipEvent_t() const { return e_; }
  void reset() {
    if (e_) { (void)hipEventDestroy(e_); owned_count(OWNED_EVENT, false); }
    e_ = nullptr;
  }
  // A new event (`flags` are hipEventCreateWithFlags'); one that is there already stays.
  int create(unsigned flags = hipEventDefault) {
    if (e_) return SRT_OK;
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) { e_ = nullptr; return srt::fail(SRT_ERR_HIP, "hipEventCreateWithFlags: %s", hipGetErrorString(e)); }
    owned_count(OWNED_EVENT, true);
    return SRT_OK;
  }

 private:
  hipEvent_t e_ = nullptr;
};
using EventPair = std::pair<Event, Event>;   // a timing bracket

// One hipStream_t.  (Whoever holds it synchronises it before it goes: reset() only destroys.)
class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept {
    if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; }
    return *this;
  }
  ~Stream() { reset(); }

  operator hipStream_t() const { return s_; }
  void reset() {
    if (s_) { (void)hipStreamDestroy(s_); owned_count(OWNED_STREAM, false); }
    s_ = nullptr;
  }
  // A new stream (`flags` are hipStreamCreateWithFlags'); one that is there already stays.
  int create(unsigned flags) {
    if (s_) return SRT_OK;
    const hipError_t e = hipStreamCreateWithFlags(&s_, flags);
    if (e != hipSuccess) { s_ = nullptr; return srt::fail(SRT_ERR_HIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(e)); }
    owned_count(OWNED_STREAM, true);
    return SRT_OK;
  }

 private:
  hipStream_t s_ = nullptr;
};

}  // namespace srt

#endif
