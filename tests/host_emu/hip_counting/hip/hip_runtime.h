// TEST-ONLY stand-in for <hip/hip_runtime.h>: the few HIP calls csrc/hip_owned.h makes, on the host heap and counted, so that
// tests/host_emu/hip_owned_main.cpp can run the owners under AddressSanitizer without a GPU.  Memory comes from malloc (the
// sanitizer sees a double free or a leak), every call is logged in order, and the k-th allocation can be made to fail.
// Never part of the product; the stand-in next door (tests/host_emu/hip/) serves the device headers and is a different thing.
#ifndef SRT_TEST_HIP_COUNTING_RUNTIME_H
#define SRT_TEST_HIP_COUNTING_RUNTIME_H
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
typedef struct hip_counting_event* hipEvent_t;
typedef struct hip_counting_stream* hipStream_t;
enum : unsigned { hipHostMallocDefault = 0u, hipHostMallocMapped = 2u, hipEventDefault = 0u, hipEventDisableTiming = 2u, hipStreamNonBlocking = 1u };
struct uint2 { unsigned x, y; };
struct float4 { float x, y, z, w; };

// What the calls did: one letter per call in `log` (m hipMalloc, f hipFree, M hipHostMalloc, F hipHostFree, p
// hipHostGetDevicePointer, c hipMemcpy, e hipEventCreateWithFlags, d hipEventDestroy, s hipStreamCreateWithFlags, x
// hipStreamDestroy), the bytes of the last allocation and copy, and the blocks / events / streams alive.  fail_at = k: the k-th
// allocating call from now (m, M, e or s) fails; 0: none does.
struct HipCounting {
  std::string log;
  size_t last_alloc_bytes = 0, last_copy_bytes = 0;
  long device_blocks = 0, pinned_blocks = 0, events = 0, streams = 0;
  int fail_at = 0;
  bool allocation_fails() { return fail_at > 0 && --fail_at == 0; }
};
inline HipCounting& hip_counting() { static HipCounting c; return c; }

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
inline hipError_t hipMalloc(void** p, size_t bytes) {
  HipCounting& c = hip_counting();
  c.log += 'm'; c.last_alloc_bytes = bytes;
  if (c.allocation_fails()) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes ? bytes : 1);
  c.device_blocks++;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) { HipCounting& c = hip_counting(); c.log += 'f'; if (p) c.device_blocks--; std::free(p); return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
  HipCounting& c = hip_counting();
  c.log += 'M'; c.last_alloc_bytes = bytes;
  if (c.allocation_fails()) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes ? bytes : 1);
  c.pinned_blocks++;
  return hipSuccess;
}
inline hipError_t hipHostFree(void* p) { HipCounting& c = hip_counting(); c.log += 'F'; if (p) c.pinned_blocks--; std::free(p); return hipSuccess; }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { hip_counting().log += 'p'; *d = h; return hipSuccess; }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  HipCounting& c = hip_counting();
  c.log += 'c'; c.last_copy_bytes = bytes;
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  HipCounting& c = hip_counting();
  c.log += 'e';
  if (c.allocation_fails()) { *e = nullptr; return hipErrorOutOfMemory; }
  *e = static_cast<hipEvent_t>(std::malloc(1));
  c.events++;
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) { HipCounting& c = hip_counting(); c.log += 'd'; if (e) c.events--; std::free(e); return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  HipCounting& c = hip_counting();
  c.log += 's';
  if (c.allocation_fails()) { *s = nullptr; return hipErrorOutOfMemory; }
  *s = static_cast<hipStream_t>(std::malloc(1));
  c.streams++;
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) { HipCounting& c = hip_counting(); c.log += 'x'; if (s) c.streams--; std::free(s); return hipSuccess; }
#endif
