// srt_pt_hit_device: scene.hit for rays that lie in device memory, results into device memory, enqueue-only.
//
// Two routes, the same bits on both:
//   cast      pack (one lane per ray: the 32-byte request of pt_stream.h's CastParams, the identity list entry, the queue's counters)
//             -> pt_cast_kernel<false, false> (launched by pt.hip: query_cast_launch) -> resolve (one lane per ray: the hit word back
//             into a Hit, the surface only when the record is wanted).  For the scenes query_cast_applies() names, in chunks.
//   per lane  the nested walk of pt_trace.h (or, under kernel mode 5, the flattened one of pt_flat.h) straight from the caller's
//             arrays - what srt_pt_hit runs on its uploaded copies.  Every other scene, and kernel modes 1 and 4.
// Both end in write_trace(): one writer of the record, the ids and the flag.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "pt_context.h"
#include "pt_device.h"
#include "srt_pt_debug.h"

#include "pt_trace.h"
#include "pt_flat.h"
#include "pt_queue.h"

namespace srt {

// Rays per cast launch: a larger call is cut into chunks enqueued back to back, so that the scratch stays at 44 B x this (184 MB)
// plus the spill columns.  SRT_HIT_CHUNK overrides it (diagnostic; read at every call).
constexpr size_t kHitChunk = 4u << 20;
// Calls of fewer rays than this take the per-lane walk under the automatic kernel mode: a persistent launch has a fixed cost, and
// 2^19 is the measured crossover for incoherent rays (262 144: 1.01x and 0.89x the per-lane walk's rate on the 74-object and the
// 131 072-triangle scene, 524 288: 1.44x and 1.00x, 2^22: 2.7x and 2.1x; DESIGN.md "Ray queries from device memory").  Kernel
// modes 2, 3, 6 and 7 always take the cast kernel where it applies.
constexpr size_t kHitCastMinRays = 1u << 19;

// What a query leaves per ray, from the closest hit `h` of world ray `r`: Trace as srt_pt_hit lays it out (nine zeros on a miss),
// {insertion index of the object, the triangle's place in the mesh's own primitive order} and the shadow-ray byte.
SRT_DEV void write_trace(const DScene& S, const Hit& h, const Ray& r, size_t i, float* __restrict__ out9, uint32_t* __restrict__ ids,
                         uint8_t* __restrict__ flag) {
  if (out9) {
    float* o = out9 + 9 * i;
    for (int k = 0; k < 9; k++) o[k] = 0.0f;
    if (h.hit) {
      const Surface sf = surface_of(S, h, r);
      o[0] = 1.0f; o[1] = h.dist;
      o[2] = sf.position.x; o[3] = sf.position.y; o[4] = sf.position.z;
      o[5] = sf.normal.x; o[6] = sf.normal.y; o[7] = sf.normal.z;
      o[8] = (float)S.objects[h.obj].material;
    }
  }
  if (ids) {
    uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu;
    if (h.hit) {
      const Object& ob = S.objects[h.obj];
      a = ob.id - 1u;
      if (ob.kind != OBJ_SPHERE) b = h.tri - ob.tri_base;
    }
    ids[2 * i] = a; ids[2 * i + 1] = b;
  }
  if (flag) flag[i] = h.hit ? 1 : 0;
}

SRT_DEV Ray load_query_ray(const float* __restrict__ org, const float* __restrict__ dir, const float* __restrict__ bounds, size_t j) {
  Ray r;
  r.o = v3(org[3 * j], org[3 * j + 1], org[3 * j + 2]);
  r.d = v3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  r.b0 = bounds ? bounds[2 * j] : 0.0f;
  r.b1 = bounds ? bounds[2 * j + 1] : INFINITY;
  return r;
}

// The per-lane route.  FLAT: through flat_trace3 (pt_flat.h) in batch slot i % 3, as pt_hit_kernel does it.
template <bool FLAT>
__global__ void pt_hit_lane_kernel(DScene S, const float* __restrict__ org, const float* __restrict__ dir, const float* __restrict__ bounds,
                                   uint32_t n, float* __restrict__ out9, uint32_t* __restrict__ ids, uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;                     // every lane stays in the kernel: flat_trace3 is a wave-wide loop
  const Ray r = load_query_ray(org, dir, bounds, live ? i : 0);
  Counters cnt;
  Hit h;
  if (FLAT) {
    const uint32_t slot = i % 3u;
    Hit res[3];
    flat_trace3(S, r.o, r.d, r.d, r.d, r.b0, r.b1, live && slot == 0, live && slot == 1, live && slot == 2, res[0], res[1], res[2]);
    h = slot == 0 ? res[0] : (slot == 1 ? res[1] : res[2]);
  } else {
    h = scene_hit<false>(S, r, cnt);
  }
  if (live) write_trace(S, h, r, i, out9, ids, flag);
}

// Cast route, stage 1: ray i of the chunk as the request at queue position i, the list entry that names it, and - lane 0 - the
// queue's length and head (the words pt_cast_kernel reads as *P.nrays and *P.head).
__global__ __launch_bounds__(256) void pt_hit_pack_kernel(const float* __restrict__ org, const float* __restrict__ dir, const float* __restrict__ bounds,
                                                          uint32_t n, float4* __restrict__ req, uint32_t* __restrict__ ray_id,
                                                          uint32_t* __restrict__ nrays, uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0u) { *nrays = n; *head = 0u; }
  if (i >= n) return;
  const Ray r = load_query_ray(org, dir, bounds, i);
  nt_store_ray(req, 2u * (size_t)i, r.o.x, r.o.y, r.o.z, r.b0);
  nt_store_ray(req, 2u * (size_t)i + 1u, r.d.x, r.d.y, r.d.z, r.b1);
  __builtin_nontemporal_store(i, ray_id + i);
}

// Cast route, stage 3: the hit word {distance bits, object << obj_shift | triangle, or 0xFFFFFFFF} back into a Hit.
__global__ __launch_bounds__(256) void pt_hit_resolve_kernel(DScene S, const float* __restrict__ org, const float* __restrict__ dir,
                                                             const float* __restrict__ bounds, const uint2* __restrict__ hits, uint32_t n,
                                                             uint32_t obj_shift, float* __restrict__ out9, uint32_t* __restrict__ ids,
                                                             uint8_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint2 w = nt_load_hit(hits, i);
  Hit h;
  h.hit = w.y != 0xFFFFFFFFu;
  h.dist = h.hit ? __uint_as_float(w.x) : 0.0f;
  h.obj = h.hit ? (w.y >> obj_shift) : 0u;
  h.tri = h.hit ? (w.y & ((1u << obj_shift) - 1u)) : 0u;
  if (!out9 && !ids) { flag[i] = h.hit ? 1 : 0; return; }   // the shadow-ray question alone: the rays are not read again
  const Ray r = load_query_ray(org, dir, bounds, i);
  write_trace(S, h, r, i, out9, ids, flag);
}

}  // namespace srt

using namespace srt;

extern "C" {

int srt_pt_hit_device(srt_pt* pt, void* stream, const float* d_origins, const float* d_dirs, const float* d_bounds, size_t n, float* d_out9,
                      uint32_t* d_ids, uint8_t* d_hit) {
  const char* what = "srt_pt_hit_device";
  if (!pt) return srt::fail(SRT_ERR_INVALID, "%s: NULL context", what);
  if (n && (!d_origins || !d_dirs)) return srt::fail(SRT_ERR_INVALID, "%s: NULL origins or directions", what);
  if (!d_out9 && !d_ids && !d_hit) return srt::fail(SRT_ERR_INVALID, "%s: no output asked for (d_out9, d_ids and d_hit are all NULL)", what);
  if (!pt->committed) return not_committed(what);         // (no settle(): the query reads the live device scene)
  if (n > 0x7fffffffull) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: too many rays in one call", what);
  if (n == 0) return SRT_OK;
  if (pt->device < 0) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the rays are traced on the device only; this context is host-only", what);
  SRT_HIP(hipSetDevice(pt->device));
  hipStream_t s = (hipStream_t)stream;
  const int mode = pt->kernel_mode;
  const DScene S = device_scene(pt);
  if (mode == 5 && !flat_walk_fits(pt->built.flat)) return srt::fail(SRT_ERR_UNSUPPORTED, "the flattened walk needs 1..31 objects");
  const bool cast = mode != 1 && mode != 4 && mode != 5 && (mode != 0 || n >= kHitCastMinRays) && query_cast_applies(pt, mode == 0);
  if (!cast) {
    const dim3 grid((unsigned)((n + 63) / 64)), block(64);
    if (mode == 5) pt_hit_lane_kernel<true><<<grid, block, 0, s>>>(S, d_origins, d_dirs, d_bounds, (uint32_t)n, d_out9, d_ids, d_hit);
    else pt_hit_lane_kernel<false><<<grid, block, 0, s>>>(S, d_origins, d_dirs, d_bounds, (uint32_t)n, d_out9, d_ids, d_hit);
    SRT_HIP(hipGetLastError());
    pt->hit_device_paths[mode == 5 ? 2 : 1]++;
    return SRT_OK;
  }
  size_t chunk = kHitChunk;
  if (const char* v = getenv("SRT_HIT_CHUNK")) { const long long c = atoll(v); if (c >= 1) chunk = (size_t)c; }
  if (chunk > n) chunk = n;
  srt_pt::QueryBuffers* Q = nullptr;
  uint32_t *nrays = nullptr, *head = nullptr, obj_shift = 0;
  int st;
  if ((st = query_cast_prepare(pt, s, chunk, &Q, &nrays, &head, &obj_shift)) != SRT_OK) return st;
  for (size_t first = 0; first < n; first += chunk) {
    const uint32_t m = (uint32_t)(n - first < chunk ? n - first : chunk);
    const float* org = d_origins + 3 * first;
    const float* dir = d_dirs + 3 * first;
    const float* bounds = d_bounds ? d_bounds + 2 * first : nullptr;
    const dim3 grid((m + 255u) / 256u), block(256);
    pt_hit_pack_kernel<<<grid, block, 0, s>>>(org, dir, bounds, m, Q->d_req, Q->d_ray_id, nrays, head);
    SRT_HIP(hipGetLastError());
    if ((st = query_cast_launch(pt, s, *Q)) != SRT_OK) return st;
    pt_hit_resolve_kernel<<<grid, block, 0, s>>>(S, org, dir, bounds, Q->d_hits, m, obj_shift, d_out9 ? d_out9 + 9 * first : nullptr,
                                                 d_ids ? d_ids + 2 * first : nullptr, d_hit ? d_hit + first : nullptr);
    SRT_HIP(hipGetLastError());
  }
  pt->hit_device_paths[0]++;
  return SRT_OK;
}

int srt_pt_hit_device_paths(srt_pt* pt, uint64_t out[3]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_hit_device_paths: NULL argument");
  for (int k = 0; k < 3; k++) out[k] = pt->hit_device_paths[k];
  return SRT_OK;
}

}  // extern "C"
