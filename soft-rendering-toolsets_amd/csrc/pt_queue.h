// The ray queue's memory accesses, for every unit that fills or drains one: the streamed render forms (pt_stream.h, pt_wave.h) and the
// device ray queries (pt_hit_device.hip).  No kernel is defined here, so any unit may include it.
#ifndef SRT_PT_QUEUE_H
#define SRT_PT_QUEUE_H

#include "pt_device.h"

namespace srt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
// The streamed forms' queue traffic - rays, list entries, hits, saved path state - passes through memory once per generation:
// non-temporal accesses, so that it does not push the scene out of L2.
SRT_DEV void nt_store_ray(float4* plane, size_t i, float x, float y, float z, float w) { __builtin_nontemporal_store(f32x4{x, y, z, w}, reinterpret_cast<f32x4*>(plane) + i); }
SRT_DEV uint2 nt_load_hit(const uint2* hits, size_t i) { const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(hits) + i); return make_uint2(v.x, v.y); }

}  // namespace srt

#endif
