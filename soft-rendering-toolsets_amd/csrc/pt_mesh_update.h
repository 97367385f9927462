// Per-triangle work of srt_pt_update_mesh as device functions: Triangle::bbox from a mesh's vertex and index arrays, and the
// Tri / TriNrm / packed records of one triangle slot.  pt_mesh_update.hip runs them one lane per triangle; the host emulation
// (tests/host_emu/update_host.cpp) compiles this header with g++ and compares with triangle_box / append_triangles of
// pt_scene.cpp, which they restate: the same comparisons in the same operand order (the sign of a zero bound is part of the
// contract of pt_bvh_device.hip) and the same fp32 subtractions.  Nothing in here multiplies, so nothing can contract.
#ifndef SRT_PT_MESH_UPDATE_H
#define SRT_PT_MESH_UPDATE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_scene.h"

namespace srt {

// std::min({a, b, c}) / std::max({a, b, c}): the first smallest / first largest element
__device__ __forceinline__ float std_min3(float a, float b, float c) {
  float m = a;
  if (b < m) m = b;
  if (c < m) m = c;
  return m;
}
__device__ __forceinline__ float std_max3(float a, float b, float c) {
  float m = a;
  if (m < b) m = b;
  if (m < c) m = c;
  return m;
}

// Triangle::bbox (student/tri_mesh.cpp:7-30) of triangle t: box6 = {mn[3], mx[3]}; zero-extent axes are widened by +1 on the max side.
__device__ __forceinline__ void mesh_triangle_box(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t t, float box6[6]) {
  const float* p0 = pos + 3 * (size_t)idx[3 * (size_t)t];
  const float* p1 = pos + 3 * (size_t)idx[3 * (size_t)t + 1];
  const float* p2 = pos + 3 * (size_t)idx[3 * (size_t)t + 2];
  for (int a = 0; a < 3; a++) {
    const float lo = std_min3(p0[a], p1[a], p2[a]);
    float hi = std_max3(p0[a], p1[a], p2[a]);
    hi = (lo >= hi) ? (lo + 1.0f) : hi;
    box6[a] = lo;
    box6[3 + a] = hi;
  }
}

// The records of triangle t as append_triangles (pt_scene.cpp) stores them: {p0, e1 = p1 - p0, e2 = p2 - p0} and the three
// vertex normals, padding zeroed; the packed record is g's nine floats without the padding.
__device__ __forceinline__ void mesh_triangle_record(const float* __restrict__ pos, const float* __restrict__ nrm, const uint32_t* __restrict__ idx,
                                                     uint32_t t, Tri* g, TriNrm* nn) {
  const size_t v0 = idx[3 * (size_t)t], v1 = idx[3 * (size_t)t + 1], v2 = idx[3 * (size_t)t + 2];
  for (int a = 0; a < 3; a++) {
    const float p = pos[3 * v0 + a];
    g->p0[a] = p;
    g->e1[a] = pos[3 * v1 + a] - p;   // p0p1, student/tri_mesh.cpp:60
    g->e2[a] = pos[3 * v2 + a] - p;   // p0p2
    nn->n0[a] = nrm[3 * v0 + a];
    nn->n1[a] = nrm[3 * v1 + a];
    nn->n2[a] = nrm[3 * v2 + a];
  }
  g->p0[3] = g->e1[3] = g->e2[3] = 0.0f;
  nn->n0[3] = nn->n1[3] = nn->n2[3] = 0.0f;
}

// BBox::enclose(BBox) (lib/bbox.h) as Box::enclose of pt_scene.cpp states it: std::min(mn, b) / std::max(mx, b) per axis, the
// kept bound first - so the device refit and refit_boxes agree on the sign of a zero bound as well.
__device__ __forceinline__ void box_enclose(float box6[6], const float other6[6]) {
  for (int a = 0; a < 3; a++) {
    if (other6[a] < box6[a]) box6[a] = other6[a];
    if (box6[3 + a] < other6[3 + a]) box6[3 + a] = other6[3 + a];
  }
}
__device__ __forceinline__ void box_empty(float box6[6]) {   // BBox(), lib/bbox.h:17
  for (int a = 0; a < 3; a++) { box6[a] = 3.402823466e+38f; box6[3 + a] = -3.402823466e+38f; }
}

}  // namespace srt

#endif
