// Per-light and per-light-triangle work of srt_pt_set_dynamic_lights as device functions: the Light record of one pose
// (Object::pdf's pair pdfT = I * trans, pdfiT = itrans * I; rays/object.h:90-94), the 2 / |cross| factor of Triangle::pdf
// (student/tri_mesh.cpp:137) under that pdfT, and the whole LightTri of one triangle of a light's mesh.  pt_light_update.hip runs
// them one lane per listed light / per light triangle; the host emulation (tests/host_emu/lights_host.cpp) compiles this header
// with g++ and compares with light_record / light_area_term / light_tri_record of pt_scene.cpp, which stay the definition: the
// same products in the same order, every sum in the same order (mat_mul accumulates from 0.0f, which decides the sign of a zero
// and where a NaN appears), the same three divides of Mat4 * Vec3, the same square root and the same IEEE divide.  The library's
// flags are part of it: -ffp-contract=off, so that no product is fused into a sum.
// A matrix is sixteen floats in Mat4::data order: m[4 * col + row].
//
// Who writes the live light arrays: the device forms (srt_pt_repose_device, srt_pt_update_mesh_device, srt_pt_refit_mesh_device,
// the skin poses) run the kernels below after their verdict and their wait and upload no Light, LightTri or light-copy triangle
// record; the host forms (srt_pt_repose, srt_pt_update_mesh, srt_pt_refit_mesh) upload the few records their host mirror holds.
#ifndef SRT_PT_LIGHT_UPDATE_H
#define SRT_PT_LIGHT_UPDATE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_mesh_update.h"
#include "pt_pose.h"
#include "pt_scene.h"

namespace srt {

// mat_mul(self, m) of pt_scene.cpp (Mat4::operator*, lib/mat4.h:110-121): r[i][j] = sum over k of m[i][k] * self[k][j], from 0.0f.
__device__ __forceinline__ void light_mat_mul(const float self[16], const float m[16], float r[16]) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.0f;
      for (int k = 0; k < 4; k++) acc += m[4 * i + k] * self[4 * k + j];
      r[4 * i + j] = acc;
    }
}

// mat_point of pt_scene.cpp (Mat4 * Vec3, lib/mat4.h:125-131): ((c0 v0 + c1 v1) + c2 v2) + c3 * 1.0f per row, then three divides.
__device__ __forceinline__ void light_mat_point(const float m[16], const float v[3], float out[3]) {
  float o[4];
  for (int j = 0; j < 4; j++) o[j] = ((m[j] * v[0] + m[4 + j] * v[1]) + m[8 + j] * v[2]) + m[12 + j] * 1.0f;
  out[0] = o[0] / o[3]; out[1] = o[1] / o[3]; out[2] = o[2] / o[3];
}

// light_record of pt_scene.cpp: the four matrices of a Light from the pose values (identities for the pdf pair when !has_trans).
__device__ __forceinline__ void light_matrices(const float trans[16], const float itrans[16], uint32_t has_trans, float pdfT[16], float pdfiT[16]) {
  float id[16];
  for (int e = 0; e < 16; e++) id[e] = pdfT[e] = pdfiT[e] = (e % 5 == 0) ? 1.0f : 0.0f;
  if (has_trans) {
    light_mat_mul(id, trans, pdfT);      // mat_mul(I, trans)
    light_mat_mul(itrans, id, pdfiT);    // mat_mul(itrans, I)
  }
}

// light_area_term of pt_scene.cpp: 2 / |cross(T v1 - T v0, T v2 - T v0)|; a zero-area triangle gives inf.
__device__ __forceinline__ float light_area(const float T[16], const float v0[3], const float v1[3], const float v2[3]) {
  float w0[3], w1[3], w2[3];
  light_mat_point(T, v0, w0);
  light_mat_point(T, v1, w1);
  light_mat_point(T, v2, w2);
  const float ax = w1[0] - w0[0], ay = w1[1] - w0[1], az = w1[2] - w0[2];
  const float bx = w2[0] - w0[0], by = w2[1] - w0[1], bz = w2[2] - w0[2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  return 2.0f / sqrtf(cx * cx + cy * cy + cz * cz);
}

// light_tri_record of pt_scene.cpp: triangle t of the mesh (pos, idx) as a LightTri under pdfT, padding zeroed.
__device__ __forceinline__ void light_triangle(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t t, const float pdfT[16], LightTri* lt) {
  const size_t i0 = idx[3 * (size_t)t], i1 = idx[3 * (size_t)t + 1], i2 = idx[3 * (size_t)t + 2];
  for (int a = 0; a < 3; a++) { lt->v0[a] = pos[3 * i0 + a]; lt->v1[a] = pos[3 * i1 + a]; lt->v2[a] = pos[3 * i2 + a]; }
  lt->v0[3] = lt->v1[3] = lt->v2[3] = 0.0f;
  lt->area_term = light_area(pdfT, lt->v0, lt->v1, lt->v2);
  lt->pad[0] = lt->pad[1] = lt->pad[2] = 0.0f;
}

// ---- launchers (pt_light_update.hip); every one only enqueues on `stream` ----
// One lane per listed light j < n: d_listed[2 j ..] = {k, light}; reads d_pose_out[k] (where launch_pose_objects left it) and writes the
// matrices and has_trans of d_lights[light] in place.  npose / nlights bound the two indices.
void launch_light_records(void* stream, const uint32_t* d_listed, uint32_t n, const PoseOut* d_pose_out, uint32_t npose, Light* d_lights, uint32_t nlights);
// One lane per light triangle of the listed lights (a row of blocks per light): reads d_ltris[..].v0..v2 and the light's pdfT,
// writes area_term.  max_ntri: the largest triangle count among the listed lights; nltris bounds the LightTri index.
void launch_light_area_terms(void* stream, const uint32_t* d_listed, uint32_t n, uint32_t max_ntri, const Light* d_lights, uint32_t nlights,
                             uint32_t light_tri_first, LightTri* d_ltris, uint32_t nltris);
// One lane per triangle t < ntri of an updated or refitted light mesh: the Tri / TriNrm / packed records of the light-list copy
// (mesh_triangle_record, index order) at d_tris / d_nrm / d_packed + t and the whole LightTri at d_ltris + t under *d_light's pdfT.
// The four output pointers are the light's ranges already.
void launch_light_triangles(void* stream, const float* d_pos, const float* d_nrm_in, const uint32_t* d_idx, uint32_t ntri, const Light* d_light,
                            Tri* d_tris, TriNrm* d_nrm, float* d_packed, LightTri* d_ltris);

}  // namespace srt

#endif
