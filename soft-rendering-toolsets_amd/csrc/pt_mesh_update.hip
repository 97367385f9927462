// srt_pt_update_mesh on the device: the two per-triangle kernels between the new vertex arrays and the arrays the render
// kernels read.  mesh_boxes_kernel feeds the device BVH builder where its boxes are; mesh_records_kernel writes the mesh's
// triangle range in the order the build (on either side) produced.  Both are bandwidth-trivial: one lane per triangle, no LDS,
// index and vertex reads through the cache (three vertices of 12 B per lane, neighbours mostly share lines), and the stores of
// a wave cover one contiguous run - 16-byte stores for the 48-byte Tri / TriNrm records, 8-byte stores for the 24-byte boxes
// and dword stores for the 36-byte packed records, whose slots are only 8- and 4-byte aligned.
#include <hip/hip_runtime.h>

#include "pt_bvh_device.h"
#include "pt_mesh_update.h"

namespace srt {
namespace {

__global__ __launch_bounds__(256) void mesh_boxes_kernel(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t ntri,
                                                         float* __restrict__ boxes6) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntri) return;
  float b[6];
  mesh_triangle_box(pos, idx, t, b);
  float2* out = reinterpret_cast<float2*>(boxes6 + 6 * (size_t)t);
  out[0] = make_float2(b[0], b[1]);
  out[1] = make_float2(b[2], b[3]);
  out[2] = make_float2(b[4], b[5]);
}

__global__ __launch_bounds__(256) void mesh_records_kernel(const float* __restrict__ pos, const float* __restrict__ nrm, const uint32_t* __restrict__ idx,
                                                           const uint32_t* __restrict__ prim, uint32_t ntri, Tri* __restrict__ tris,
                                                           TriNrm* __restrict__ tri_nrm, float* __restrict__ packed) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ntri) return;
  const uint32_t t = prim ? prim[k] : k;
  if (t >= ntri) return;   // (a permutation of [0, ntri) by construction; never an address outside the mesh's vertex arrays)
  Tri g;
  TriNrm nn;
  mesh_triangle_record(pos, nrm, idx, t, &g, &nn);
  float4* to = reinterpret_cast<float4*>(tris + k);
  to[0] = make_float4(g.p0[0], g.p0[1], g.p0[2], g.p0[3]);
  to[1] = make_float4(g.e1[0], g.e1[1], g.e1[2], g.e1[3]);
  to[2] = make_float4(g.e2[0], g.e2[1], g.e2[2], g.e2[3]);
  float4* no = reinterpret_cast<float4*>(tri_nrm + k);
  no[0] = make_float4(nn.n0[0], nn.n0[1], nn.n0[2], nn.n0[3]);
  no[1] = make_float4(nn.n1[0], nn.n1[1], nn.n1[2], nn.n1[3]);
  no[2] = make_float4(nn.n2[0], nn.n2[1], nn.n2[2], nn.n2[3]);
  float* po = packed + 9 * (size_t)k;
  for (int a = 0; a < 3; a++) { po[a] = g.p0[a]; po[3 + a] = g.e1[a]; po[6 + a] = g.e2[a]; }
}

}  // namespace

void launch_mesh_boxes(void* stream, const float* d_pos, const uint32_t* d_idx, uint32_t ntri, float* d_boxes6) {
  if (!ntri) return;
  mesh_boxes_kernel<<<dim3((ntri + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(d_pos, d_idx, ntri, d_boxes6);
}

void launch_mesh_records(void* stream, const float* d_pos, const float* d_nrm_in, const uint32_t* d_idx, const uint32_t* d_prim, uint32_t ntri,
                         Tri* d_tris, TriNrm* d_nrm, float* d_packed) {
  if (!ntri) return;
  mesh_records_kernel<<<dim3((ntri + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(d_pos, d_nrm_in, d_idx, d_prim, ntri, d_tris, d_nrm, d_packed);
}

}  // namespace srt
