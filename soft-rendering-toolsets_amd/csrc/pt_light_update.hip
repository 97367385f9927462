// srt_pt_set_dynamic_lights on the device: the three kernels that give a re-posed or deformed area light the tables a fresh
// commit would upload for it (pt_light_update.h has the arithmetic).  All are a few hundred to a few thousand lanes of copies with
// a little arithmetic: one lane per light or per light triangle, every index checked against the array it addresses, no LDS and
// no atomics.  A Light is 272 B and a LightTri 64 B, both 16-byte aligned, so the matrices and the triangle records go out as
// 16-byte stores; the packed triangle record (36 B, 4-byte aligned) goes out as dwords.  They run after the caller's verdict and
// its wait: nothing of the context is in flight while they write the live arrays.
#include <hip/hip_runtime.h>

#include "pt_light_update.h"

namespace srt {
namespace {

static_assert(sizeof(Light) == 16 + 4 * 64 && sizeof(LightTri) == 64, "light table layout");
static_assert(offsetof(Light, trans) == 16 && offsetof(Light, pdfT) == 144 && offsetof(LightTri, area_term) == 48, "light table layout");

__device__ __forceinline__ void store_mat(float4* to, const float m[16]) {
  for (int c = 0; c < 4; c++) to[c] = make_float4(m[4 * c], m[4 * c + 1], m[4 * c + 2], m[4 * c + 3]);
}

__global__ __launch_bounds__(256) void light_records_kernel(const uint32_t* __restrict__ listed, uint32_t n, const PoseOut* __restrict__ pose, uint32_t npose,
                                                            Light* __restrict__ lights, uint32_t nlights) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t k = listed[2 * (size_t)j], li = listed[2 * (size_t)j + 1];
  if (k >= npose || li >= nlights) return;                        // (the table was made on the host from the checked list)
  float t[16], it[16], pdfT[16], pdfiT[16];
  for (int e = 0; e < 16; e++) { t[e] = pose[k].trans[e]; it[e] = pose[k].itrans[e]; }
  const uint32_t has_trans = pose[k].has_trans;
  light_matrices(t, it, has_trans, pdfT, pdfiT);
  Light* L = lights + li;
  L->has_trans = has_trans;                                      // tri_base, ntri, pad stay
  float4* m = reinterpret_cast<float4*>(&L->trans);              // trans, itrans, pdfT, pdfiT: the record's last sixteen quads
  store_mat(m, t);
  store_mat(m + 4, it);
  store_mat(m + 8, pdfT);
  store_mat(m + 12, pdfiT);
}

// blockIdx.y = listed light, blockIdx.x * 256 + threadIdx.x = triangle of that light
__global__ __launch_bounds__(256) void light_area_terms_kernel(const uint32_t* __restrict__ listed, uint32_t n, const Light* __restrict__ lights, uint32_t nlights,
                                                               uint32_t light_tri_first, LightTri* __restrict__ ltris, uint32_t nltris) {
  const uint32_t j = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t li = listed[2 * (size_t)j + 1];
  if (li >= nlights) return;
  const Light* L = lights + li;
  if (t >= L->ntri || L->tri_base < light_tri_first) return;
  const size_t at = (size_t)(L->tri_base - light_tri_first) + t;
  if (at >= nltris) return;
  float T[16];
  for (int e = 0; e < 16; e++) T[e] = L->pdfT.c[e / 4][e % 4];
  const float4* in = reinterpret_cast<const float4*>(ltris + at);
  const float4 a = in[0], b = in[1], c = in[2];
  const float v0[3] = {a.x, a.y, a.z}, v1[3] = {b.x, b.y, b.z}, v2[3] = {c.x, c.y, c.z};
  ltris[at].area_term = light_area(T, v0, v1, v2);
}

__global__ __launch_bounds__(256) void light_triangles_kernel(const float* __restrict__ pos, const float* __restrict__ nrm, const uint32_t* __restrict__ idx,
                                                              uint32_t ntri, const Light* __restrict__ light, Tri* __restrict__ tris, TriNrm* __restrict__ tri_nrm,
                                                              float* __restrict__ packed, LightTri* __restrict__ ltris) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntri) return;
  Tri g;
  TriNrm nn;
  mesh_triangle_record(pos, nrm, idx, t, &g, &nn);
  float4* to = reinterpret_cast<float4*>(tris + t);
  to[0] = make_float4(g.p0[0], g.p0[1], g.p0[2], g.p0[3]);
  to[1] = make_float4(g.e1[0], g.e1[1], g.e1[2], g.e1[3]);
  to[2] = make_float4(g.e2[0], g.e2[1], g.e2[2], g.e2[3]);
  float4* no = reinterpret_cast<float4*>(tri_nrm + t);
  no[0] = make_float4(nn.n0[0], nn.n0[1], nn.n0[2], nn.n0[3]);
  no[1] = make_float4(nn.n1[0], nn.n1[1], nn.n1[2], nn.n1[3]);
  no[2] = make_float4(nn.n2[0], nn.n2[1], nn.n2[2], nn.n2[3]);
  float* po = packed + 9 * (size_t)t;
  for (int a = 0; a < 3; a++) { po[a] = g.p0[a]; po[3 + a] = g.e1[a]; po[6 + a] = g.e2[a]; }
  float T[16];
  for (int e = 0; e < 16; e++) T[e] = light->pdfT.c[e / 4][e % 4];
  LightTri lt;
  light_triangle(pos, idx, t, T, &lt);
  float4* lo = reinterpret_cast<float4*>(ltris + t);
  lo[0] = make_float4(lt.v0[0], lt.v0[1], lt.v0[2], lt.v0[3]);
  lo[1] = make_float4(lt.v1[0], lt.v1[1], lt.v1[2], lt.v1[3]);
  lo[2] = make_float4(lt.v2[0], lt.v2[1], lt.v2[2], lt.v2[3]);
  lo[3] = make_float4(lt.area_term, lt.pad[0], lt.pad[1], lt.pad[2]);
}

}  // namespace

void launch_light_records(void* stream, const uint32_t* d_listed, uint32_t n, const PoseOut* d_pose_out, uint32_t npose, Light* d_lights, uint32_t nlights) {
  if (!n) return;
  light_records_kernel<<<dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(d_listed, n, d_pose_out, npose, d_lights, nlights);
}

void launch_light_area_terms(void* stream, const uint32_t* d_listed, uint32_t n, uint32_t max_ntri, const Light* d_lights, uint32_t nlights,
                             uint32_t light_tri_first, LightTri* d_ltris, uint32_t nltris) {
  if (!n || !max_ntri) return;
  // (a grid has at most 65535 rows: more listed lights than that go in several launches)
  for (uint32_t from = 0; from < n; from += 65535u) {
    const uint32_t rows = n - from < 65535u ? n - from : 65535u;
    light_area_terms_kernel<<<dim3((max_ntri + 255u) / 256u, rows), dim3(256), 0, (hipStream_t)stream>>>(d_listed + 2 * (size_t)from, rows, d_lights, nlights,
                                                                                                        light_tri_first, d_ltris, nltris);
  }
}

void launch_light_triangles(void* stream, const float* d_pos, const float* d_nrm_in, const uint32_t* d_idx, uint32_t ntri, const Light* d_light,
                            Tri* d_tris, TriNrm* d_nrm, float* d_packed, LightTri* d_ltris) {
  if (!ntri) return;
  light_triangles_kernel<<<dim3((ntri + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(d_pos, d_nrm_in, d_idx, ntri, d_light, d_tris, d_nrm, d_packed, d_ltris);
}

}  // namespace srt
