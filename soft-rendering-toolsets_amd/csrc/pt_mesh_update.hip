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

// ---- srt_pt_refit_mesh: new boxes for a kept BVH<Triangle> ----
// All of them read and write 24-byte boxes as three 8-byte halves (a box is only 8-byte aligned), one lane per item; a wave's
// leaf / level-list / record entries are consecutive 8-byte pairs.  The boxes go into an array of their own (six floats per
// node, by node index): nothing a render kernel reads is written before refit_write_kernel.
__device__ __forceinline__ void load_box(const float* boxes6, uint32_t i, float b[6]) {
  const float2* in = reinterpret_cast<const float2*>(boxes6 + 6 * (size_t)i);
  const float2 x = in[0], y = in[1], z = in[2];
  b[0] = x.x; b[1] = x.y; b[2] = y.x; b[3] = y.y; b[4] = z.x; b[5] = z.y;
}
__device__ __forceinline__ void store_box(float* boxes6, uint32_t i, const float b[6]) {
  float2* out = reinterpret_cast<float2*>(boxes6 + 6 * (size_t)i);
  out[0] = make_float2(b[0], b[1]);
  out[1] = make_float2(b[2], b[3]);
  out[2] = make_float2(b[4], b[5]);
}

// One lane per leaf: leaf = {node, (first slot << 3) | count}; the fold of its triangles' boxes in primitive order.  Every index
// in the tables was checked against the mesh's counts where they were made (make_refit_tables, pt_update_mesh.cpp), where a bad one is an error.
// mask (the BVH<Object> under srt_pt_set_active; NULL: every primitive counts): one byte per primitive, 0 = BBox() is folded in the
// place of its box (an enclose of the empty box leaves the fold unchanged).
__global__ __launch_bounds__(256) void refit_leaves_kernel(const uint2* __restrict__ leaves, uint32_t nleaves, const uint32_t* __restrict__ prim,
                                                           const float* __restrict__ tri_boxes6, const uint8_t* __restrict__ mask,
                                                           float* __restrict__ node_boxes6) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nleaves) return;
  const uint2 leaf = leaves[i];
  const uint32_t first = leaf.y >> 3, count = leaf.y & 7u;
  float b[6];
  box_empty(b);
  for (uint32_t k = first; k < first + count; k++) {
    const uint32_t t = prim[k];
    float tb[6];
    if (mask && !mask[t]) box_empty(tb);
    else load_box(tri_boxes6, t, tb);
    box_enclose(b, tb);
  }
  store_box(node_boxes6, leaf.x, b);
}

// An interior node {node, left child} (right = left + 1, as everywhere in the flattened tree): left, then right.
__device__ __forceinline__ void refit_interior(uint2 e, float* node_boxes6) {
  float b[6], c[6];
  box_empty(b);
  load_box(node_boxes6, e.y, c);
  box_enclose(b, c);
  load_box(node_boxes6, e.y + 1u, c);
  box_enclose(b, c);
  store_box(node_boxes6, e.x, b);
}

// One level of more than 256 interior nodes: one lane per node of the level's run in the level-sorted list.
__global__ __launch_bounds__(256) void refit_level_kernel(const uint2* __restrict__ level, uint32_t count, float* node_boxes6) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) refit_interior(level[i], node_boxes6);
}

// Levels [lo, hi] of at most 256 interior nodes each, deepest first, in ONE workgroup: a barrier between levels orders a
// level's stores before the reads of the level above (same workgroup, so __syncthreads' fence covers global memory).
__global__ __launch_bounds__(256) void refit_levels_block_kernel(const uint2* __restrict__ list, const uint32_t* __restrict__ level_off, uint32_t lo,
                                                                 uint32_t hi, float* node_boxes6) {
  for (uint32_t l = hi + 1u; l-- > lo;) {
    const uint32_t from = level_off[l], count = level_off[l + 1u] - from;
    if (threadIdx.x < count) refit_interior(list[from + threadIdx.x], node_boxes6);
    __syncthreads();
  }
}

// After the verdict: lane i < nnodes writes node i's box into the mesh's live Node; lane nnodes + q writes the two child boxes
// of the mesh's q-th interior record (children = {left node, right node}).  Links, references and counts are not touched.
__global__ __launch_bounds__(256) void refit_write_kernel(const float* __restrict__ node_boxes6, uint32_t nnodes, Node* __restrict__ nodes,
                                                          const uint2* __restrict__ children, uint32_t nrec, WaveInterior* __restrict__ recs) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  float b[6];
  if (i < nnodes) {
    load_box(node_boxes6, i, b);
    Node* n = nodes + i;
    n->mn[0] = b[0]; n->mn[1] = b[1]; n->mn[2] = b[2];
    n->mx[0] = b[3]; n->mx[1] = b[4]; n->mx[2] = b[5];
  } else if (i - nnodes < nrec) {
    const uint32_t q = i - nnodes;
    const uint2 c = children[q];
    float4* out = reinterpret_cast<float4*>(recs + q);     // boxl[6] boxr[6]: the record's first 48 bytes
    float r[6];
    load_box(node_boxes6, c.x, b);
    load_box(node_boxes6, c.y, r);
    out[0] = make_float4(b[0], b[1], b[2], b[3]);
    out[1] = make_float4(b[4], b[5], r[0], r[1]);
    out[2] = make_float4(r[2], r[3], r[4], r[5]);
  }
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

void launch_refit_boxes(void* stream, const RefitTables& T, const float* d_leaf_boxes6, float* d_node_boxes6, const uint8_t* d_mask) {
  hipStream_t s = (hipStream_t)stream;
  if (T.nleaves)
    refit_leaves_kernel<<<dim3((T.nleaves + 255u) / 256u), dim3(256), 0, s>>>(T.d_leaves, T.nleaves, T.d_prim, d_leaf_boxes6, d_mask, d_node_boxes6);
  // deepest level first; runs of levels that fit one workgroup share a launch
  const std::vector<uint32_t>& off = T.level_off;
  uint32_t l = (uint32_t)off.size() - 1u;          // number of levels
  while (l > 0u) {
    const uint32_t hi = l - 1u, count = off[hi + 1u] - off[hi];
    if (count > 256u || T.level_launches) {
      if (count) refit_level_kernel<<<dim3((count + 255u) / 256u), dim3(256), 0, s>>>(T.d_list + off[hi], count, d_node_boxes6);
      l = hi;
    } else {
      uint32_t lo = hi;
      while (lo > 0u && off[lo] - off[lo - 1u] <= 256u) lo--;
      refit_levels_block_kernel<<<dim3(1), dim3(256), 0, s>>>(T.d_list, T.d_level_off, lo, hi, d_node_boxes6);
      l = lo;
    }
  }
}

void launch_refit_write(void* stream, const RefitTables& T, const float* d_node_boxes6, Node* d_mesh_nodes, WaveInterior* d_mesh_recs) {
  const uint32_t n = T.nnodes + T.nrec;
  if (!n) return;
  refit_write_kernel<<<dim3((n + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(d_node_boxes6, T.nnodes, d_mesh_nodes, T.d_children, T.nrec, d_mesh_recs);
}

}  // namespace srt
