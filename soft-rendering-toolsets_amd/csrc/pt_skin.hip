// Skeleton::find_joints and Skeleton::skin on the device: the launches around the per-vertex functions of pt_skin.h.  One lane
// per vertex everywhere (one per triangle for the last-triangle pass); positions and normals are the 12 B-strided arrays
// srt_pt_update_mesh_device takes, so a wave's loads and stores cover one contiguous 768 B run.  The vertex -> joints map is CSR:
// a count per vertex, an exclusive scan (256 counts per block in LDS, then one block over the block sums), the fill.  The joint
// data (inverse bind matrix, extent and radius; 80 B per joint) are read at a wave-uniform index in the find_joints passes - the
// compiler keeps them in scalar registers - and the per-frame matrices (64 B per joint) at a per-lane index, from L2: a skin holds
// at most kSkinMaxJoints of them.  All loops are bounded by the joint count or a vertex's influence count; the only atomic is a
// vector atomicMax on a global uint32_t.
#include <hip/hip_runtime.h>

#include "pt_skin.h"

namespace srt {
namespace {

constexpr uint32_t kBlock = 256;

__device__ __forceinline__ SkinV3 load3(const float* __restrict__ a, uint32_t v) { return {a[3 * (size_t)v], a[3 * (size_t)v + 1], a[3 * (size_t)v + 2]}; }
__device__ __forceinline__ void store3(float* __restrict__ a, uint32_t v, SkinV3 p) {
  a[3 * (size_t)v] = p.x; a[3 * (size_t)v + 1] = p.y; a[3 * (size_t)v + 2] = p.z;
}

__global__ __launch_bounds__(kBlock) void skin_count_kernel(const float* __restrict__ pos, uint32_t nverts, const float* __restrict__ inv,
                                                           const float* __restrict__ cap, uint32_t njoints, uint32_t* __restrict__ counts) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nverts) return;
  counts[v] = skin_count_joints(inv, cap, njoints, load3(pos, v));
}

// Inclusive scan of one value per thread of the block (Hillis-Steele in LDS); every thread of the block calls it.
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t* s, uint32_t value) {
  const uint32_t tid = threadIdx.x;
  s[tid] = value;
  __syncthreads();
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    const uint32_t t = tid >= d ? s[tid - d] : 0u;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}

// off[v] = the exclusive sum of the block's counts in front of v; sums[block] = the block's total
__global__ __launch_bounds__(kBlock) void skin_scan_blocks_kernel(const uint32_t* __restrict__ counts, uint32_t nverts, uint32_t* __restrict__ off,
                                                                 uint32_t* __restrict__ sums) {
  __shared__ uint32_t s[kBlock];
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t c = v < nverts ? counts[v] : 0u;
  const uint32_t incl = block_inclusive_scan(s, c);
  if (v < nverts) off[v] = incl - c;
  if (threadIdx.x == kBlock - 1) sums[blockIdx.x] = incl;
}

// One block: sums[] becomes its own exclusive scan, 256 entries per trip with a carry, and the grand total goes to *total.
__global__ __launch_bounds__(kBlock) void skin_scan_sums_kernel(uint32_t* __restrict__ sums, uint32_t nblocks, uint32_t* __restrict__ total) {
  __shared__ uint32_t s[kBlock];
  uint32_t carry = 0;                                     // the same value in every thread
  for (uint32_t base = 0; base < nblocks; base += kBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t c = i < nblocks ? sums[i] : 0u;
    const uint32_t incl = block_inclusive_scan(s, c);
    if (i < nblocks) sums[i] = carry + (incl - c);
    carry += s[kBlock - 1];
    __syncthreads();                                      // s is rewritten by the next trip
  }
  if (threadIdx.x == 0) *total = carry;
}

// off[v] += the sum of the blocks in front
__global__ __launch_bounds__(kBlock) void skin_scan_add_kernel(uint32_t* __restrict__ off, uint32_t nverts, const uint32_t* __restrict__ sums) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v < nverts) off[v] += sums[blockIdx.x];
}

__global__ __launch_bounds__(kBlock) void skin_fill_kernel(const float* __restrict__ pos, uint32_t nverts, const float* __restrict__ inv,
                                                          const float* __restrict__ cap, uint32_t njoints, const uint32_t* __restrict__ off,
                                                          uint32_t* jidx, float* w) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nverts) return;
  const uint32_t begin = off[v], end = off[v + 1], total = off[nverts];
  if (begin > end || end > total) return;   // (never: off is a scan; no address outside jidx / w)
  skin_fill_joints(inv, cap, njoints, load3(pos, v), begin, end, jidx, w);
}

__global__ __launch_bounds__(kBlock) void skin_last_triangle_kernel(const uint32_t* __restrict__ idx, uint32_t ntri, uint32_t nverts, uint32_t* last) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= ntri) return;
  for (int k = 0; k < 3; k++) {
    const uint32_t v = idx[3 * (size_t)t + k];
    if (v < nverts) atomicMax(&last[v], t + 1u);
  }
}

__global__ __launch_bounds__(kBlock) void skin_vertices_kernel(const float* __restrict__ pos, const float* __restrict__ nrm, uint32_t nverts,
                                                              const float* __restrict__ mats, uint32_t njoints, const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ jidx, const float* __restrict__ w,
                                                              float* __restrict__ pos_out, float* __restrict__ nrm_out) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nverts) return;
  store3(pos_out, v, skin_vertex(mats, off, jidx, w, njoints, load3(pos, v), v));
  if (nrm_out) store3(nrm_out, v, load3(nrm, v));
}

__global__ __launch_bounds__(kBlock) void skin_flat_normals_kernel(const float* __restrict__ pos_out, const float* __restrict__ nrm,
                                                                  const uint32_t* __restrict__ idx, uint32_t ntri, const uint32_t* __restrict__ last,
                                                                  uint32_t nverts, float* __restrict__ nrm_out) {
  const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
  if (v >= nverts) return;
  const uint32_t t1 = last[v];
  bool named = t1 != 0u && t1 <= ntri;
  if (named)
    for (int k = 0; k < 3; k++) named = named && idx[3 * (size_t)(t1 - 1u) + k] < nverts;   // (always: srt_pt_add_mesh checked the indices)
  store3(nrm_out, v, named ? skin_flat_normal(pos_out, idx, t1 - 1u) : load3(nrm, v));
}

dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1u) / kBlock); }

}  // namespace

void launch_skin_count(void* stream, const float* d_pos, uint32_t nverts, const float* d_inv, const float* d_cap, uint32_t njoints, uint32_t* d_counts) {
  if (!nverts) return;
  skin_count_kernel<<<grid_for(nverts), dim3(kBlock), 0, (hipStream_t)stream>>>(d_pos, nverts, d_inv, d_cap, njoints, d_counts);
}

void launch_skin_scan(void* stream, const uint32_t* d_counts, uint32_t nverts, uint32_t* d_off, uint32_t* d_sums) {
  if (!nverts) return;
  const dim3 grid = grid_for(nverts);
  skin_scan_blocks_kernel<<<grid, dim3(kBlock), 0, (hipStream_t)stream>>>(d_counts, nverts, d_off, d_sums);
  skin_scan_sums_kernel<<<dim3(1), dim3(kBlock), 0, (hipStream_t)stream>>>(d_sums, grid.x, d_off + nverts);
  skin_scan_add_kernel<<<grid, dim3(kBlock), 0, (hipStream_t)stream>>>(d_off, nverts, d_sums);
}

void launch_skin_fill(void* stream, const float* d_pos, uint32_t nverts, const float* d_inv, const float* d_cap, uint32_t njoints, const uint32_t* d_off,
                      uint32_t* d_jidx, float* d_w) {
  if (!nverts) return;
  skin_fill_kernel<<<grid_for(nverts), dim3(kBlock), 0, (hipStream_t)stream>>>(d_pos, nverts, d_inv, d_cap, njoints, d_off, d_jidx, d_w);
}

void launch_skin_last_triangle(void* stream, const uint32_t* d_idx, uint32_t ntri, uint32_t nverts, uint32_t* d_last) {
  if (!ntri) return;
  skin_last_triangle_kernel<<<grid_for(ntri), dim3(kBlock), 0, (hipStream_t)stream>>>(d_idx, ntri, nverts, d_last);
}

void launch_skin_vertices(void* stream, const float* d_pos, const float* d_nrm, uint32_t nverts, const float* d_mats, uint32_t njoints, const uint32_t* d_off,
                          const uint32_t* d_jidx, const float* d_w, float* d_pos_out, float* d_nrm_out) {
  if (!nverts) return;
  skin_vertices_kernel<<<grid_for(nverts), dim3(kBlock), 0, (hipStream_t)stream>>>(d_pos, d_nrm, nverts, d_mats, njoints, d_off, d_jidx, d_w, d_pos_out,
                                                                                 d_nrm_out);
}

void launch_skin_flat_normals(void* stream, const float* d_pos_out, const float* d_nrm, const uint32_t* d_idx, uint32_t ntri, const uint32_t* d_last,
                              uint32_t nverts, float* d_nrm_out) {
  if (!nverts) return;
  skin_flat_normals_kernel<<<grid_for(nverts), dim3(kBlock), 0, (hipStream_t)stream>>>(d_pos_out, d_nrm, d_idx, ntri, d_last, nverts, d_nrm_out);
}

}  // namespace srt
