// srt_pt_repose_device on the device: the pose kernel (one lane per listed object: 64 B of transform in, the Object ctor's and
// Object::bbox's values out) and the two record kernels between the table of records by insertion index and the live records in
// object order.  None of them is more than a copy with a little arithmetic: no LDS, no atomics, one launch each.
// A record is 176 B = eleven 16-byte quads.  A lane that wrote a whole record would have its wave store 64 runs 176 B apart; the
// record kernels give a record to eleven consecutive lanes instead, one quad each, so that a wave's stores (and, on the side that
// is in slot order, its loads) are one contiguous kilobyte.  The pose kernel's lanes each write 39 + 33 + 6 dwords of their own
// object: its launches are a few thousand lanes of a few hundred bytes, and its matrices are where the arithmetic is.
#include <hip/hip_runtime.h>

#include "pt_bvh_device.h"
#include "pt_pose.h"

namespace srt {
namespace {

constexpr uint32_t kQuads = sizeof(Object) / 16;                 // 11
static_assert(sizeof(Object) == 16 * kQuads, "a record is whole quads");
// word 3 = use_bvh (quad 0), word 4 = node_base (quad 1), word 9 = id (quad 2): pt_scene.h
static_assert(offsetof(Object, use_bvh) == 12 && offsetof(Object, node_base) == 16 && offsetof(Object, id) == 36 && offsetof(Object, trans) == 48,
              "record layout");

__device__ __forceinline__ bool has_blas_nodes(const uint32_t* rec) { return rec[0] == OBJ_MESH && (rec[3] & 1u) != 0u; }

// lane = 11 slot + quad: the live record of a slot, scattered to its insertion index
__global__ __launch_bounds__(256) void pose_tables_kernel(const Object* __restrict__ live, uint32_t nobj, uint32_t tlas_nodes, Object* __restrict__ by_index) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nobj * kQuads) return;
  const uint32_t slot = (uint32_t)(t / kQuads), q = (uint32_t)(t % kQuads);
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(live + slot);
  const uint32_t i = rec[9] - 1u;
  if (i >= nobj) return;                                         // (ids are a permutation of 1 .. nobj by construction; never a store outside the table)
  uint4 v = reinterpret_cast<const uint4*>(live + slot)[q];
  if (q == 0u) v.w &= 0xffu;
  if (q == 1u && has_blas_nodes(rec)) v.x -= tlas_nodes;
  reinterpret_cast<uint4*>(by_index + i)[q] = v;
}

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

// one lane per object: Object::bbox of the committed pose
__global__ __launch_bounds__(256) void posed_boxes_kernel(const Object* __restrict__ by_index, uint32_t nobj, const float* __restrict__ local6,
                                                          float* __restrict__ posed6) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nobj) return;
  float b[6], t[16];
  load_box(local6, i, b);
  if (by_index[i].has_trans) {
    for (int e = 0; e < 16; e++) t[e] = by_index[i].trans.c[e / 4][e % 4];
    pose_box(t, b);
  }
  store_box(posed6, i, b);
}

__global__ __launch_bounds__(256) void pose_objects_kernel(const uint32_t* __restrict__ listed, const float* __restrict__ trans, uint32_t n, uint32_t nobj,
                                                           const float* __restrict__ local6, PoseOut* __restrict__ out, Object* __restrict__ by_index,
                                                           float* __restrict__ posed6) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = listed[k];
  if (i >= nobj) return;                                         // (the list was checked on the host before anything was enqueued)
  float t[16], b[6];
  for (int e = 0; e < 16; e++) t[e] = trans[16 * (size_t)k + e];
  load_box(local6, i, b);
  PoseOut o;
  pose_object(t, b, &o);
  out[k] = o;
  Object* rec = by_index + i;
  rec->has_trans = o.has_trans;
  float4* m = reinterpret_cast<float4*>(&rec->trans);           // trans, itrans: the record's last eight quads
  for (int c = 0; c < 4; c++) {
    m[c] = make_float4(o.trans[4 * c], o.trans[4 * c + 1], o.trans[4 * c + 2], o.trans[4 * c + 3]);
    m[4 + c] = make_float4(o.itrans[4 * c], o.itrans[4 * c + 1], o.itrans[4 * c + 2], o.itrans[4 * c + 3]);
  }
  store_box(posed6, i, o.box);
}

// lane = 11 slot + quad: the record of the slot's object, gathered into the live array
__global__ __launch_bounds__(256) void pose_records_kernel(const Object* __restrict__ by_index, const uint32_t* __restrict__ prim,
                                                           const uint32_t* __restrict__ ordinal, uint32_t nobj, uint32_t tlas_nodes, Object* __restrict__ live) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)nobj * kQuads) return;
  const uint32_t slot = (uint32_t)(t / kQuads), q = (uint32_t)(t % kQuads);
  const uint32_t i = prim ? prim[slot] : slot;
  if (i >= nobj) return;                                         // (a permutation of [0, nobj) by construction; never a load outside the table)
  const uint32_t* rec = reinterpret_cast<const uint32_t*>(by_index + i);
  uint4 v = reinterpret_cast<const uint4*>(by_index + i)[q];
  if (q == 0u && ordinal) v.w |= ordinal[slot];
  if (q == 1u && has_blas_nodes(rec)) v.x += tlas_nodes;
  reinterpret_cast<uint4*>(live + slot)[q] = v;
}

// srt_pt_repose_refit_device.  One lane per slot: the slot of every object (insertion index), from the tree's primitive order.
__global__ __launch_bounds__(256) void top_slots_kernel(const uint32_t* __restrict__ prim, uint32_t nobj, uint32_t* __restrict__ slot_of) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= nobj) return;
  const uint32_t i = prim[slot];
  if (i < nobj) slot_of[i] = slot;                               // (a permutation of [0, nobj) by construction; never a store outside the table)
}

// lane = 9 k + q: listed object k's matrices (the last eight quads of its record by insertion index, where the pose kernel left
// them) into its live record, q == 8: its has_trans word.  Nothing else of the live record is touched.
__global__ __launch_bounds__(256) void top_objects_kernel(const uint32_t* __restrict__ listed, uint32_t n, uint32_t nobj, const uint32_t* __restrict__ slot_of,
                                                          const Object* __restrict__ by_index, Object* __restrict__ live) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * 9u) return;
  const uint32_t k = (uint32_t)(t / 9u), q = (uint32_t)(t % 9u);
  const uint32_t i = listed[k];
  if (i >= nobj) return;                                         // (the list was checked on the host before anything was enqueued)
  const uint32_t slot = slot_of ? slot_of[i] : i;
  if (slot >= nobj) return;
  if (q < 8u) reinterpret_cast<uint4*>(live + slot)[3u + q] = reinterpret_cast<const uint4*>(by_index + i)[3u + q];
  else live[slot].has_trans = by_index[i].has_trans;
}

// srt_pt_set_active_device.  One lane per listed object: its flag (any non-zero byte: active) into the table by insertion index, as 0 / 1.
// An element scatter of single bytes - a few thousand lanes at the most, the table a few cache lines: loads of consecutive list words
// and flag bytes, one byte store per lane, no two lanes on one byte (the list holds no duplicate: checked on the host).
__global__ __launch_bounds__(256) void active_scatter_kernel(const uint32_t* __restrict__ listed, const uint8_t* __restrict__ flags, uint32_t n, uint32_t nobj,
                                                             uint8_t* __restrict__ table) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = listed[k];
  if (i >= nobj) return;                                         // (the list was checked on the host before anything was enqueued)
  table[i] = flags[k] ? (uint8_t)1 : (uint8_t)0;
}

// What the leaves of the BVH<Object> hold for the walks, after the table changed (write_top_counts, pt_scene.h).  One lane per leaf
// {node, (first slot << 3) | count}: the count word of its live node - its count, or 0 while every object in it is inactive.
__global__ __launch_bounds__(256) void top_leaf_counts_kernel(const uint2* __restrict__ leaves, uint32_t nleaves, const uint32_t* __restrict__ prim,
                                                              const uint8_t* __restrict__ table, uint32_t nobj, uint32_t nnodes, Node* __restrict__ nodes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nleaves) return;
  const uint2 leaf = leaves[i];
  if (leaf.x >= nnodes) return;                                  // (the tables were checked where they were made: make_refit_tables)
  const uint32_t first = leaf.y >> 3, count = leaf.y & 7u;
  uint32_t any = 0u;
  for (uint32_t k = first; k < first + count; k++) {
    const uint32_t o = prim[k];
    if (o < nobj && table[o]) any = 1u;
  }
  nodes[leaf.x].count = LEAF_BIT | (any ? count : 0u);
}

// One lane per sweep record, in a launch behind the one above: children = {left node, right node}; a child that is a leaf gives the
// record its count.  An interior child's entry is not touched.
__global__ __launch_bounds__(256) void top_record_counts_kernel(const uint2* __restrict__ children, uint32_t nrec, uint32_t nnodes, const Node* __restrict__ nodes,
                                                                WaveInterior* __restrict__ recs) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nrec) return;
  const uint2 c = children[q];
  if (c.x >= nnodes || c.y >= nnodes) return;
  const uint32_t l = nodes[c.x].count, r = nodes[c.y].count;
  if (l & LEAF_BIT) recs[q].l_cnt = l & ~LEAF_BIT;
  if (r & LEAF_BIT) recs[q].r_cnt = r & ~LEAF_BIT;
}

// srt_pt_refit_mesh_inplace_device, the link between the two trees.  One lane per member of a refitted mesh's family (the mesh and its
// instances, by insertion index): the mesh's new root box - node 0 of its refitted node boxes - becomes the member's object-space box,
// and Object::bbox of it under the member's unchanged transform (its record by insertion index) the member's posed box: pose_box
// when has_trans, the box itself otherwise, as posed_boxes_kernel and pose_object have it.  A family is a handful of lanes; each
// reads the same 24 B box and its own record's 64 B matrix, and writes 48 B.  No two lanes write one object (the family holds no duplicate).
__global__ __launch_bounds__(256) void mesh_link_kernel(const uint32_t* __restrict__ family, uint32_t n, uint32_t nobj, const float* __restrict__ node_boxes6,
                                                        const Object* __restrict__ by_index, float* __restrict__ local6, float* __restrict__ posed6) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = family[k];
  if (i >= nobj) return;                                         // (the family was made on the host from the committed scene)
  float b[6], t[16];
  load_box(node_boxes6, 0u, b);
  store_box(local6, i, b);
  if (by_index[i].has_trans) {
    for (int e = 0; e < 16; e++) t[e] = by_index[i].trans.c[e / 4][e % 4];
    pose_box(t, b);
  }
  store_box(posed6, i, b);
}

__global__ __launch_bounds__(256) void particle_transforms_kernel(const float* __restrict__ pos, uint32_t n, float scale, float* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float p[3] = {pos[3 * (size_t)k], pos[3 * (size_t)k + 1], pos[3 * (size_t)k + 2]};
  float t[16];
  pose_translate_scale(p, scale, t);
  for (int e = 0; e < 16; e++) out[16 * (size_t)k + e] = t[e];  // (the caller's array is only known to be 4-byte aligned)
}

uint32_t blocks_for(size_t lanes) { return (uint32_t)((lanes + 255u) / 256u); }

}  // namespace

void launch_pose_tables(void* stream, const Object* d_objects, uint32_t nobj, uint32_t tlas_nodes, Object* d_by_index, const float* d_local_boxes6,
                        float* d_posed_boxes6) {
  if (!nobj) return;
  hipStream_t s = (hipStream_t)stream;
  pose_tables_kernel<<<dim3(blocks_for((size_t)nobj * kQuads)), dim3(256), 0, s>>>(d_objects, nobj, tlas_nodes, d_by_index);
  posed_boxes_kernel<<<dim3(blocks_for(nobj)), dim3(256), 0, s>>>(d_by_index, nobj, d_local_boxes6, d_posed_boxes6);
}

void launch_pose_objects(void* stream, const uint32_t* d_listed, const float* d_trans, uint32_t n, uint32_t nobj, const float* d_local_boxes6,
                         PoseOut* d_out, Object* d_by_index, float* d_posed_boxes6) {
  if (!n) return;
  pose_objects_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(d_listed, d_trans, n, nobj, d_local_boxes6, d_out, d_by_index, d_posed_boxes6);
}

void launch_pose_records(void* stream, const Object* d_by_index, const uint32_t* d_prim, const uint32_t* d_ordinal, uint32_t nobj, uint32_t tlas_nodes,
                         Object* d_objects) {
  if (!nobj) return;
  pose_records_kernel<<<dim3(blocks_for((size_t)nobj * kQuads)), dim3(256), 0, (hipStream_t)stream>>>(d_by_index, d_prim, d_ordinal, nobj, tlas_nodes, d_objects);
}

void launch_top_slots(void* stream, const uint32_t* d_prim, uint32_t nobj, uint32_t* d_slot_of) {
  if (!nobj) return;
  top_slots_kernel<<<dim3(blocks_for(nobj)), dim3(256), 0, (hipStream_t)stream>>>(d_prim, nobj, d_slot_of);
}

void launch_top_objects(void* stream, const uint32_t* d_listed, uint32_t n, uint32_t nobj, const uint32_t* d_slot_of, const Object* d_by_index,
                        Object* d_objects) {
  if (!n) return;
  top_objects_kernel<<<dim3(blocks_for((size_t)n * 9u)), dim3(256), 0, (hipStream_t)stream>>>(d_listed, n, nobj, d_slot_of, d_by_index, d_objects);
}

void launch_active_scatter(void* stream, const uint32_t* d_listed, const uint8_t* d_flags, uint32_t n, uint32_t nobj, uint8_t* d_table) {
  if (!n) return;
  active_scatter_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(d_listed, d_flags, n, nobj, d_table);
}

void launch_top_counts(void* stream, const RefitTables& T, const uint8_t* d_table, uint32_t nobj, Node* d_nodes, WaveInterior* d_wave) {
  hipStream_t s = (hipStream_t)stream;
  if (T.nleaves) top_leaf_counts_kernel<<<dim3(blocks_for(T.nleaves)), dim3(256), 0, s>>>(T.d_leaves, T.nleaves, T.d_prim, d_table, nobj, T.nnodes, d_nodes);
  if (T.nrec) top_record_counts_kernel<<<dim3(blocks_for(T.nrec)), dim3(256), 0, s>>>(T.d_children, T.nrec, T.nnodes, d_nodes, d_wave);
}

void launch_mesh_link(void* stream, const uint32_t* d_family, uint32_t n, uint32_t nobj, const float* d_node_boxes6, const Object* d_by_index,
                      float* d_local_boxes6, float* d_posed_boxes6) {
  if (!n) return;
  mesh_link_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(d_family, n, nobj, d_node_boxes6, d_by_index, d_local_boxes6, d_posed_boxes6);
}

void launch_particle_transforms(void* stream, const float* d_pos, uint32_t n, float scale, float* d_trans_out) {
  if (!n) return;
  particle_transforms_kernel<<<dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream>>>(d_pos, n, scale, d_trans_out);
}

}  // namespace srt
