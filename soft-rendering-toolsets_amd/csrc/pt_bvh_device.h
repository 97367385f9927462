// The device BVH builder's core (pt_bvh_device.hip) and the per-triangle kernels of srt_pt_update_mesh (pt_mesh_update.hip) as
// the path tracer's host code (srt_pt_scene_commit in pt_context.cpp, pt_update*.cpp) calls them.  `stream` is a hipStream_t.
#ifndef SRT_PT_BVH_DEVICE_H
#define SRT_PT_BVH_DEVICE_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "hip_owned.h"
#include "pt_scene.h"

namespace srt {

// What one device build needs next to its input: the boxes (n x 6 floats), the node array, the primitive order, the two rank
// lists of a partition, the level plan and its split count.  build_bvh_device makes one per build; a context that rebuilds a
// mesh per frame (srt_pt_update_mesh) keeps one, grown on demand.
struct BvhWorkspace {
  DeviceBuffer<float> d_boxes;
  DeviceBuffer<void> d_nodes;        // (typed in pt_bvh_device.hip)
  DeviceBuffer<uint32_t> d_prim, d_l, d_r, d_child, d_ns;
  size_t build_prims = 0;  // the primitives the six arrays next to d_prim have room for (0: only d_prim is there)
};
// Room for a build over n primitives (prim_only: for d_prim alone - the order of a host build on its way to the record kernel).
// Allocates only when n exceeds what is there.  false: out of device memory (what was there is freed).
bool bvh_workspace_reserve(BvhWorkspace* ws, uint32_t n, bool prim_only);

// BVH<Primitive>::build over the n boxes in d_boxes6 (ws->d_boxes, or an array of the caller's that holds them already), enqueued
// on `stream` (which it synchronises once per level and at the end).  Nodes and primitive order come back in *out and the order
// stays in ws->d_prim.  false: the build does not terminate, or a HIP call failed (out is then empty).
bool build_bvh_device_core(BvhWorkspace* ws, void* stream, const float* d_boxes6, uint32_t n, uint32_t max_leaf, HostBVH* out);

// One lane per triangle: Triangle::bbox of the ntri triangles of (d_pos, d_idx) into d_boxes6 (pt_mesh_update.h).
void launch_mesh_boxes(void* stream, const float* d_pos, const uint32_t* d_idx, uint32_t ntri, float* d_boxes6);
// One lane per triangle slot k < ntri: the records of triangle d_prim[k] (k itself when d_prim is NULL) into d_tris[k], d_nrm[k]
// and d_packed[9 k ..] - the caller passes the three arrays offset to the mesh's first slot.
void launch_mesh_records(void* stream, const float* d_pos, const float* d_nrm_in, const uint32_t* d_idx, const uint32_t* d_prim, uint32_t ntri,
                         Tri* d_tris, TriNrm* d_nrm, float* d_packed);

// What a refit of one mesh (srt_pt_refit_mesh) keeps on the device, made from the host tree at the mesh's first refit and
// dropped when the mesh is rebuilt or the scene committed again: the primitive order (4 B per triangle), the leaves as {node,
// (first slot << 3) | count}, the interior nodes as {node, left child} sorted by level with the level offsets, the interior
// records' {left node, right node} (8 B each), and the two box arrays the kernels work in.
struct RefitTables {
  uint32_t ntri = 0, nnodes = 0, nleaves = 0, nrec = 0;
  DeviceBuffer<uint32_t> d_prim;
  DeviceBuffer<uint2> d_leaves, d_list, d_children;
  DeviceBuffer<uint32_t> d_level_off;
  std::vector<uint32_t> level_off;       // levels + 1 offsets into d_list (level 0: the root)
  DeviceBuffer<float> d_tri_boxes, d_node_boxes;   // (d_tri_boxes: a mesh's only - the BVH<Object>'s leaf boxes are the pose tables')
  uint64_t uncounted_bytes = 0;          // what went up for these tables and is not in the context's upload figure yet (a refused refit adds nothing)
  int level_launches = 0;                // != 0: one launch per level even where a run of levels fits one workgroup (measurements)
};
// Leaf boxes from d_leaf_boxes6 (by original primitive: a mesh's T.d_tri_boxes, launch_mesh_boxes' output; the BVH<Object>'s posed
// boxes), then the interior levels, deepest first, into d_node_boxes6 (six floats per node).  Only enqueues.  d_mask (NULL: none): one
// byte per original primitive, 0 = the leaf stage folds BBox() in the place of that primitive's box (srt_pt_set_active's table).
void launch_refit_boxes(void* stream, const RefitTables& T, const float* d_leaf_boxes6, float* d_node_boxes6, const uint8_t* d_mask = nullptr);
// The boxes into the mesh's live nodes (d_mesh_nodes: its first Node) and interior records (d_mesh_recs: its first record).
void launch_refit_write(void* stream, const RefitTables& T, const float* d_node_boxes6, Node* d_mesh_nodes, WaveInterior* d_mesh_recs);

}  // namespace srt

#endif
