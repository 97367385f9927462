// The device BVH builder's core (pt_bvh_device.hip) and the per-triangle kernels of srt_pt_update_mesh (pt_mesh_update.hip) as
// pt.hip calls them.  Plain pointers only: `stream` is a hipStream_t.
#ifndef SRT_PT_BVH_DEVICE_H
#define SRT_PT_BVH_DEVICE_H

#include <cstddef>
#include <cstdint>

#include "pt_scene.h"

namespace srt {

// What one device build needs next to its input: the boxes (n x 6 floats), the node array, the primitive order, the two rank
// lists of a partition, the level plan and its split count.  build_bvh_device allocates and frees one per build; a context that
// rebuilds a mesh per frame (srt_pt_update_mesh) keeps one, grown on demand and freed with the context.
struct BvhWorkspace {
  float* d_boxes = nullptr;
  void* d_nodes = nullptr;
  uint32_t *d_prim = nullptr, *d_l = nullptr, *d_r = nullptr, *d_child = nullptr, *d_ns = nullptr;
  size_t prims = 0;        // capacity of d_prim
  size_t build_prims = 0;  // capacity of the six others (0: only d_prim is there)
};
// Room for a build over n primitives (prim_only: for d_prim alone - the order of a host build on its way to the record kernel).
// Allocates only when n exceeds what is there.  false: out of device memory (what was there is freed).
bool bvh_workspace_reserve(BvhWorkspace* ws, uint32_t n, bool prim_only);
void bvh_workspace_free(BvhWorkspace* ws);

// BVH<Primitive>::build over the n boxes in ws->d_boxes, enqueued on `stream` (which it synchronises once per level and at the
// end).  Nodes and primitive order come back in *out and the order stays in ws->d_prim.  false: the build does not terminate,
// or a HIP call failed (out is then empty).
bool build_bvh_device_core(BvhWorkspace* ws, void* stream, uint32_t n, uint32_t max_leaf, HostBVH* out);

// One lane per triangle: Triangle::bbox of the ntri triangles of (d_pos, d_idx) into d_boxes6 (pt_mesh_update.h).
void launch_mesh_boxes(void* stream, const float* d_pos, const uint32_t* d_idx, uint32_t ntri, float* d_boxes6);
// One lane per triangle slot k < ntri: the records of triangle d_prim[k] (k itself when d_prim is NULL) into d_tris[k], d_nrm[k]
// and d_packed[9 k ..] - the caller passes the three arrays offset to the mesh's first slot.
void launch_mesh_records(void* stream, const float* d_pos, const float* d_nrm_in, const uint32_t* d_idx, const uint32_t* d_prim, uint32_t ntri,
                         Tri* d_tris, TriNrm* d_nrm, float* d_packed);

}  // namespace srt

#endif
