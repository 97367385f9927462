// What the units that change a committed scene share - pt_update.cpp, pt_update_mesh.cpp, pt_update_skin.cpp, pt_update_pose.cpp,
// pt_update_shading.cpp and pt_update_emitter.cpp - and nobody else: each name here is used by more than one of them; what the rest of csrc/ calls is in
// pt_context.h.  Host code only.
#ifndef SRT_PT_UPDATE_H
#define SRT_PT_UPDATE_H

#include <vector>

#include "pt_context.h"

namespace srt {

// Every device write that follows a replaced host mirror (apply_* of pt_scene.h) returns through here: after a failed one the
// device arrays are behind the host's, so the scene is no longer committed and has to be committed again.
inline int written(srt_pt* pt, int status) {
  if (status != SRT_OK) pt->committed = false;
  return status;
}

// (pt_update.cpp)
hipError_t quiesce(srt_pt* pt);
int ensure_mesh_idx(srt_pt* pt, uint32_t object);
int write_top_level(srt_pt* pt, hipStream_t s, size_t old_tlas_nodes);
int upload_object_tables(srt_pt* pt, bool records = true);
int upload_light(srt_pt* pt, uint32_t li, bool triangles);
// The listed area lights (srt_pt_set_dynamic_lights): {position in the list, light} pairs as the light kernels take them, and the largest triangle count.
struct ListedLights { std::vector<uint32_t> pairs; uint32_t max_ntri = 0; };
ListedLights listed_lights(const BuiltScene& built, const uint32_t* objects, uint32_t n);
int upload_listed_lights(srt_pt* pt, const uint32_t* objects, uint32_t n);
void launch_listed_lights(srt_pt* pt, hipStream_t s, uint32_t nl, uint32_t max_ntri, uint32_t n);

// (pt_update_mesh.cpp)
// The new vertex arrays of a mesh on both sides.  h_*: the host form's arrays; d_*: the device form's (h_* NULL), read back into back_*.
struct MeshVertices { const float *h_pos, *h_nrm, *d_pos, *d_nrm; std::vector<float> back_pos, back_nrm; };
int update_mesh(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, MeshVertices V, uint32_t nverts);
int refit_mesh(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, MeshVertices V, uint32_t nverts);
int refit_mesh_inplace(srt_pt* pt, const char* what, uint32_t object, const float* pos, const float* nrm, uint32_t nverts);
int refit_mesh_inplace_device(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, const float* d_pos, const float* d_nrm, uint32_t nverts);
int make_refit_tables(const HostBVH& tree, const char* what, uint32_t object, RefitTables* T);

// The parts of settle() (pt_update_mesh.cpp, pt_update_pose.cpp, pt_update_shading.cpp): settle_top begins with settle_mesh
int settle_mesh(srt_pt* pt);
int settle_top(srt_pt* pt);
int settle_shading(srt_pt* pt);

// (pt_update_pose.cpp) What the enqueue-only refits of the BVH<Object> share - srt_pt_repose_refit_device, srt_pt_set_active_device and
// srt_pt_refit_mesh_inplace_device.  ensure_top_tables: the pose tables and the tree's refit tables, made (blocking, counted once) at
// the first such call after a commit or after a call that replaced the tree.  enqueue_top_boxes: the leaf stage masked by the active
// table, the levels, the write into the live top-level nodes and sweep records.  record_top_pending: the launch check, the event
// behind the call, one more call for settle_top.  top_broken / top_hip_broken: a HIP failure after the first enqueue - the scene is no
// longer committed and nothing is pending.  write_top_refit: the host forms' upload of the top-level nodes, the sweep records and
// the n listed object records.
int ensure_top_tables(srt_pt* pt, hipStream_t s, const char* what);
void enqueue_top_boxes(srt_pt* pt, hipStream_t s);
int record_top_pending(srt_pt* pt, hipStream_t s, const char* what);
int top_broken(srt_pt* pt, int status);
int top_hip_broken(srt_pt* pt, const char* what, hipError_t e, const char* step);
int write_top_refit(srt_pt* pt, const uint32_t* objects, uint32_t n);

// The head of srt_pt_skin, srt_pt_timeline, srt_pt_shading_timeline and srt_pt_emitter: a handle belongs to the scene its context held when it was
// made.  (Each handle's *_usable refuses NULL and a stale handle in words of its own.)
struct SceneHandle {
  srt_pt* pt = nullptr;
  uint64_t generation = 0;                  // pt->scene_generation at creation
  bool stale() const { return !pt->committed || generation != pt->scene_generation; }
};

// The tail of a handle's creation: what `up` puts on the device (a device context only), or the handle deleted and up's refusal.
template <class H, class Up>
int handle_publish(H* h, H** out, Up up) {
  const int st = h->pt->device >= 0 ? up() : SRT_OK;
  if (st != SRT_OK) { delete h; return st; }
  *out = h;
  return SRT_OK;
}

template <class H>
int handle_destroy(H* h) {
  if (!h) return SRT_OK;
  if (h->pt->device >= 0) (void)quiesce(h->pt);
  delete h;
  return SRT_OK;
}

}  // namespace srt

#endif
