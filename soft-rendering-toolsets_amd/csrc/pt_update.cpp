// The path tracer's host side after srt_pt_scene_commit: what changes or queries a committed scene - new vertices (srt_pt_update_mesh,
// srt_pt_refit_mesh), skinning (srt_pt_skin*), new poses (srt_pt_repose*) and the figures about them.  Host code only: the kernels are in
// pt_mesh_update.hip, pt_pose.hip, pt_light_update.hip, pt_skin.hip and pt_bvh_device.hip, the context and what the units share in pt_context.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_anim.h"
#include "pt_context.h"
#include "pt_light_update.h"
#include "pt_mesh_update.h"
#include "pt_skin.h"
#include "srt_pt_debug.h"

using namespace srt;

// ---- srt_pt_skin: Skeleton::find_joints once, Skeleton::skin per frame (pt_skin.h, pt_skin.hip) ----
struct srt_pt_skin {
  srt_pt* pt = nullptr;
  uint64_t generation = 0;                  // pt->scene_generation at creation
  uint32_t object = 0, nverts = 0, ntri = 0, njoints = 0, ninf = 0;
  std::vector<float> inv;                   // Mat4::inverse(joint_to_bind(j)), 16 floats per joint
  std::vector<float> mats;                  // the frame's posed_j * inverse_j on their way up
  DeviceBuffer<float> d_pos, d_nrm;                     // the bind-pose mesh
  DeviceBuffer<float> d_inv, d_cap, d_mats;
  DeviceBuffer<uint32_t> d_off, d_jidx, d_last;
  DeviceBuffer<float> d_w;
  DeviceBuffer<float> d_pos_out, d_nrm_out;             // srt_pt_skin_pose's staging
  // srt_pt_skin_set_rig: the hierarchy and the joints' keys, on both sides; d_local: Mat4::euler(pose) per joint, the frame's
  bool rigged = false;
  std::vector<int32_t> parent;
  std::vector<float> cap, rest_pose, knot_times, knot_quats;   // cap: {extent, radius} per joint, from srt_pt_skin_create
  std::vector<uint32_t> knot_offsets;
  float base[3] = {0.0f, 0.0f, 0.0f};
  DeviceBuffer<int32_t> d_parent;
  DeviceBuffer<uint32_t> d_knot_offsets;
  DeviceBuffer<float> d_base, d_rest_pose, d_knot_times, d_knot_quats, d_local;
};

// ---- srt_pt_timeline: Anim_Pose::at(t) and Pose::transform() of listed objects (pt_anim.h, pt_anim.hip) ----
struct srt_pt_timeline {
  srt_pt* pt = nullptr;
  uint64_t generation = 0;                  // pt->scene_generation at creation
  std::vector<uint32_t> objects, track_offsets;           // insertion indices; 3 tracks per object, CSR
  std::vector<float> knot_times, knot_values;
  DeviceBuffer<uint32_t> d_track_offsets;
  DeviceBuffer<float> d_knot_times, d_knot_values, d_trans;   // d_trans: the frame's transforms, 16 floats per object
};

// ---- srt_pt_shading_timeline: Anim_Material::at(t) / Scene_Light::set_time(t) of listed materials and delta lights (pt_anim.h, pt_anim.hip) ----
struct srt_pt_shading_timeline {
  srt_pt* pt = nullptr;
  uint64_t generation = 0;                  // pt->scene_generation at creation
  std::vector<uint32_t> materials, lights, track_offsets;   // 6 tracks per material, then 6 per light, then 2 of the environment (env), CSR
  bool env = false;
  std::vector<float> knot_times, knot_values;
  DeviceBuffer<uint32_t> d_track_offsets, d_materials, d_lights;
  DeviceBuffer<float> d_knot_times, d_knot_values;
};

namespace {

// The refit tables of `object` (UINT32_MAX: of every mesh): its tree is about to be replaced.
void drop_refit_tables(srt_pt* pt, uint32_t object) {
  for (auto it = pt->refit_tables.begin(); it != pt->refit_tables.end();) {
    if (object == UINT32_MAX || it->first == object) it = pt->refit_tables.erase(it);
    else ++it;
  }
}

// The BVH<Object> is about to be replaced (or d_pose_list to be overwritten by another call: then only the list is forgotten).
void forget_top_list(srt_pt* pt) { pt->top_list_valid = false; pt->top_list.clear(); }
void drop_top_tables(srt_pt* pt) {
  pt->top_tables = RefitTables();
  pt->have_top_tables = false;
  pt->d_slot_of.reset();
  forget_top_list(pt);
}

void drop_pose_tables(srt_pt* pt) {
  pt->d_pose_records.reset(); pt->d_local_boxes.reset(); pt->d_posed_boxes.reset();
  pt->pose_tables = false;
}

// No srt_pt_repose_refit_device call is waiting for settle() any more.
void forget_pending(srt_pt* pt) {
  pt->top_pending = 0;
  for (uint32_t i : pt->top_pending_objects) pt->top_pending_flag[i] = 0;
  pt->top_pending_objects.clear();
}

// Nothing is in flight any more: epochs the caller enqueued on streams of its own read the arrays that are about to change.
hipError_t quiesce(srt_pt* pt) {
  hipError_t e;
  if ((e = hipSetDevice(pt->device)) != hipSuccess || (e = hipStreamSynchronize(pt->stream)) != hipSuccess) return e;
  return hipDeviceSynchronize();
}

// The index buffer of mesh `object` on the device.  Every mesh that can be updated has its own from the commit on; an emissive
// mesh has it from the commit only when srt_pt_set_dynamic_lights was on by then - otherwise it is appended here, at the light's
// first update, refit or skin.  Nothing a render kernel reads; the caller has waited for whatever reads d_idx.
int ensure_mesh_idx(srt_pt* pt, uint32_t object) {
  if (pt->idx_off[object] != SIZE_MAX) return SRT_OK;
  const std::vector<uint32_t>& idx = pt->built.inputs[object].mesh.idx;
  DeviceBuffer<uint32_t> fresh;
  int st;
  if ((st = fresh.ensure(pt->idx_words + idx.size()))) return st;
  if ((pt->idx_words && hipMemcpy(fresh, pt->d_idx, pt->idx_words * sizeof(uint32_t), hipMemcpyDeviceToDevice) != hipSuccess) ||
      hipMemcpy(fresh + pt->idx_words, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    return srt::fail(SRT_ERR_HIP, "index buffer of object %u: device copy failed", object);
  pt->d_idx = std::move(fresh);                           // (frees the old array)
  pt->idx_off[object] = pt->idx_words;
  pt->idx_words += idx.size();
  pt->idx_uncounted += idx.size() * sizeof(uint32_t);
  return SRT_OK;
}

// Host forms of the dynamic-light calls (srt_pt_repose, srt_pt_update_mesh, srt_pt_refit_mesh): the light's record and its
// LightTri records from the host mirror, and - after new vertices - its light-list triangle copies.  The device forms run the
// kernels of pt_light_update.hip instead and upload none of this.
int upload_light(srt_pt* pt, uint32_t li, bool triangles) {
  const FlatScene& F = pt->built.flat;
  const Light& L = F.lights[li];
  const size_t lt = (size_t)(L.tri_base - F.light_tri_first), n = L.ntri;
  SRT_HIP(hipMemcpy(pt->d_lights + li, &L, sizeof(Light), hipMemcpyHostToDevice));
  if (n) SRT_HIP(hipMemcpy(pt->d_ltris + lt, &F.light_tris[lt], n * sizeof(LightTri), hipMemcpyHostToDevice));
  pt->bytes_uploaded += sizeof(Light) + n * sizeof(LightTri);
  if (triangles && n) {
    SRT_HIP(hipMemcpy(pt->d_tris + L.tri_base, &F.tris[L.tri_base], n * sizeof(Tri), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->d_nrm + L.tri_base, &F.tri_nrm[L.tri_base], n * sizeof(TriNrm), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->d_tri_packed + 9 * (size_t)L.tri_base, &F.tri_packed[9 * (size_t)L.tri_base], 9 * n * sizeof(float), hipMemcpyHostToDevice));
    const uint64_t bytes = n * (sizeof(Tri) + sizeof(TriNrm) + 9 * sizeof(float));
    pt->bytes_uploaded += bytes;
    pt->tri_bytes_uploaded += bytes;
  }
  return SRT_OK;
}

// The light tables of an emissive mesh after new vertices (the verdict is in, the host mirror is true, nothing is in flight):
// the device forms rewrite them with the kernel from the arrays where they are, the host forms upload them.
int write_light_mesh_device(srt_pt* pt, hipStream_t s, uint32_t object, bool device_form, const float* d_pos, const float* d_nrm) {
  const int32_t li = light_of(pt->built, object);
  if (li < 0) return SRT_OK;
  if (!device_form) return upload_light(pt, (uint32_t)li, true);
  const FlatScene& F = pt->built.flat;
  const Light& L = F.lights[(size_t)li];
  launch_light_triangles(s, d_pos, d_nrm, pt->d_idx + pt->idx_off[object], L.ntri, pt->d_lights + li, pt->d_tris + L.tri_base, pt->d_nrm + L.tri_base,
                         pt->d_tri_packed + 9 * (size_t)L.tri_base, pt->d_ltris + (L.tri_base - F.light_tri_first));
  SRT_HIP(hipStreamSynchronize(s));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

// The BVH<Object>'s nodes after the scene layer replaced them.  With their count unchanged the BVH<Triangle> nodes behind them have
// not moved: the first tlas_nodes nodes are copied in place, enqueued on `s`.  Otherwise all of d_nodes goes up anew, once what
// `s` holds is done with the old array.
int write_top_level(srt_pt* pt, hipStream_t s, size_t old_tlas_nodes) {
  const FlatScene& F = pt->built.flat;
  if (F.tlas_nodes != old_tlas_nodes) {
    SRT_HIP(hipStreamSynchronize(s));
    return upload(pt, &pt->d_nodes, F.nodes);
  }
  if (F.tlas_nodes) SRT_HIP(hipMemcpyAsync(pt->d_nodes, F.nodes.data(), (size_t)F.tlas_nodes * sizeof(Node), hipMemcpyHostToDevice, s));
  pt->bytes_uploaded += (uint64_t)F.tlas_nodes * sizeof(Node);
  return SRT_OK;
}

// The tables in object order after the scene layer replaced them: the sweep records, which of their children hold a real
// BVH<Triangle> and - unless a kernel has gathered them in place - the object records.  Nothing may be reading the old ones.
int upload_object_tables(srt_pt* pt, bool records = true) {
  const FlatScene& F = pt->built.flat;
  int st;
  if ((records && (st = upload(pt, &pt->d_objects, F.objects))) || (st = upload(pt, &pt->d_wave, F.wave_tlas))) return st;
  return upload(pt, &pt->d_wave_lazy, F.wave_lazy);
}

// Device side of a mesh update whose verdict is in (srt_pt_update_mesh): the node and record arrays after the scene layer
// re-packed them.  [0, keep) of the old array has not moved and [from, size) of the new one is new or has moved; with another
// total length the array is allocated anew, the part that stays is copied on the device and only the rest comes from the host.
template <typename T>
int upload_tail(srt_pt* pt, hipStream_t s, DeviceBuffer<T>* dst, size_t old_size, const std::vector<T>& src, size_t keep_from, size_t keep_to, size_t keep_n,
                size_t up_from, size_t up_to, bool tri_class) {
  // old[keep_from, keep_from + keep_n) -> new[keep_to, ..);  src[up_from, up_to) -> new[up_from, up_to)
  if (src.size() != old_size || keep_from != keep_to) {
    DeviceBuffer<T> fresh;
    int st;
    if ((st = fresh.ensure(src.empty() ? 1 : src.size()))) return st;
    if ((keep_n && hipMemcpyAsync(fresh + keep_to, *dst + keep_from, keep_n * sizeof(T), hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
      return srt::fail(SRT_ERR_HIP, "srt_pt_update_mesh: device copy failed");
    *dst = std::move(fresh);                              // (frees the old array)
  }
  if (up_to > up_from) {
    SRT_HIP(hipMemcpyAsync(*dst + up_from, src.data() + up_from, (up_to - up_from) * sizeof(T), hipMemcpyHostToDevice, s));
    pt->bytes_uploaded += (up_to - up_from) * sizeof(T);
    if (tri_class) pt->tri_bytes_uploaded += (up_to - up_from) * sizeof(T);
  }
  return SRT_OK;
}

// What srt_pt_update_mesh and srt_pt_refit_mesh refuse before they touch anything, in this order.
int check_mesh_call(srt_pt* pt, const char* what, uint32_t object, uint32_t nverts, const float* h_pos) {
  const int ready = need_committed(pt, what);
  if (ready != SRT_OK) return ready;
  const std::string refused = check_mesh_update(pt->built, object, nverts);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (pt->device < 0 && !h_pos) return srt::fail(SRT_ERR_NO_DEVICE, "%s needs a HIP device; this context is host-only", what);
  return SRT_OK;
}

// The new vertex arrays of a mesh on both sides.  h_*: the host form's arrays; d_*: the device form's (h_* NULL), read back into back_*.
struct MeshVertices { const float *h_pos, *h_nrm, *d_pos, *d_nrm; std::vector<float> back_pos, back_nrm; };

// The head of a mesh update or refit on a device: nothing is in flight, the mesh's index buffer is there (an emissive mesh's goes up
// at its first call under srt_pt_set_dynamic_lights) and the arrays are on both sides, 24 B per vertex.  The host form's go up into
// the staging - nothing of the live scene yet; blocking: the caller's arrays are not read after the call, however it returns -
// and *staged_bytes says how much, for the caller to count.  The device form's come back, so that BuiltScene::inputs and the host
// mirrors stay true: the copies are enqueued on `s`, V->h_* hold them once the caller has synchronised `s`.
int stage_vertices(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, uint32_t nverts, bool refuse_non_finite, MeshVertices* V,
                   uint64_t* staged_bytes) {
  const size_t vfloats = 3 * (size_t)nverts;
  SRT_HIP(quiesce(pt));
  int st;
  if ((st = ensure_mesh_idx(pt, object))) return st;
  if (V->h_pos) {
    if (refuse_non_finite)
      for (size_t k = 0; k < vfloats; k++)
        if (!std::isfinite(V->h_pos[k])) return srt::fail(SRT_ERR_INVALID, "%s: vertex %zu of the new positions has a non-finite coordinate", what, k / 3);
    if ((st = pt->d_vpos.ensure(vfloats)) || (st = pt->d_vnrm.ensure(vfloats))) return st;
    SRT_HIP(hipMemcpy(pt->d_vpos, V->h_pos, vfloats * sizeof(float), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->d_vnrm, V->h_nrm, vfloats * sizeof(float), hipMemcpyHostToDevice));
    *staged_bytes = 2 * vfloats * sizeof(float);
    V->d_pos = pt->d_vpos; V->d_nrm = pt->d_vnrm;
  } else {
    V->back_pos.resize(vfloats); V->back_nrm.resize(vfloats);
    SRT_HIP(hipMemcpyAsync(V->back_pos.data(), V->d_pos, vfloats * sizeof(float), hipMemcpyDeviceToHost, s));
    SRT_HIP(hipMemcpyAsync(V->back_nrm.data(), V->d_nrm, vfloats * sizeof(float), hipMemcpyDeviceToHost, s));
    V->h_pos = V->back_pos.data(); V->h_nrm = V->back_nrm.data();
  }
  return SRT_OK;
}

// srt_pt_update_mesh / srt_pt_update_mesh_device (then `s` is the caller's stream).
int update_mesh(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, MeshVertices V, uint32_t nverts) {
  int st;
  if ((st = check_mesh_call(pt, what, object, nverts, V.h_pos))) return st;
  const bool on_device = pt->device >= 0;
  const bool use_bvh = pt->built.flat.use_bvh;
  const bool device_form = V.h_pos == nullptr;
  const MeshStore old = pt->built.store[object];
  const uint32_t ntri = old.ntri;
  if (on_device) {
    uint64_t staged_bytes = 0;
    if ((st = stage_vertices(pt, what, s, object, nverts, false, &V, &staged_bytes))) return st;
    pt->bytes_uploaded += staged_bytes;                   // (whatever the verdict)
    if (device_form) SRT_HIP(hipStreamSynchronize(s));
  }
  // the one BVH<Triangle> build goes where srt_pt_scene_commit's would: a mesh at or above the device builder's threshold is
  // built there, from boxes computed there; anything else on the host
  const bool device_builder = device_builds(pt);
  const uint32_t* d_mesh_idx = on_device ? pt->d_idx + pt->idx_off[object] : nullptr;
  HostBVH device_tree;
  const bool device_wanted = device_builder && use_bvh && ntri >= pt->bvh_device_min && ntri > 4u;
  bool device_built = false;
  if (device_wanted && bvh_workspace_reserve(&pt->bvh_ws, ntri, false)) {
    launch_mesh_boxes(s, V.d_pos, d_mesh_idx, ntri, pt->bvh_ws.d_boxes);
    device_built = build_bvh_device_core(&pt->bvh_ws, s, pt->bvh_ws.d_boxes, ntri, 4, &device_tree);
  }
  // The BVH<Object> build goes where srt_pt_repose's does.  A device build of the mesh that failed - no termination, or no
  // memory - is not tried a second time through the wrapper: the host builds give the verdict.
  const DeviceBuilderScope builder(pt, device_builder && !(device_wanted && !device_built));
  MeshUpdate U;
  bool bad_argument = false;
  const std::string err = prepare_mesh_update(pt->built, object, V.h_pos, V.h_nrm, nverts, device_built ? &device_tree : nullptr, &U, &bad_argument);
  if (!err.empty()) return srt::fail(bad_argument ? SRT_ERR_INVALID : SRT_ERR_UNSUPPORTED, "%s: %s", what, err.c_str());
  if ((st = check_depth(U.top.max_tlas_depth, U.max_blas_depth))) return st;
  if (on_device && use_bvh && !device_built) {            // a host build: its primitive order goes up, 4 B per triangle
    if (!bvh_workspace_reserve(&pt->bvh_ws, ntri, true)) return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
    SRT_HIP(hipMemcpy(pt->bvh_ws.d_prim, U.blas.prim.data(), (size_t)ntri * 4, hipMemcpyHostToDevice));
    pt->bytes_uploaded += (uint64_t)ntri * 4;
  }
  // the verdict is in: from here on the new arrays replace the old ones, on the host and then on the device
  const size_t old_tlas = pt->built.flat.tlas_nodes, old_nodes = pt->built.flat.nodes.size(), old_recs = pt->built.flat.blas_recs.size();
  apply_mesh_update(&pt->built, &U);
  if (on_device) drop_update_tables(pt, object);          // they describe the tree and the boxes that were just replaced
  if (use_bvh) pt->blas_builds++;
  pt->cast_blocks = 0;                                    // the ray-cast kernel's stack depth follows the scene
  if (!on_device) return SRT_OK;
  pt->bytes_uploaded += pt->idx_uncounted;
  pt->idx_uncounted = 0;
  // the record kernel over the mesh's triangle range, the nodes and records that are new or moved, the tables of object order
  auto write = [&]() -> int {
    const FlatScene& F = pt->built.flat;
    const MeshStore now = pt->built.store[object];
    launch_mesh_records(s, V.d_pos, V.d_nrm, d_mesh_idx, use_bvh ? pt->bvh_ws.d_prim : nullptr, ntri, pt->d_tris + now.tri_base, pt->d_nrm + now.tri_base,
                        pt->d_tri_packed + 9 * (size_t)now.tri_base);
    int w;
    if (use_bvh) {
      // nodes: the BVH<Object>'s and the mesh's are new; the BVH<Triangle>s in front stay, those behind move when the mesh's count changed
      const bool same_nodes = now.nnodes == old.nnodes, same_recs = now.nrec == old.nrec;
      const size_t at = (size_t)F.tlas_nodes + now.node_off;
      if ((w = upload_tail(pt, s, &pt->d_nodes, old_nodes, F.nodes, old_tlas, F.tlas_nodes, old.node_off, at,
                           same_nodes && F.tlas_nodes == old_tlas ? at + now.nnodes : F.nodes.size(), false)) ||
          (w = write_top_level(pt, s, F.tlas_nodes)) ||     // (upload_tail has laid d_nodes out anew: the BVH<Object>'s nodes go in place, whatever their count was)
          (w = upload_tail(pt, s, &pt->d_blas, old_recs, F.blas_recs, 0, 0, old.rec_base, now.rec_base,
                           same_recs ? (size_t)now.rec_base + now.nrec : F.blas_recs.size(), true)))
        return w;
    }
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    if ((w = upload_object_tables(pt))) return w;
    return write_light_mesh_device(pt, s, object, device_form, V.d_pos, V.d_nrm);
  };
  return written(pt, write());
}

// The device tables of a tree's refits, from the host tree: made at the first refit after a commit or a rebuild.  `tree`: a mesh's
// BVH<Triangle> (object: its insertion index) or the BVH<Object> (object == UINT32_MAX; its primitives are the objects, whose
// boxes the pose tables hold already: no box array of their own is made).
int make_refit_tables(const HostBVH& tree, const char* what, uint32_t object, RefitTables* T) {
  const bool top = object == UINT32_MAX;
  const std::string whose = top ? std::string("the BVH<Object>") : "object " + std::to_string(object);
  const char* const inside = top ? "scene" : "mesh";
  const uint32_t nn = (uint32_t)tree.nodes.size(), ntri = (uint32_t)tree.prim.size();
  // a node's level: children lie behind their parent (level order, student/bvh.inl:144-145), so one forward pass does it
  std::vector<uint32_t> level(nn, 0u);
  uint32_t levels = 0;
  for (uint32_t n = 0; n < nn; n++) {
    const HostNode& h = tree.nodes[n];
    if (h.l == h.r) {
      // the leaf table packs (first slot << 3) | count, and the kernels trust it: refuse here what they could not take
      if (h.size > 7u || h.start >= (1u << 29) || (uint64_t)h.start + h.size > ntri)
        return srt::fail(SRT_ERR_UNSUPPORTED, "%s: leaf %u of %s holds %u primitives from slot %u (at most 7, below 2^29, inside the %s)", what, n,
                         whose.c_str(), h.size, h.start, inside);
      continue;
    }
    if (h.l <= n || h.r != h.l + 1u || h.r >= nn) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the tree of %s is not in level order", what, whose.c_str());
    level[h.l] = level[h.r] = level[n] + 1u;
    levels = std::max(levels, level[n] + 1u);
  }
  for (uint32_t t : tree.prim)
    if (t >= ntri) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the primitive order of %s names %s %u of %u", what, whose.c_str(), top ? "object" : "triangle", t, ntri);
  std::vector<uint2> leaves, list, children;
  std::vector<uint32_t> off(levels + 1u, 0u);
  for (uint32_t n = 0; n < nn; n++) {
    const HostNode& h = tree.nodes[n];
    if (h.l == h.r) leaves.push_back(make_uint2(n, (h.start << 3) | (h.size & 7u)));
    else { off[level[n] + 1u]++; children.push_back(make_uint2(h.l, h.r)); }     // records are numbered in node order (append_records)
  }
  for (uint32_t l = 0; l < levels; l++) off[l + 1u] += off[l];
  list.resize(children.size());
  std::vector<uint32_t> at(off.begin(), off.end() - 1);
  for (uint32_t n = 0; n < nn; n++)
    if (tree.nodes[n].l != tree.nodes[n].r) list[at[level[n]]++] = make_uint2(n, tree.nodes[n].l);
  T->ntri = ntri; T->nnodes = nn; T->nleaves = (uint32_t)leaves.size(); T->nrec = (uint32_t)children.size();
  T->level_off = off;
  const char* ll = getenv("SRT_REFIT_LEVEL_LAUNCHES");
  T->level_launches = ll && atoi(ll) != 0;
  if (T->d_prim.upload(tree.prim) || T->d_leaves.upload(leaves) || T->d_list.upload(list) || T->d_children.upload(children) || T->d_level_off.upload(off) ||
      (!top && T->d_tri_boxes.ensure((size_t)ntri * 6)) || T->d_node_boxes.ensure((size_t)(nn ? nn : 1) * 6)) {
    *T = RefitTables();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  T->uncounted_bytes += (tree.prim.size() + off.size()) * sizeof(uint32_t) + (leaves.size() + list.size() + children.size()) * sizeof(uint2);
  return SRT_OK;
}

// srt_pt_refit_mesh / srt_pt_refit_mesh_device / srt_pt_skin_pose_refit.
int refit_mesh(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, MeshVertices V, uint32_t nverts) {
  int st;
  if ((st = check_mesh_call(pt, what, object, nverts, V.h_pos))) return st;
  if (!pt->built.flat.use_bvh) return update_mesh(pt, what, s, object, V, nverts);   // a list has no tree: the update
  const bool on_device = pt->device >= 0;
  const MeshStore m = pt->built.store[object];
  const bool device_form = V.h_pos == nullptr;
  std::vector<float> node_boxes;
  RefitTables* T = nullptr;
  uint64_t staged_bytes = 0;                              // (counted with the verdict: a refused refit adds nothing to the figures)
  if (on_device) {
    if ((st = stage_vertices(pt, what, s, object, nverts, true, &V, &staged_bytes))) return st;
    auto it = pt->refit_tables.find(object);
    if (it == pt->refit_tables.end()) {
      RefitTables fresh;
      if ((st = make_refit_tables(pt->built.blas[object], "srt_pt_refit_mesh", object, &fresh)) != SRT_OK) { (void)hipStreamSynchronize(s); return st; }   // (the read-back is on s)
      it = pt->refit_tables.emplace(object, std::move(fresh)).first;
    }
    T = &it->second;
    // the new boxes, aside: triangle boxes, leaves, levels.  They come back (24 B per node) with the arrays of the device form
    // (24 B per vertex): the host checks those, takes the root box and keeps its own tree true.
    launch_mesh_boxes(s, V.d_pos, pt->d_idx + pt->idx_off[object], m.ntri, T->d_tri_boxes);
    launch_refit_boxes(s, *T, T->d_tri_boxes, T->d_node_boxes);
    node_boxes.resize(6 * (size_t)T->nnodes);
    SRT_HIP(hipMemcpyAsync(node_boxes.data(), T->d_node_boxes, node_boxes.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
  }
  const DeviceBuilderScope builder(pt, device_builds(pt));   // the BVH<Object> build goes where srt_pt_repose's does
  MeshRefit R;
  bool bad_argument = false;
  const std::string err = prepare_mesh_refit(pt->built, object, V.h_pos, V.h_nrm, nverts, on_device ? node_boxes.data() : nullptr, &R, &bad_argument);
  if (!err.empty()) return srt::fail(bad_argument ? SRT_ERR_INVALID : SRT_ERR_UNSUPPORTED, "%s: %s", what, err.c_str());
  if ((st = check_depth(R.top.max_tlas_depth, pt->built.flat.max_blas_depth))) return st;
  // the verdict is in: from here on the new boxes and records replace the old ones in place, on the host and then on the device
  const size_t old_tlas = pt->built.flat.tlas_nodes;
  apply_mesh_refit(&pt->built, &R);
  pt->refits++;
  pt->cast_blocks = 0;                                    // the ray-cast kernel's stack depth follows the scene
  if (!on_device) return SRT_OK;
  drop_pose_tables(pt);                                   // the object-space boxes changed
  drop_top_tables(pt);                                    // the BVH<Object> was rebuilt
  pt->bytes_uploaded += staged_bytes + T->uncounted_bytes + pt->idx_uncounted;   // the vertices of the host form; the tables, at the mesh's first successful refit
  T->uncounted_bytes = 0;
  pt->idx_uncounted = 0;
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_level(pt, s, old_tlas))) return w;
    launch_refit_write(s, *T, T->d_node_boxes, pt->d_nodes + pt->built.flat.tlas_nodes + m.node_off, pt->d_blas + m.rec_base);
    launch_mesh_records(s, V.d_pos, V.d_nrm, pt->d_idx + pt->idx_off[object], T->d_prim, m.ntri, pt->d_tris + m.tri_base, pt->d_nrm + m.tri_base,
                        pt->d_tri_packed + 9 * (size_t)m.tri_base);
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    if ((w = upload_object_tables(pt))) return w;
    return write_light_mesh_device(pt, s, object, device_form, V.d_pos, V.d_nrm);
  };
  return written(pt, write());
}

// What srt_pt_skin_set_rig put on the device goes (the caller has waited for what reads it).
void skin_drop_rig(srt_pt_skin* k) {
  k->d_parent.reset(); k->d_knot_offsets.reset(); k->d_base.reset(); k->d_rest_pose.reset(); k->d_knot_times.reset(); k->d_knot_quats.reset(); k->d_local.reset();
  k->rigged = false;
}

// The device side of srt_pt_skin_create.
int skin_build(srt_pt_skin* k, const float* bind_positions, const float* bind_normals, const srt_pt_skin_joint* joints) {
  srt_pt* pt = k->pt;
  const size_t vfloats = 3 * (size_t)k->nverts;
  std::vector<float>& cap = k->cap;
  cap.resize(4 * (size_t)k->njoints);
  for (uint32_t j = 0; j < k->njoints; j++) {
    skin_mat4_inverse(joints[j].bind, &k->inv[16 * (size_t)j]);
    for (int a = 0; a < 3; a++) cap[4 * (size_t)j + a] = joints[j].extent[a];
    cap[4 * (size_t)j + 3] = joints[j].radius;
  }
  SRT_HIP(hipSetDevice(pt->device));
  hipStream_t s = pt->stream;
  const uint32_t nblocks = (k->nverts + 255u) / 256u;
  int st;
  if ((st = k->d_pos.ensure(vfloats)) || (st = k->d_nrm.ensure(vfloats)) || (st = k->d_pos_out.ensure(vfloats)) || (st = k->d_nrm_out.ensure(vfloats)) ||
      (st = k->d_inv.ensure(k->inv.size())) || (st = k->d_mats.ensure(k->inv.size())) || (st = k->d_cap.ensure(cap.size())) ||
      (st = k->d_off.ensure((size_t)k->nverts + 1)) || (st = k->d_last.ensure(k->nverts)))
    return st;
  SRT_HIP(hipMemcpy(k->d_pos, bind_positions, vfloats * sizeof(float), hipMemcpyHostToDevice));
  SRT_HIP(hipMemcpy(k->d_nrm, bind_normals, vfloats * sizeof(float), hipMemcpyHostToDevice));
  SRT_HIP(hipMemcpy(k->d_inv, k->inv.data(), k->inv.size() * sizeof(float), hipMemcpyHostToDevice));
  SRT_HIP(hipMemcpy(k->d_cap, cap.data(), cap.size() * sizeof(float), hipMemcpyHostToDevice));
  pt->bytes_uploaded += (2 * vfloats + k->inv.size() + cap.size()) * sizeof(float);
  // count, scan, fill; the counts and the block sums live only here
  uint32_t total = 0;
  {
    DeviceBuffer<uint32_t> d_sums, d_counts;              // (freed in the reverse order: the counts first)
    if ((st = d_counts.ensure(k->nverts))) return st;
    if (d_sums.ensure(nblocks)) return srt::fail(SRT_ERR_HIP, "srt_pt_skin_create: out of device memory");
    launch_skin_count(s, k->d_pos, k->nverts, k->d_inv, k->d_cap, k->njoints, d_counts);
    launch_skin_scan(s, d_counts, k->nverts, k->d_off, d_sums);
    if (hipMemcpyAsync(&total, k->d_off + k->nverts, sizeof total, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
        hipGetLastError() != hipSuccess)
      return srt::fail(SRT_ERR_HIP, "srt_pt_skin_create: the find_joints kernels failed");
  }
  k->ninf = total;
  if ((st = k->d_jidx.ensure(total ? (size_t)total : 1)) || (st = k->d_w.ensure(total ? (size_t)total : 1))) return st;
  launch_skin_fill(s, k->d_pos, k->nverts, k->d_inv, k->d_cap, k->njoints, k->d_off, k->d_jidx, k->d_w);
  SRT_HIP(hipMemsetAsync(k->d_last, 0, (size_t)k->nverts * sizeof(uint32_t), s));
  launch_skin_last_triangle(s, pt->d_idx + pt->idx_off[k->object], k->ntri, k->nverts, k->d_last);
  SRT_HIP(hipStreamSynchronize(s));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int skin_usable(const srt_pt_skin* k, const char* what) {
  if (!k) return srt::fail(SRT_ERR_INVALID, "%s: NULL skin", what);
  if (!k->pt->committed || k->generation != k->pt->scene_generation)
    return srt::fail(SRT_ERR_STATE, "%s: the skin is stale - its context's scene was begun or committed again after srt_pt_skin_create", what);
  return SRT_OK;
}

// The skinning kernels on s, behind whatever wrote the frame's matrices into d_mats there.
void skin_launch(srt_pt_skin* k, hipStream_t s, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  launch_skin_vertices(s, k->d_pos, k->d_nrm, k->nverts, k->d_mats, k->njoints, k->d_off, k->d_jidx, k->d_w, d_pos_out, flat_normals ? nullptr : d_nrm_out);
  if (flat_normals)
    launch_skin_flat_normals(s, d_pos_out, k->d_nrm, k->pt->d_idx + k->pt->idx_off[k->object], k->ntri, k->d_last, k->nverts, d_nrm_out);
}

// Enqueues the frame's matrices and the skinning kernels on s, for a skin that is usable.
int skin_enqueue(srt_pt_skin* k, const char* what, hipStream_t s, const float* posed, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  const int usable = skin_usable(k, what);
  if (usable != SRT_OK) return usable;
  SRT_HIP(hipSetDevice(k->pt->device));
  for (uint32_t j = 0; j < k->njoints; j++) skin_mat4_mul(posed + 16 * (size_t)j, &k->inv[16 * (size_t)j], &k->mats[16 * (size_t)j]);
  SRT_HIP(hipMemcpyAsync(k->d_mats, k->mats.data(), k->mats.size() * sizeof(float), hipMemcpyHostToDevice, s));   // 64 B per joint
  k->pt->bytes_uploaded += k->mats.size() * sizeof(float);
  skin_launch(k, s, flat_normals, d_pos_out, d_nrm_out);
  return SRT_OK;
}

int skin_rigged(const srt_pt_skin* k, const char* what) {
  const int usable = skin_usable(k, what);
  if (usable != SRT_OK) return usable;
  if (!k->rigged) return srt::fail(SRT_ERR_STATE, "%s: the skin has no rig (srt_pt_skin_set_rig)", what);
  return SRT_OK;
}

// The joint kernels for time t on s: Mat4::euler(pose) per joint, then the chains - into the skin's matrices (to_mats) and / or d_posed_out.
void rig_launch(srt_pt_skin* k, hipStream_t s, float t, bool to_mats, float* d_posed_out) {
  launch_anim_joints(s, k->d_parent, k->d_cap, k->d_base, k->d_rest_pose, k->d_knot_offsets, k->d_knot_times, k->d_knot_quats, k->njoints, t, k->d_local,
                     k->d_inv, to_mats ? k->d_mats : nullptr, d_posed_out);
}

// The same with the matrices from the rig at time t: the joint kernels write them where the skinning kernels read them; nothing goes up.
int skin_enqueue_at(srt_pt_skin* k, const char* what, hipStream_t s, float t, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  const int rigged = skin_rigged(k, what);
  if (rigged != SRT_OK) return rigged;
  SRT_HIP(hipSetDevice(k->pt->device));
  rig_launch(k, s, t, true, nullptr);
  skin_launch(k, s, flat_normals, d_pos_out, d_nrm_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

// srt_pt_skin_pose / srt_pt_skin_pose_refit: the frame's vertices into the skin's staging, then update_mesh or refit_mesh from there.
// (The staging is read by nothing of the context: writing it before the verdict changes no scene.)
int skin_pose(srt_pt_skin* skin, const char* what, void* stream, const float* posed, int flat_normals, decltype(update_mesh)* mesh_call) {
  if (!skin || !posed) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_enqueue(skin, what, (hipStream_t)stream, posed, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  return mesh_call(skin->pt, what, (hipStream_t)stream, skin->object, {nullptr, nullptr, skin->d_pos_out, skin->d_nrm_out, {}, {}}, skin->nverts);
}

int skin_pose_at(srt_pt_skin* skin, const char* what, void* stream, float t, int flat_normals, decltype(update_mesh)* mesh_call) {
  if (!skin) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_enqueue_at(skin, what, (hipStream_t)stream, t, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  return mesh_call(skin->pt, what, (hipStream_t)stream, skin->object, {nullptr, nullptr, skin->d_pos_out, skin->d_nrm_out, {}, {}}, skin->nverts);
}

int timeline_usable(const srt_pt_timeline* tl, const char* what) {
  if (!tl) return srt::fail(SRT_ERR_INVALID, "%s: NULL timeline", what);
  if (!tl->pt->committed || tl->generation != tl->pt->scene_generation)
    return srt::fail(SRT_ERR_STATE, "%s: the timeline is stale - its context's scene was begun or committed again after srt_pt_timeline_create", what);
  return SRT_OK;
}

// Usable, on a device context, and the transforms of time t enqueued on s into the timeline's own buffer.
int timeline_enqueue(srt_pt_timeline* tl, const char* what, hipStream_t s, float t, float* d_out) {
  const int usable = timeline_usable(tl, what);
  if (usable != SRT_OK) return usable;
  if (tl->pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the kernels run on the device only; this context is host-only (srt_pt_timeline_transforms is the host form)", what);
  SRT_HIP(hipSetDevice(tl->pt->device));
  launch_anim_pose(s, tl->d_track_offsets, tl->d_knot_times, tl->d_knot_values, (uint32_t)tl->objects.size(), t, d_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

// What srt_pt_skin_set_rig refuses about its arrays, as a message (empty: nothing).
std::string check_rig(uint32_t njoints, const int32_t* parent, const uint32_t* knot_offsets, const float* knot_times) {
  for (uint32_t j = 0; j < njoints; j++)
    if (parent[j] < -1 || parent[j] >= (int32_t)j)
      return "joint " + std::to_string(j) + " has parent " + std::to_string(parent[j]) + " (-1, or a joint in front of it: parents come first, as Skeleton::for_joints visits them)";
  return anim_check_tracks(knot_offsets, njoints, 1, knot_times, false, "joint");
}

std::vector<Mat4> matrices(const float* trans, uint32_t n) {
  static_assert(sizeof(Mat4) == 16 * sizeof(float), "Mat4 is sixteen floats");
  std::vector<Mat4> T(n);
  if (n) std::memcpy(T.data(), trans, (size_t)n * sizeof(Mat4));
  return T;
}

// The listed area lights (srt_pt_set_dynamic_lights): {position in the list, light} pairs as the light kernels take them, and the largest triangle count.
struct ListedLights { std::vector<uint32_t> pairs; uint32_t max_ntri = 0; };
ListedLights listed_lights(const BuiltScene& built, const uint32_t* objects, uint32_t n) {
  ListedLights L;
  for (uint32_t k = 0; k < n; k++) {
    const int32_t li = built.inputs[objects[k]].is_light ? light_of(built, objects[k]) : -1;   // (light_of counts the lights in front)
    if (li < 0) continue;
    L.pairs.push_back(k);
    L.pairs.push_back((uint32_t)li);
    L.max_ntri = std::max(L.max_ntri, built.flat.lights[(size_t)li].ntri);
  }
  return L;
}

// Host forms: the listed lights' records as the host mirror has them now.
int upload_listed_lights(srt_pt* pt, const uint32_t* objects, uint32_t n) {
  const ListedLights L = listed_lights(pt->built, objects, n);
  int st = SRT_OK;
  for (size_t q = 1; q < L.pairs.size() && st == SRT_OK; q += 2) st = upload_light(pt, L.pairs[q], false);
  return st;
}

// Device forms: the records of the `nl` lights in d_light_list from the pose kernel's output where it lies (d_pose_out, `n` poses),
// then their area terms under the new pdfT.  No upload.
void launch_listed_lights(srt_pt* pt, hipStream_t s, uint32_t nl, uint32_t max_ntri, uint32_t n) {
  const FlatScene& F = pt->built.flat;
  launch_light_records(s, pt->d_light_list, nl, pt->d_pose_out, n, pt->d_lights, (uint32_t)F.lights.size());
  launch_light_area_terms(s, pt->d_light_list, nl, max_ntri, pt->d_lights, (uint32_t)F.lights.size(), F.light_tri_first, pt->d_ltris, (uint32_t)F.light_tris.size());
}

// The tables the pose kernels work in, made at the first device-form repose after a commit or after a call that dropped them: the
// records by insertion index come from the live records (a kernel on `s`; nothing goes up), the posed boxes from them and the
// object-space boxes (24 B per object up, added to *bytes).
int ensure_pose_tables(srt_pt* pt, hipStream_t s, const char* what, uint64_t* bytes) {
  if (pt->pose_tables) return SRT_OK;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  const size_t room = nobj ? nobj : 1;
  drop_pose_tables(pt);
  if (pt->d_pose_records.ensure(room) || pt->d_local_boxes.ensure(room * 6) || pt->d_posed_boxes.ensure(room * 6)) {
    (void)hipGetLastError();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  // (blocking copy, then kernels on `s` that read what the last commit or repose left in d_objects: all of it done by now)
  if (nobj) SRT_HIP(hipMemcpy(pt->d_local_boxes, pt->built.local_boxes.data(), (size_t)nobj * 6 * sizeof(float), hipMemcpyHostToDevice));
  *bytes += (uint64_t)nobj * 6 * sizeof(float);
  launch_pose_tables(s, pt->d_objects, nobj, pt->built.flat.tlas_nodes, pt->d_pose_records, pt->d_local_boxes, pt->d_posed_boxes);
  pt->pose_tables = true;
  return SRT_OK;
}

// A pinned staging buffer of at least `words` words whose last copy has left it (or a new one).
int pinned_list(srt_pt* pt, size_t words, srt_pt::PinnedList** out) {
  for (auto& pl : pt->pinned) {
    if (pl.h.capacity() < words) continue;
    const hipError_t left = hipEventQuery(pl.done);
    (void)hipGetLastError();                              // (hipErrorNotReady of a query is no error: not left behind for the launch check)
    if (left == hipSuccess) { *out = &pl; return SRT_OK; }
  }
  srt_pt::PinnedList pl;
  if (pl.h.ensure(std::max<size_t>(words, 1024))) return srt::fail(SRT_ERR_HIP, "out of pinned host memory");
  if (pl.done.create(hipEventDisableTiming)) return srt::fail(SRT_ERR_HIP, "event creation failed");
  pt->pinned.push_back(std::move(pl));
  *out = &pt->pinned.back();
  return SRT_OK;
}

// srt_pt_repose_refit's device side after apply_top_refit: the arrays that changed, from the host's record.
int write_top_refit(srt_pt* pt, const uint32_t* objects, uint32_t n) {
  const FlatScene& F = pt->built.flat;
  if (F.use_bvh) {
    if (F.tlas_nodes) SRT_HIP(hipMemcpy(pt->d_nodes, F.nodes.data(), (size_t)F.tlas_nodes * sizeof(Node), hipMemcpyHostToDevice));
    if (!F.wave_tlas.empty()) SRT_HIP(hipMemcpy(pt->d_wave, F.wave_tlas.data(), F.wave_tlas.size() * sizeof(WaveInterior), hipMemcpyHostToDevice));
    pt->bytes_uploaded += (uint64_t)F.tlas_nodes * sizeof(Node) + F.wave_tlas.size() * sizeof(WaveInterior);
  }
  // the listed records, one copy per run of neighbouring slots (a pool that moves as a whole is a handful of runs)
  std::vector<uint32_t> slot_of(pt->built.tlas.prim.size()), slots(n);
  for (size_t k = 0; k < slot_of.size(); k++) slot_of[pt->built.tlas.prim[k]] = (uint32_t)k;
  for (uint32_t k = 0; k < n; k++) slots[k] = slot_of[objects[k]];
  std::sort(slots.begin(), slots.end());
  for (uint32_t k = 0; k < n;) {
    uint32_t e = k + 1;
    while (e < n && slots[e] == slots[e - 1] + 1u) e++;
    SRT_HIP(hipMemcpy(pt->d_objects + slots[k], &F.objects[slots[k]], (size_t)(e - k) * sizeof(Object), hipMemcpyHostToDevice));
    pt->bytes_uploaded += (uint64_t)(e - k) * sizeof(Object);
    k = e;
  }
  return upload_listed_lights(pt, objects, n);
}


// ---- new values for a committed scene: srt_pt_update_materials / srt_pt_update_lights / srt_pt_update_env_light and the shading timelines ----
const char* material_type_name(uint32_t type) {
  static const char* names[] = {"Lambertian", "Mirror", "Glass", "Diffuse Light", "Refract"};
  return type <= SRT_MAT_REFRACT ? names[type] : "unknown";
}

// What the calls refuse about a list of indices into a table of `size` records, as a message (empty: nothing).
std::string check_index_list(const uint32_t* list, uint32_t n, size_t size, const char* item) {
  std::vector<uint8_t> seen(size, 0);
  for (uint32_t k = 0; k < n; k++) {
    if (list[k] >= size) return std::string(item) + " " + std::to_string(list[k]) + " (entry " + std::to_string(k) + ") is out of range: the scene has " + std::to_string(size);
    if (seen[list[k]]) return std::string(item) + " " + std::to_string(list[k]) + " is listed twice";
    seen[list[k]] = 1;
  }
  return std::string();
}

// The record the kernels read, from a material as srt_pt_add_material takes it: what build_scene makes of it at a commit.
Material material_record(const srt_pt_material& m) {
  Material r;
  r.type = m.type;
  for (int i = 0; i < 3; i++) { r.a[i] = m.a[i]; r.b[i] = m.b[i]; }
  r.ior = m.ior;
  anim_material_store(&r);
  return r;
}

// The verdict is in and nothing of the context is in flight: the listed records into the host's record and, one copy per record, onto the device.
template <typename T>
int write_records(srt_pt* pt, std::vector<T>* host, T* d_table, const uint32_t* list, const std::vector<T>& fresh) {
  for (size_t k = 0; k < fresh.size(); k++) (*host)[list[k]] = fresh[k];
  if (pt->device < 0) return SRT_OK;
  for (size_t k = 0; k < fresh.size(); k++) SRT_HIP(hipMemcpy(d_table + list[k], &fresh[k], sizeof(T), hipMemcpyHostToDevice));
  pt->bytes_uploaded += fresh.size() * sizeof(T);
  return SRT_OK;
}

int update_materials(srt_pt* pt, const char* what, const uint32_t* materials, const srt_pt_material* m, uint32_t n) {
  if (!pt || (n && (!materials || !m))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  FlatScene& F = pt->built.flat;
  const std::string refused = check_index_list(materials, n, F.materials.size(), "material");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<Material> fresh(n);
  for (uint32_t k = 0; k < n; k++) {
    if (m[k].type != F.materials[materials[k]].type)
      return srt::fail(SRT_ERR_INVALID, "%s: material %u was committed as %s (type %u) and cannot become %s (type %u): the type decides the light list, the instancing rules and the elision proof - commit again",
                       what, materials[k], material_type_name(F.materials[materials[k]].type), F.materials[materials[k]].type, material_type_name(m[k].type), m[k].type);
    fresh[k] = material_record(m[k]);
  }
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  return written(pt, write_records(pt, &F.materials, pt->d_mats.get(), materials, fresh));
}

int update_lights(srt_pt* pt, const char* what, const uint32_t* lights, const float* radiance, const float* angle_bounds, const float* trans, uint32_t n) {
  if (!pt || (n && (!lights || !radiance || !trans))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  FlatScene& F = pt->built.flat;
  const std::string refused = check_index_list(lights, n, F.delta_lights.size(), "light");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<DeltaLight> fresh(n);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t type = F.delta_lights[lights[k]].type;
    if (type == DL_SPOT && !angle_bounds) return srt::fail(SRT_ERR_INVALID, "%s: light %u is a spot light and needs angle_bounds", what, lights[k]);
    Mat4 T;
    std::memcpy(&T, trans + 16 * (size_t)k, sizeof(Mat4));
    fresh[k] = make_delta_light(type, radiance + 3 * (size_t)k, angle_bounds ? angle_bounds + 2 * (size_t)k : nullptr, T);
  }
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  return written(pt, write_records(pt, &F.delta_lights, pt->d_dlights.get(), lights, fresh));
}

int update_env_light(srt_pt* pt, const char* what, const float radiance[3]) {
  if (!pt || !radiance) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  if (pt->env_type != SRT_ENV_SPHERE && pt->env_type != SRT_ENV_HEMISPHERE)
    return srt::fail(SRT_ERR_INVALID, "%s: the scene was committed %s; a radiance is what a sphere or hemisphere environment light has", what,
                     pt->env_type == SRT_ENV_MAP ? "with an environment map" : "without an environment light");
  for (int i = 0; i < 3; i++) pt->env_radiance[i] = radiance[i];
  return SRT_OK;
}

int shading_usable(const srt_pt_shading_timeline* tl, const char* what) {
  if (!tl) return srt::fail(SRT_ERR_INVALID, "%s: NULL timeline", what);
  if (!tl->pt->committed || tl->generation != tl->pt->scene_generation)
    return srt::fail(SRT_ERR_STATE, "%s: the timeline is stale - its context's scene was begun or committed again after srt_pt_shading_timeline_create", what);
  return SRT_OK;
}

// The host form: every listed item at time t from the host's record of the scene (the committed types; the values a light's triple
// without a key keeps).  lights21: radiance3, angle_bounds2, trans16 per light.
void shading_values(const srt_pt_shading_timeline* tl, float t, srt_pt_material* materials, float* lights21, float env[3]) {
  const FlatScene& F = tl->pt->built.flat;
  const uint32_t nm = (uint32_t)tl->materials.size(), nl = (uint32_t)tl->lights.size();
  const uint32_t* off = tl->track_offsets.data();
  for (uint32_t k = 0; k < nm; k++) {
    Material m;
    m.type = F.materials[tl->materials[k]].type;
    anim_material_item(off, tl->knot_times.data(), tl->knot_values.data(), k, t, &m);
    materials[k].type = m.type;
    for (int i = 0; i < 3; i++) { materials[k].a[i] = m.a[i]; materials[k].b[i] = m.b[i]; }
    materials[k].ior = m.ior;
  }
  for (uint32_t j = 0; j < nl; j++) {
    const DeltaLight& L = F.delta_lights[tl->lights[j]];
    AnimLightOut out;
    anim_light_item(off + 6 * (size_t)nm + 6 * (size_t)j, tl->knot_times.data(), tl->knot_values.data(), t, &out);
    float* o = lights21 + 21 * (size_t)j;
    for (int i = 0; i < 3; i++) o[i] = out.options ? out.radiance[i] : L.radiance[i];
    for (int i = 0; i < 2; i++) o[3 + i] = out.options ? out.angle_bounds[i] : L.angle_bounds[i];
    if (out.pose) std::memcpy(o + 5, out.trans, 16 * sizeof(float));
    else std::memcpy(o + 5, &L.trans, 16 * sizeof(float));
  }
  if (tl->env) anim_env_item(off + 6 * (size_t)nm + 6 * (size_t)nl, tl->knot_times.data(), tl->knot_values.data(), t, env);
}

}  // namespace

namespace srt {

void drop_update_tables(srt_pt* pt, uint32_t object) { drop_refit_tables(pt, object); drop_pose_tables(pt); drop_top_tables(pt); }

// The host's record catches up with the device after srt_pt_repose_refit_device calls: one wait for the event behind the last of
// them, one read-back (176 B per object: the records by insertion index; 24 B per node: the top-level boxes), and the scene
// layer's own apply_top_refit - the lights' records come from the host's light_record / light_area_term.  With nothing pending it
// does nothing.
// The same after srt_pt_shading_timeline_apply calls: one wait for the event behind the last of them, d_mats and / or d_dlights read back
// once (32 B per material, 160 B per light) into the host's record.
static int settle_shading(srt_pt* pt) {
  if (!pt->shade_pending_mats && !pt->shade_pending_lights) return SRT_OK;
  const bool mats = pt->shade_pending_mats, lights = pt->shade_pending_lights;
  pt->shade_pending_mats = pt->shade_pending_lights = false;
  if (!pt->committed) return SRT_OK;                      // (a failure took the scene away: there is no record to bring up to date)
  FlatScene& F = pt->built.flat;
  if (hipSetDevice(pt->device) != hipSuccess || hipEventSynchronize(pt->shade_event) != hipSuccess ||
      (mats && !F.materials.empty() && hipMemcpy(F.materials.data(), pt->d_mats, F.materials.size() * sizeof(Material), hipMemcpyDeviceToHost) != hipSuccess) ||
      (lights && !F.delta_lights.empty() &&
       hipMemcpy(F.delta_lights.data(), pt->d_dlights, F.delta_lights.size() * sizeof(DeltaLight), hipMemcpyDeviceToHost) != hipSuccess)) {
    pt->committed = false;
    return srt::fail(SRT_ERR_HIP, "settling srt_pt_shading_timeline_apply: %s; the scene has to be committed again", hipGetErrorString(hipGetLastError()));
  }
  return SRT_OK;
}

static int settle_top(srt_pt* pt);
int settle(srt_pt* pt) {
  if (!pt) return SRT_OK;
  const int st = settle_top(pt);
  return st != SRT_OK ? st : settle_shading(pt);
}

static int settle_top(srt_pt* pt) {
  if (!pt->top_pending) return SRT_OK;
  if (!pt->committed) { discard_pending(pt); return SRT_OK; }   // (a failure took the scene away: there is no record to bring up to date)
  const uint64_t calls = pt->top_pending;
  std::vector<uint32_t> objects = pt->top_pending_objects;
  forget_pending(pt);
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  const bool use_bvh = pt->built.flat.use_bvh;
  std::vector<Object> records(nobj);
  TopRefit R;
  if (use_bvh) R.boxes.resize(6 * (size_t)pt->top_tables.nnodes);
  if (hipSetDevice(pt->device) != hipSuccess || hipEventSynchronize(pt->top_event) != hipSuccess ||
      (nobj && hipMemcpy(records.data(), pt->d_pose_records, (size_t)nobj * sizeof(Object), hipMemcpyDeviceToHost) != hipSuccess) ||
      (!R.boxes.empty() && hipMemcpy(R.boxes.data(), pt->top_tables.d_node_boxes, R.boxes.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
    pt->committed = false;
    return srt::fail(SRT_ERR_HIP, "settling srt_pt_repose_refit_device: %s; the scene has to be committed again", hipGetErrorString(hipGetLastError()));
  }
  for (uint32_t i : objects) {                            // (every object once: top_pending_flag)
    R.listed.push_back(i);
    R.trans.push_back(records[i].trans);
    R.itrans.push_back(records[i].itrans);
    R.has_trans.push_back(records[i].has_trans);
  }
  apply_top_refit(&pt->built, &R);
  pt->top_refits += calls;
  return SRT_OK;
}

// srt_pt_scene_begin, srt_pt_scene_commit, srt_pt_destroy: wait for what is pending and forget it.
void discard_pending(srt_pt* pt) {
  if (pt->shade_pending_mats || pt->shade_pending_lights) {
    if (hipSetDevice(pt->device) == hipSuccess) (void)hipEventSynchronize(pt->shade_event);
    pt->shade_pending_mats = pt->shade_pending_lights = false;
  }
  if (!pt->top_pending) return;
  if (hipSetDevice(pt->device) == hipSuccess) (void)hipEventSynchronize(pt->top_event);
  pt->top_refits += pt->top_pending;                      // (they ran; only their read-back is not worth making any more)
  forget_pending(pt);
}

int not_committed(const char* what) { return srt::fail(SRT_ERR_STATE, "%s before srt_pt_scene_commit", what); }
int need_committed(srt_pt* pt, const char* what) {
  const int settled = settle(pt);
  return settled != SRT_OK ? settled : pt->committed ? SRT_OK : not_committed(what);
}

bool device_builds(const srt_pt* pt) {
  const char* be = getenv("SRT_BVH_BUILDER");
  return pt->device >= 0 && (be ? strcmp(be, "host") != 0 : pt->bvh_builder != 0);
}

DeviceBuilderScope::DeviceBuilderScope(const srt_pt* pt, bool on) {
  if (on) set_device_bvh_builder(build_bvh_device, pt->bvh_device_min);
  else set_device_bvh_builder(nullptr, 0);
}
DeviceBuilderScope::~DeviceBuilderScope() { set_device_bvh_builder(nullptr, 0); }

// (Calls that replace only the BVH<Object> pass the committed BVH<Triangle> depth, which is within the limit.)
int check_depth(uint32_t tlas_depth, uint32_t blas_depth) {
  if ((int)tlas_depth <= kMaxTlasDepth && (int)blas_depth <= kMaxBlasDepth) return SRT_OK;
  return srt::fail(SRT_ERR_UNSUPPORTED, "BVH too deep for the traversal stacks (TLAS %u > %d or BLAS %u > %d)", tlas_depth, kMaxTlasDepth, blas_depth, kMaxBlasDepth);
}

}  // namespace srt

extern "C" {

int srt_pt_update_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts) {
  if (!pt || !positions || !normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_update_mesh: NULL argument");
  return update_mesh(pt, "srt_pt_update_mesh", pt->stream, object, {positions, normals, nullptr, nullptr, {}, {}}, nverts);
}

int srt_pt_update_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts) {
  if (!pt || !d_positions || !d_normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_update_mesh_device: NULL argument");
  return update_mesh(pt, "srt_pt_update_mesh_device", (hipStream_t)stream, object, {nullptr, nullptr, d_positions, d_normals, {}, {}}, nverts);
}

int srt_pt_refit_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts) {
  if (!pt || !positions || !normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_mesh: NULL argument");
  return refit_mesh(pt, "srt_pt_refit_mesh", pt->stream, object, {positions, normals, nullptr, nullptr, {}, {}}, nverts);
}

int srt_pt_refit_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts) {
  if (!pt || !d_positions || !d_normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_mesh_device: NULL argument");
  return refit_mesh(pt, "srt_pt_refit_mesh_device", (hipStream_t)stream, object, {nullptr, nullptr, d_positions, d_normals, {}, {}}, nverts);
}

int srt_pt_mesh_tree_cost(srt_pt* pt, uint32_t object, double* cost) {
  if (!pt || !cost) return srt::fail(SRT_ERR_INVALID, "srt_pt_mesh_tree_cost: NULL argument");
  if (!pt->committed) return not_committed("srt_pt_mesh_tree_cost");
  const std::string refused = check_mesh_update(pt->built, object, (uint32_t)(object < pt->built.inputs.size() ? pt->built.inputs[object].mesh.pos.size() / 3 : 0));
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "srt_pt_mesh_tree_cost: %s", refused.c_str());
  if (!pt->built.flat.use_bvh) return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_mesh_tree_cost: the scene was committed without BVHs, the mesh has no tree");
  *cost = tree_cost(pt->built.blas[object]);
  return SRT_OK;
}

int srt_pt_refit_count(srt_pt* pt, uint64_t* refits) {
  if (!pt || !refits) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_count: NULL argument");
  *refits = pt->refits;
  return SRT_OK;
}

int srt_pt_skin_create(srt_pt* pt, uint32_t object, const float* bind_positions, const float* bind_normals, uint32_t nverts,
                       const srt_pt_skin_joint* joints, uint32_t njoints, srt_pt_skin** skin) {
  if (skin) *skin = nullptr;
  if (!pt || !bind_positions || !bind_normals || !joints || !skin) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_create: NULL argument");
  if (!pt->committed) return not_committed("srt_pt_skin_create");
  const std::string refused = check_mesh_update(pt->built, object, nverts);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_create: %s", refused.c_str());
  if (njoints == 0) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_create: a skin needs at least one joint");
  if (njoints > kSkinMaxJoints || (uint64_t)nverts * njoints > kSkinMaxPairs)
    return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_skin_create: %u joints on %u vertices (at most %u joints and 2^31 vertex-joint pairs)", njoints, nverts,
                     kSkinMaxJoints);
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_skin_create: skinning runs on the device only; this context is host-only and there is no CPU path");
  srt_pt_skin* k = new (std::nothrow) srt_pt_skin;
  if (!k) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  k->pt = pt; k->generation = pt->scene_generation; k->object = object; k->nverts = nverts; k->njoints = njoints;
  k->ntri = pt->built.store[object].ntri;
  k->inv.resize(16 * (size_t)njoints);
  k->mats.resize(16 * (size_t)njoints);
  int st = SRT_OK;
  if (pt->idx_off[object] == SIZE_MAX) {                  // an emissive mesh under srt_pt_set_dynamic_lights: its index buffer goes up now
    if (quiesce(pt) != hipSuccess) st = srt::fail(SRT_ERR_HIP, "srt_pt_skin_create: synchronisation failed");
    else st = ensure_mesh_idx(pt, object);
    if (st == SRT_OK) { pt->bytes_uploaded += pt->idx_uncounted; pt->idx_uncounted = 0; }
  }
  if (st == SRT_OK) st = skin_build(k, bind_positions, bind_normals, joints);
  if (st != SRT_OK) { delete k; return st; }
  *skin = k;
  return SRT_OK;
}

int srt_pt_skin_destroy(srt_pt_skin* skin) {
  if (!skin) return SRT_OK;
  if (skin->pt->device >= 0) (void)quiesce(skin->pt);
  delete skin;
  return SRT_OK;
}

int srt_pt_skin_counts(srt_pt_skin* skin, uint32_t out[4]) {
  if (!skin || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_counts: NULL argument");
  out[0] = skin->nverts; out[1] = skin->njoints; out[2] = skin->ninf; out[3] = skin->ntri;
  return SRT_OK;
}

int srt_pt_skin_map(srt_pt_skin* skin, uint32_t* offsets, uint32_t* joints, float* weights, uint32_t cap) {
  if (!skin || !offsets || !joints || !weights) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_map: NULL argument");
  int st = skin_usable(skin, "srt_pt_skin_map");
  if (st != SRT_OK) return st;
  if (cap < skin->ninf) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_map: the map has %u influences, the arrays hold %u", skin->ninf, cap);
  SRT_HIP(hipSetDevice(skin->pt->device));
  SRT_HIP(hipMemcpy(offsets, skin->d_off, ((size_t)skin->nverts + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (skin->ninf) {
    SRT_HIP(hipMemcpy(joints, skin->d_jidx, (size_t)skin->ninf * sizeof(uint32_t), hipMemcpyDeviceToHost));
    SRT_HIP(hipMemcpy(weights, skin->d_w, (size_t)skin->ninf * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SRT_OK;
}

int srt_pt_skin_vertices_device(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals, float* d_positions_out, float* d_normals_out) {
  if (!skin || !posed || !d_positions_out || !d_normals_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_vertices_device: NULL argument");
  return skin_enqueue(skin, "srt_pt_skin_vertices_device", (hipStream_t)stream, posed, flat_normals, d_positions_out, d_normals_out);
}

int srt_pt_skin_vertices(srt_pt_skin* skin, const float* posed, int flat_normals, float* positions_out, float* normals_out) {
  if (!skin || !posed || !positions_out || !normals_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_vertices: NULL argument");
  hipStream_t s = skin->pt->stream;
  const int st = skin_enqueue(skin, "srt_pt_skin_vertices", s, posed, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  const size_t bytes = 3 * (size_t)skin->nverts * sizeof(float);
  SRT_HIP(hipMemcpyAsync(positions_out, skin->d_pos_out, bytes, hipMemcpyDeviceToHost, s));
  SRT_HIP(hipMemcpyAsync(normals_out, skin->d_nrm_out, bytes, hipMemcpyDeviceToHost, s));
  SRT_HIP(hipStreamSynchronize(s));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_skin_pose(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals) {
  return skin_pose(skin, "srt_pt_skin_pose", stream, posed, flat_normals, update_mesh);
}

int srt_pt_skin_pose_refit(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals) {
  return skin_pose(skin, "srt_pt_skin_pose_refit", stream, posed, flat_normals, refit_mesh);
}

int srt_pt_repose(srt_pt* pt, const uint32_t* objects, const float* trans, uint32_t n) {
  if (!pt || (n && (!objects || !trans))) return srt::fail(SRT_ERR_INVALID, "srt_pt_repose: NULL argument");
  int st;
  if ((st = need_committed(pt, "srt_pt_repose"))) return st;
  const bool on_device = pt->device >= 0;
  if (on_device) SRT_HIP(hipSetDevice(pt->device));
  const DeviceBuilderScope builder(pt, device_builds(pt));   // the BVH<Object> build goes where srt_pt_scene_commit's does
  ReposedTop top;
  bool bad_argument = false;
  const std::string err = prepare_repose(pt->built, objects, matrices(trans, n).data(), n, &top, &bad_argument);
  if (!err.empty()) return srt::fail(bad_argument ? SRT_ERR_INVALID : SRT_ERR_UNSUPPORTED, "srt_pt_repose: %s", err.c_str());
  if ((st = check_depth(top.max_tlas_depth, pt->built.flat.max_blas_depth))) return st;
  // from here on nothing fails on the host side: the new tables replace the old ones
  const size_t old_tlas_nodes = pt->built.flat.tlas_nodes;
  if (on_device) SRT_HIP(quiesce(pt));
  apply_repose(&pt->built, &top);
  pt->cast_blocks = 0;                                    // the ray-cast kernel's stack depth follows the scene
  if (!on_device) return SRT_OK;
  drop_pose_tables(pt);                                   // srt_pt_repose_device's tables mirror the poses that were just replaced
  drop_top_tables(pt);                                    // srt_pt_repose_refit_device's describe the tree that was just replaced
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_level(pt, pt->stream, old_tlas_nodes))) return w;
    SRT_HIP(hipStreamSynchronize(pt->stream));            // (a host form returns with its copies complete)
    if ((w = upload_object_tables(pt))) return w;
    return upload_listed_lights(pt, objects, n);
  };
  return written(pt, write());
}

int srt_pt_repose_device(srt_pt* pt, void* stream, const uint32_t* objects, const float* d_trans, uint32_t n) {
  const char* what = "srt_pt_repose_device";
  if (!pt || (n && (!objects || !d_trans))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  const std::string refused = check_repose_list(pt->built, objects, n);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the poses are computed on the device only; this context is host-only (srt_pt_repose takes host matrices)", what);
  SRT_HIP(hipSetDevice(pt->device));
  forget_top_list(pt);                                    // d_pose_list and d_light_list are about to hold this call's lists
  hipStream_t s = (hipStream_t)stream;
  const bool use_bvh = pt->built.flat.use_bvh;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  uint64_t staged_bytes = 0;                              // (counted with the verdict: a refused repose adds nothing to the figures)
  if ((st = ensure_pose_tables(pt, s, what, &staged_bytes))) return st;
  // From here to the verdict only these tables and the staging are written; a refusal drops the tables (the next call makes them
  // again from the committed records, which are not touched).
  auto refuse = [&](int status) { drop_pose_tables(pt); return status; };
  auto copy_failed = [&] { return refuse(srt::fail(SRT_ERR_HIP, "%s: copy failed", what)); };
  std::vector<PoseOut> posed(n);
  std::vector<float> boxes;
  if (n) {
    if ((st = pt->d_pose_list.ensure(n)) || (st = pt->d_pose_out.ensure(n))) return refuse(st);
    if (hipMemcpyAsync(pt->d_pose_list, objects, (size_t)n * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
    staged_bytes += (uint64_t)n * 4;
    launch_pose_objects(s, pt->d_pose_list, d_trans, n, nobj, pt->d_local_boxes, pt->d_pose_out, pt->d_pose_records, pt->d_posed_boxes);
    if (hipMemcpyAsync(posed.data(), pt->d_pose_out, (size_t)n * sizeof(PoseOut), hipMemcpyDeviceToHost, s) != hipSuccess) return copy_failed();
  }
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return refuse(srt::fail(SRT_ERR_HIP, "%s: the pose kernel failed", what));
  // The BVH<Object> build goes where srt_pt_repose's does: on the device, over the boxes where they are, for a scene at or above
  // the device builder's threshold; anything else - and a device build that failed: the host build gives the verdict - on the host,
  // over the boxes read back (24 B per object).
  HostBVH device_tree;
  bool device_built = false;
  if (use_bvh && device_builds(pt) && nobj >= pt->bvh_device_min && nobj > 1u && bvh_workspace_reserve(&pt->bvh_ws, nobj, false)) {
    device_built = build_bvh_device_core(&pt->bvh_ws, s, pt->d_posed_boxes, nobj, 1, &device_tree);   // over the posed boxes where they are
  }
  if (use_bvh && !device_built) {
    boxes.resize((size_t)nobj * 6);
    if (hipMemcpyAsync(boxes.data(), pt->d_posed_boxes, boxes.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return copy_failed();
  }
  std::vector<Mat4> trans(n), itrans(n);
  std::vector<uint32_t> has_trans(n);
  for (uint32_t k = 0; k < n; k++) {
    std::memcpy(&trans[k], posed[k].trans, sizeof(Mat4));
    std::memcpy(&itrans[k], posed[k].itrans, sizeof(Mat4));
    has_trans[k] = posed[k].has_trans;
    // (with a device-built tree the posed box has served already; the host's record holds it in the tree's leaves)
  }
  SuppliedPoses P;
  P.trans = trans.data(); P.itrans = itrans.data(); P.has_trans = has_trans.data();
  P.boxes6 = boxes.empty() ? nullptr : boxes.data();
  P.prebuilt = device_built ? &device_tree : nullptr;
  const DeviceBuilderScope builder(pt, false);            // (the tree is supplied, or built on the host)
  ReposedTop top;
  bool bad_argument = false;
  const std::string err = prepare_repose_supplied(pt->built, objects, n, P, &top, &bad_argument);
  if (!err.empty()) return refuse(srt::fail(bad_argument ? SRT_ERR_INVALID : SRT_ERR_UNSUPPORTED, "%s: %s", what, err.c_str()));
  if ((st = check_depth(top.max_tlas_depth, pt->built.flat.max_blas_depth))) return refuse(st);
  // the primitive order and the mesh ordinals per slot, still aside: a host build's order goes up (4 B per slot), a device build's
  // is where the record kernel reads it; the ordinals (bits 8 and up of use_bvh) are the host's
  const uint32_t *d_prim = nullptr, *d_ordinal = nullptr;
  std::vector<uint32_t> ordinal;
  if (use_bvh) {
    if (!device_built) {
      if (!bvh_workspace_reserve(&pt->bvh_ws, nobj, true)) return refuse(srt::fail(SRT_ERR_HIP, "%s: out of device memory", what));
      if (hipMemcpyAsync(pt->bvh_ws.d_prim, top.tlas.prim.data(), (size_t)nobj * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
      staged_bytes += (uint64_t)nobj * 4;
    }
    d_prim = pt->bvh_ws.d_prim;
    if (!top.lazy_objects.empty()) {
      ordinal.assign(nobj, 0u);
      for (size_t q = 0; q < top.lazy_objects.size(); q++) ordinal[top.lazy_objects[q]] = (uint32_t)q << 8;
      if ((st = pt->d_slot_ordinal.ensure(nobj))) return refuse(st);
      if (hipMemcpyAsync(pt->d_slot_ordinal, ordinal.data(), (size_t)nobj * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
      staged_bytes += (uint64_t)nobj * 4;
      d_ordinal = pt->d_slot_ordinal;
    }
  }
  // the listed area lights (srt_pt_set_dynamic_lights), still aside
  const ListedLights lights = listed_lights(pt->built, objects, n);
  if (!lights.pairs.empty()) {
    if ((st = pt->d_light_list.ensure(lights.pairs.size()))) return refuse(st);
    if (hipMemcpyAsync(pt->d_light_list, lights.pairs.data(), lights.pairs.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
    staged_bytes += (uint64_t)lights.pairs.size() * 4;
  }
  // the verdict is in; nothing of the context may be in flight while the live arrays change
  const size_t old_tlas_nodes = pt->built.flat.tlas_nodes;
  if (hipStreamSynchronize(s) != hipSuccess || quiesce(pt) != hipSuccess) return refuse(srt::fail(SRT_ERR_HIP, "%s: synchronisation failed", what));
  apply_repose(&pt->built, &top);
  drop_top_tables(pt);                                    // srt_pt_repose_refit_device's describe the tree that was just replaced
  pt->cast_blocks = 0;                                    // the ray-cast kernel's stack depth follows the scene
  pt->bytes_uploaded += staged_bytes;
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_level(pt, s, old_tlas_nodes))) return w;
    // the records in place (the object count never changes): gathered on the device by the new order
    launch_pose_records(s, pt->d_pose_records, d_prim, d_ordinal, nobj, pt->built.flat.tlas_nodes, pt->d_objects);
    if (!lights.pairs.empty()) launch_listed_lights(pt, s, (uint32_t)(lights.pairs.size() / 2), lights.max_ntri, n);
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    return upload_object_tables(pt, false);
  };
  st = written(pt, write());
  if (st != SRT_OK) drop_pose_tables(pt);
  return st;
}

int srt_pt_repose_refit(srt_pt* pt, const uint32_t* objects, const float* trans, uint32_t n) {
  if (!pt || (n && (!objects || !trans))) return srt::fail(SRT_ERR_INVALID, "srt_pt_repose_refit: NULL argument");
  int st;
  if ((st = need_committed(pt, "srt_pt_repose_refit"))) return st;
  TopRefit R;
  const std::string err = prepare_top_refit(pt->built, objects, matrices(trans, n).data(), n, &R);
  if (!err.empty()) return srt::fail(SRT_ERR_INVALID, "srt_pt_repose_refit: %s", err.c_str());
  // nothing fails on the host side from here on: the new boxes and records replace the old ones in place
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  apply_top_refit(&pt->built, &R);
  pt->top_refits++;
  if (pt->device < 0) return SRT_OK;
  drop_pose_tables(pt);                                   // they mirror the poses that were just replaced (the tree's tables stay: the tree did)
  return written(pt, write_top_refit(pt, objects, n));
}

int srt_pt_repose_refit_device(srt_pt* pt, void* stream, const uint32_t* objects, const float* d_trans, uint32_t n) {
  const char* what = "srt_pt_repose_refit_device";
  if (!pt || (n && (!objects || !d_trans))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (!pt->committed) return not_committed(what);         // (no settle(): this call only adds to what is pending)
  const std::string refused = check_repose_list(pt->built, objects, n);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the poses are computed on the device only; this context is host-only (srt_pt_repose_refit takes host matrices)", what);
  SRT_HIP(hipSetDevice(pt->device));
  hipStream_t s = (hipStream_t)stream;
  const FlatScene& F = pt->built.flat;
  const bool use_bvh = F.use_bvh;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  int st;
  // First call after a commit or after a call that replaced the BVH<Object> (blocking, counted once): the pose tables as
  // srt_pt_repose_device makes them (24 B per object up), the tree's refit tables (about 28 B per object up) and the slot of
  // every object (a kernel).  Nothing is pending then - every call that drops these tables settles first.
  if ((st = ensure_pose_tables(pt, s, what, &pt->bytes_uploaded))) return st;
  if (use_bvh && !pt->have_top_tables) {
    drop_top_tables(pt);
    RefitTables fresh;
    if ((st = make_refit_tables(pt->built.tlas, what, UINT32_MAX, &fresh)) != SRT_OK) return st;
    pt->top_tables = std::move(fresh);
    pt->have_top_tables = true;
    pt->bytes_uploaded += pt->top_tables.uncounted_bytes;
    pt->top_tables.uncounted_bytes = 0;
    if (pt->d_slot_of.ensure(nobj ? nobj : 1)) {
      (void)hipGetLastError();
      drop_top_tables(pt);
      return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
    }
    launch_top_slots(s, pt->top_tables.d_prim, nobj, pt->d_slot_of);
  }
  // A HIP failure from here on may leave tables, lists or live arrays half written: the scene is no longer committed, what was
  // pending is forgotten (settle() has no record to bring up to date) and the tables go; the scene has to be committed again.
  auto broken = [&](int status) {
    pt->committed = false;
    if (hipSetDevice(pt->device) == hipSuccess) (void)hipDeviceSynchronize();
    (void)hipGetLastError();
    forget_pending(pt);
    drop_pose_tables(pt);
    drop_top_tables(pt);
    return status;
  };
  auto hip_broken = [&](hipError_t e, const char* step) { return broken(srt::fail(SRT_ERR_HIP, "%s: %s failed (%s); the scene has to be committed again", what, step, hipGetErrorString(e))); };
  hipError_t he;
  // The list (4 B per listed object, 8 B more per listed light), through pinned memory so that the copy is only enqueued - unless
  // the device holds this very list already.
  if (n && !(pt->top_list_valid && pt->top_list.size() == n && std::memcmp(pt->top_list.data(), objects, (size_t)n * 4) == 0)) {
    const ListedLights lights = listed_lights(pt->built, objects, n);
    forget_top_list(pt);
    // (growing one of these arrays frees the old one, which waits for what reads it: first calls and longer lists only)
    if ((st = pt->d_pose_list.ensure(n)) || (st = pt->d_pose_out.ensure(n)) || (!lights.pairs.empty() && (st = pt->d_light_list.ensure(lights.pairs.size()))))
      return broken(st);
    srt_pt::PinnedList* pl = nullptr;
    if ((st = pinned_list(pt, (size_t)n + lights.pairs.size(), &pl)) != SRT_OK) return broken(st);
    uint32_t* const h = pl->h;
    std::memcpy(h, objects, (size_t)n * 4);
    if (!lights.pairs.empty()) std::memcpy(h + n, lights.pairs.data(), lights.pairs.size() * 4);
    if ((he = hipMemcpyAsync(pt->d_pose_list, h, (size_t)n * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return hip_broken(he, "the copy of the list");
    if (!lights.pairs.empty() && (he = hipMemcpyAsync(pt->d_light_list, h + n, lights.pairs.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
      return hip_broken(he, "the copy of the light list");
    if ((he = hipEventRecord(pl->done, s)) != hipSuccess) return hip_broken(he, "hipEventRecord");
    pt->bytes_uploaded += (uint64_t)n * 4 + lights.pairs.size() * 4;
    pt->top_list.assign(objects, objects + n);
    pt->top_lights = (uint32_t)(lights.pairs.size() / 2);
    pt->top_light_max_ntri = lights.max_ntri;
    pt->top_list_valid = true;
  }
  if (pt->top_event.create(hipEventDisableTiming)) return hip_broken(hipGetLastError(), "hipEventCreate");
  // Everything below only enqueues on `s`: the poses, the leaves through the tree's primitive order, the levels deepest first, the
  // boxes into the live nodes and sweep records, the listed records' matrices, the listed lights.  No verdict is needed: depth,
  // counts, order, kernel form and stack sizes are those of the committed tree.
  if (n) launch_pose_objects(s, pt->d_pose_list, d_trans, n, nobj, pt->d_local_boxes, pt->d_pose_out, pt->d_pose_records, pt->d_posed_boxes);
  if (use_bvh) {
    launch_refit_boxes(s, pt->top_tables, pt->d_posed_boxes, pt->top_tables.d_node_boxes);   // the tree's primitives are the objects: their boxes are the pose tables'
    launch_refit_write(s, pt->top_tables, pt->top_tables.d_node_boxes, pt->d_nodes, pt->d_wave);
  }
  if (n) {
    launch_top_objects(s, pt->d_pose_list, n, nobj, use_bvh ? pt->d_slot_of : nullptr, pt->d_pose_records, pt->d_objects);
    if (pt->top_lights) launch_listed_lights(pt, s, pt->top_lights, pt->top_light_max_ntri, n);
  }
  if ((he = hipGetLastError()) != hipSuccess) return hip_broken(he, "a launch");
  if ((he = hipEventRecord(pt->top_event, s)) != hipSuccess) return hip_broken(he, "hipEventRecord");
  // the host's record is behind from here until settle(): one more call, and the objects it listed that no pending call had listed
  pt->top_pending++;
  if (pt->top_pending_flag.size() != nobj) pt->top_pending_flag.assign(nobj, 0);   // (nothing is pending across a commit)
  for (uint32_t k = 0; k < n; k++)
    if (!pt->top_pending_flag[objects[k]]) { pt->top_pending_flag[objects[k]] = 1; pt->top_pending_objects.push_back(objects[k]); }
  return SRT_OK;
}

int srt_pt_skin_set_rig(srt_pt_skin* skin, const int32_t* parent, const float base[3], const float* rest_pose, const uint32_t* knot_offsets,
                        const float* knot_times, const float* knot_quats) {
  const char* what = "srt_pt_skin_set_rig";
  if (!skin || !parent || !base || !rest_pose || !knot_offsets || !knot_times || !knot_quats) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st = skin_usable(skin, what);
  if (st != SRT_OK) return st;
  const uint32_t nj = skin->njoints;
  const std::string refused = check_rig(nj, parent, knot_offsets, knot_times);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt* pt = skin->pt;
  SRT_HIP(quiesce(pt));                                   // (a rig set before may still be read)
  skin_drop_rig(skin);
  const size_t nk = knot_offsets[nj];
  skin->parent.assign(parent, parent + nj);
  skin->rest_pose.assign(rest_pose, rest_pose + 3 * (size_t)nj);
  skin->knot_offsets.assign(knot_offsets, knot_offsets + nj + 1);
  skin->knot_times.assign(knot_times, knot_times + nk);
  skin->knot_quats.assign(knot_quats, knot_quats + 4 * nk);
  std::memcpy(skin->base, base, sizeof skin->base);
  if ((st = skin->d_parent.upload(skin->parent)) || (st = skin->d_base.upload(skin->base, 3)) || (st = skin->d_rest_pose.upload(skin->rest_pose)) ||
      (st = skin->d_knot_offsets.upload(skin->knot_offsets)) || (st = skin->d_knot_times.upload(skin->knot_times)) ||
      (st = skin->d_knot_quats.upload(skin->knot_quats)))
    return st;
  pt->bytes_uploaded += (nj + skin->knot_offsets.size()) * sizeof(uint32_t) + (3 + skin->rest_pose.size() + 5 * nk) * sizeof(float);
  if (skin->d_local.ensure(16 * (size_t)nj)) {
    (void)hipGetLastError();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  skin->rigged = true;
  return SRT_OK;
}

int srt_pt_skin_posed(srt_pt_skin* skin, float t, float* posed_out) {
  if (!skin || !posed_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_posed: NULL argument");
  const int st = skin_rigged(skin, "srt_pt_skin_posed");
  if (st != SRT_OK) return st;
  std::vector<float> local(16 * (size_t)skin->njoints);   // Mat4::euler(pose) per joint: the call's own, so the host form only reads the skin
  anim_rig_posed_host(skin->parent.data(), skin->cap.data(), skin->base, skin->rest_pose.data(), skin->knot_offsets.data(), skin->knot_times.data(),
                      skin->knot_quats.data(), skin->njoints, t, nullptr, local.data(), posed_out);
  return SRT_OK;
}

int srt_pt_skin_posed_device(srt_pt_skin* skin, void* stream, float t, float* d_posed_out) {
  if (!skin || !d_posed_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_posed_device: NULL argument");
  const int st = skin_rigged(skin, "srt_pt_skin_posed_device");
  if (st != SRT_OK) return st;
  SRT_HIP(hipSetDevice(skin->pt->device));
  rig_launch(skin, (hipStream_t)stream, t, false, d_posed_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_skin_vertices_at_device(srt_pt_skin* skin, void* stream, float t, int flat_normals, float* d_positions_out, float* d_normals_out) {
  if (!skin || !d_positions_out || !d_normals_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_vertices_at_device: NULL argument");
  return skin_enqueue_at(skin, "srt_pt_skin_vertices_at_device", (hipStream_t)stream, t, flat_normals, d_positions_out, d_normals_out);
}

int srt_pt_skin_pose_at(srt_pt_skin* skin, void* stream, float t, int flat_normals) {
  return skin_pose_at(skin, "srt_pt_skin_pose_at", stream, t, flat_normals, update_mesh);
}

int srt_pt_skin_pose_refit_at(srt_pt_skin* skin, void* stream, float t, int flat_normals) {
  return skin_pose_at(skin, "srt_pt_skin_pose_refit_at", stream, t, flat_normals, refit_mesh);
}

int srt_pt_rig_posed_host(uint32_t njoints, const int32_t* parent, const float* extents, const float base[3], const float* rest_pose,
                          const uint32_t* knot_offsets, const float* knot_times, const float* knot_quats, float t, float* euler_out, float* posed_out) {
  const char* what = "srt_pt_rig_posed_host";
  if (!parent || !extents || !base || !rest_pose || !knot_offsets || !knot_times || !knot_quats || !posed_out) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const std::string refused = check_rig(njoints, parent, knot_offsets, knot_times);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<float> cap(4 * (size_t)njoints, 0.0f), local(16 * (size_t)njoints);
  for (uint32_t j = 0; j < njoints; j++)
    for (int a = 0; a < 3; a++) cap[4 * (size_t)j + a] = extents[3 * (size_t)j + a];
  anim_rig_posed_host(parent, cap.data(), base, rest_pose, knot_offsets, knot_times, knot_quats, njoints, t, euler_out, local.data(), posed_out);
  return SRT_OK;
}

int srt_pt_timeline_create(srt_pt* pt, const uint32_t* objects, uint32_t nobjects, const uint32_t* track_offsets, const float* knot_times,
                           const float* knot_values, srt_pt_timeline** timeline) {
  const char* what = "srt_pt_timeline_create";
  if (timeline) *timeline = nullptr;
  if (!pt || !objects || !track_offsets || !knot_times || !knot_values || !timeline) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  std::string refused = check_repose_list(pt->built, objects, nobjects);
  if (refused.empty()) refused = anim_check_tracks(track_offsets, nobjects, 3, knot_times, true, "object");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt_timeline* tl = new (std::nothrow) srt_pt_timeline;
  if (!tl) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  const size_t nk = track_offsets[3 * (size_t)nobjects];
  tl->pt = pt; tl->generation = pt->scene_generation;
  tl->objects.assign(objects, objects + nobjects);
  tl->track_offsets.assign(track_offsets, track_offsets + 3 * (size_t)nobjects + 1);
  tl->knot_times.assign(knot_times, knot_times + nk);
  tl->knot_values.assign(knot_values, knot_values + 4 * nk);
  if (pt->device >= 0) {
    auto up = [&]() -> int {
      SRT_HIP(hipSetDevice(pt->device));
      int w;
      if ((w = tl->d_track_offsets.upload(tl->track_offsets)) || (w = tl->d_knot_times.upload(tl->knot_times)) || (w = tl->d_knot_values.upload(tl->knot_values)))
        return w;
      pt->bytes_uploaded += tl->track_offsets.size() * sizeof(uint32_t) + 5 * nk * sizeof(float);
      return tl->d_trans.ensure((nobjects ? (size_t)nobjects : 1) * 16);
    };
    if ((st = up()) != SRT_OK) { delete tl; return st; }
  }
  *timeline = tl;
  return SRT_OK;
}

int srt_pt_timeline_destroy(srt_pt_timeline* timeline) {
  if (!timeline) return SRT_OK;
  if (timeline->pt->device >= 0) (void)quiesce(timeline->pt);
  delete timeline;
  return SRT_OK;
}

int srt_pt_timeline_transforms(srt_pt_timeline* timeline, float t, float* trans_out) {
  if (!timeline || !trans_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_timeline_transforms: NULL argument");
  const int st = timeline_usable(timeline, "srt_pt_timeline_transforms");
  if (st != SRT_OK) return st;
  for (uint32_t k = 0; k < (uint32_t)timeline->objects.size(); k++)
    anim_object_transform(timeline->track_offsets.data(), timeline->knot_times.data(), timeline->knot_values.data(), k, t, nullptr, trans_out + 16 * (size_t)k);
  return SRT_OK;
}

int srt_pt_timeline_transforms_device(srt_pt_timeline* timeline, void* stream, float t, float* d_trans_out) {
  if (!timeline || !d_trans_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_timeline_transforms_device: NULL argument");
  return timeline_enqueue(timeline, "srt_pt_timeline_transforms_device", (hipStream_t)stream, t, d_trans_out);
}

int srt_pt_timeline_repose_refit(srt_pt_timeline* timeline, void* stream, float t) {
  const int st = timeline_enqueue(timeline, "srt_pt_timeline_repose_refit", (hipStream_t)stream, t, timeline ? timeline->d_trans : nullptr);
  if (st != SRT_OK) return st;
  return srt_pt_repose_refit_device(timeline->pt, stream, timeline->objects.data(), timeline->d_trans, (uint32_t)timeline->objects.size());
}

int srt_pt_timeline_repose(srt_pt_timeline* timeline, void* stream, float t) {
  const int st = timeline_enqueue(timeline, "srt_pt_timeline_repose", (hipStream_t)stream, t, timeline ? timeline->d_trans : nullptr);
  if (st != SRT_OK) return st;
  return srt_pt_repose_device(timeline->pt, stream, timeline->objects.data(), timeline->d_trans, (uint32_t)timeline->objects.size());
}

int srt_pt_update_materials(srt_pt* pt, const uint32_t* materials, const srt_pt_material* m, uint32_t n) {
  return update_materials(pt, "srt_pt_update_materials", materials, m, n);
}

int srt_pt_update_lights(srt_pt* pt, const uint32_t* lights, const float* radiance, const float* angle_bounds, const float* trans, uint32_t n) {
  return update_lights(pt, "srt_pt_update_lights", lights, radiance, angle_bounds, trans, n);
}

int srt_pt_update_env_light(srt_pt* pt, const float radiance[3]) { return update_env_light(pt, "srt_pt_update_env_light", radiance); }

int srt_pt_shading_timeline_create(srt_pt* pt, const uint32_t* materials, uint32_t nmaterials, const uint32_t* lights, uint32_t nlights, int env,
                                   const uint32_t* track_offsets, const float* knot_times, const float* knot_values, srt_pt_shading_timeline** out) {
  const char* what = "srt_pt_shading_timeline_create";
  if (out) *out = nullptr;
  if (!pt || (nmaterials && !materials) || (nlights && !lights) || !track_offsets || !knot_times || !knot_values || !out)
    return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  const FlatScene& F = pt->built.flat;
  if (!nmaterials && !nlights && !env) return srt::fail(SRT_ERR_INVALID, "%s: nothing is listed", what);
  if ((uint64_t)nmaterials + nlights > (1u << 28)) return srt::fail(SRT_ERR_INVALID, "%s: %u materials and %u lights", what, nmaterials, nlights);
  std::string refused = check_index_list(materials, nmaterials, F.materials.size(), "material");
  if (refused.empty()) refused = check_index_list(lights, nlights, F.delta_lights.size(), "light");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (env && pt->env_type != SRT_ENV_SPHERE && pt->env_type != SRT_ENV_HEMISPHERE)
    return srt::fail(SRT_ERR_INVALID, "%s: environment keys need a sphere or hemisphere environment light (the scene has %s)", what,
                     pt->env_type == SRT_ENV_MAP ? "an environment map" : "none");
  const uint32_t ntracks = 6u * nmaterials + 6u * nlights + (env ? 2u : 0u);
  refused = anim_check_tracks(track_offsets, ntracks, 1, knot_times, false, "track");
  const uint32_t* lo = track_offsets + 6 * (size_t)nmaterials;
  const char* const no_key = "has no key on any track (Splines::any() is false: the reference would not change it)";
  for (uint32_t k = 0; k < nmaterials && refused.empty(); k++)
    if (track_offsets[6 * (size_t)k] == track_offsets[6 * (size_t)k + 6]) refused = "material " + std::to_string(k) + " of the list " + no_key;
  for (uint32_t j = 0; j < nlights && refused.empty(); j++)
    if (lo[6 * (size_t)j] == lo[6 * (size_t)j + 6]) refused = "light " + std::to_string(j) + " of the list " + no_key;
  if (env && refused.empty() && lo[6 * (size_t)nlights] == lo[6 * (size_t)nlights + 2]) refused = std::string("the environment light ") + no_key;
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt_shading_timeline* tl = new (std::nothrow) srt_pt_shading_timeline;
  if (!tl) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  const size_t nk = track_offsets[ntracks];
  tl->pt = pt; tl->generation = pt->scene_generation; tl->env = env != 0;
  if (nmaterials) tl->materials.assign(materials, materials + nmaterials);
  if (nlights) tl->lights.assign(lights, lights + nlights);
  tl->track_offsets.assign(track_offsets, track_offsets + ntracks + 1);
  tl->knot_times.assign(knot_times, knot_times + nk);
  tl->knot_values.assign(knot_values, knot_values + 4 * nk);
  if (pt->device >= 0) {
    auto up = [&]() -> int {
      SRT_HIP(hipSetDevice(pt->device));
      int w;
      if ((w = tl->d_track_offsets.upload(tl->track_offsets)) || (w = tl->d_materials.upload(tl->materials)) || (w = tl->d_lights.upload(tl->lights)) ||
          (w = tl->d_knot_times.upload(tl->knot_times)) || (w = tl->d_knot_values.upload(tl->knot_values)))
        return w;
      pt->bytes_uploaded += (tl->track_offsets.size() + tl->materials.size() + tl->lights.size()) * sizeof(uint32_t) + 5 * nk * sizeof(float);
      return SRT_OK;
    };
    if ((st = up()) != SRT_OK) { delete tl; return st; }
  }
  *out = tl;
  return SRT_OK;
}

int srt_pt_shading_timeline_destroy(srt_pt_shading_timeline* timeline) {
  if (!timeline) return SRT_OK;
  if (timeline->pt->device >= 0) (void)quiesce(timeline->pt);
  delete timeline;
  return SRT_OK;
}

int srt_pt_shading_timeline_values(srt_pt_shading_timeline* timeline, float t, srt_pt_material* materials_out, float* lights_out, float env_out[3]) {
  const char* what = "srt_pt_shading_timeline_values";
  int st = shading_usable(timeline, what);
  if (st != SRT_OK) return st;
  if ((!timeline->materials.empty() && !materials_out) || (!timeline->lights.empty() && !lights_out) || (timeline->env && !env_out))
    return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if ((st = settle(timeline->pt)) != SRT_OK) return st;   // (a light's triple without a key keeps the record's values)
  shading_values(timeline, t, materials_out, lights_out, env_out);
  return SRT_OK;
}

int srt_pt_shading_timeline_update(srt_pt_shading_timeline* timeline, float t) {
  const char* what = "srt_pt_shading_timeline_update";
  int st = shading_usable(timeline, what);
  if (st != SRT_OK) return st;
  srt_pt* pt = timeline->pt;
  if ((st = settle(pt)) != SRT_OK) return st;
  const uint32_t nm = (uint32_t)timeline->materials.size(), nl = (uint32_t)timeline->lights.size();
  std::vector<srt_pt_material> mats(nm);
  std::vector<float> lights(21 * (size_t)nl), radiance(3 * (size_t)nl), bounds(2 * (size_t)nl), trans(16 * (size_t)nl);
  float env[3] = {0.0f, 0.0f, 0.0f};
  shading_values(timeline, t, mats.data(), lights.data(), env);
  for (uint32_t j = 0; j < nl; j++) {
    std::memcpy(&radiance[3 * (size_t)j], &lights[21 * (size_t)j], 3 * sizeof(float));
    std::memcpy(&bounds[2 * (size_t)j], &lights[21 * (size_t)j + 3], 2 * sizeof(float));
    std::memcpy(&trans[16 * (size_t)j], &lights[21 * (size_t)j + 5], 16 * sizeof(float));
  }
  if (nm && (st = update_materials(pt, what, timeline->materials.data(), mats.data(), nm))) return st;
  if (nl && (st = update_lights(pt, what, timeline->lights.data(), radiance.data(), bounds.data(), trans.data(), nl))) return st;
  if (timeline->env && (st = update_env_light(pt, what, env))) return st;
  return SRT_OK;
}

int srt_pt_shading_timeline_apply(srt_pt_shading_timeline* timeline, void* stream, float t) {
  const char* what = "srt_pt_shading_timeline_apply";
  const int usable = shading_usable(timeline, what);     // (no settle(): this call only adds to what is pending)
  if (usable != SRT_OK) return usable;
  srt_pt* pt = timeline->pt;
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the kernel runs on the device only; this context is host-only (srt_pt_shading_timeline_update is the host form)", what);
  SRT_HIP(hipSetDevice(pt->device));
  const uint32_t nm = (uint32_t)timeline->materials.size(), nl = (uint32_t)timeline->lights.size();
  if (nm + nl) {
    { const int made = pt->shade_event.create(hipEventDisableTiming); if (made != SRT_OK) return made; }
    launch_anim_shading(stream, timeline->d_track_offsets, timeline->d_knot_times, timeline->d_knot_values, timeline->d_materials, nm, timeline->d_lights, nl, t,
                        pt->d_mats, pt->d_dlights);
    // the host's record is behind from here until settle(); a HIP failure leaves a record nobody can vouch for: commit again
    pt->shade_pending_mats = pt->shade_pending_mats || nm != 0;
    pt->shade_pending_lights = pt->shade_pending_lights || nl != 0;
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipEventRecord(pt->shade_event, (hipStream_t)stream);
    if (he != hipSuccess) {
      pt->committed = false;
      pt->shade_pending_mats = pt->shade_pending_lights = false;
      return srt::fail(SRT_ERR_HIP, "%s: the launch failed (%s); the scene has to be committed again", what, hipGetErrorString(he));
    }
  }
  // the environment's radiance is a launch parameter: one item, evaluated here by the function of pt_anim.h, in effect from the next launch
  if (timeline->env)
    anim_env_item(timeline->track_offsets.data() + 6 * (size_t)nm + 6 * (size_t)nl, timeline->knot_times.data(), timeline->knot_values.data(), t, pt->env_radiance);
  return SRT_OK;
}

int srt_pt_dump_shading(srt_pt* pt, int from_device, uint32_t counts[2], srt_pt_material* materials, size_t cap_materials, uint32_t* light_heads,
                        float* light_values, size_t cap_lights, uint32_t* env_type, float env_radiance[3]) {
  const char* what = "srt_pt_dump_shading";
  if (!pt || !counts || (cap_materials && !materials) || (cap_lights && (!light_heads || !light_values))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  { const int ready = need_committed(pt, what); if (ready != SRT_OK) return ready; }
  if (from_device && pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: this context is host-only, there are no device arrays to read (from_device = 0 reads the host's)", what);
  const FlatScene& F = pt->built.flat;
  std::vector<Material> mats(F.materials);
  std::vector<DeltaLight> lights(F.delta_lights);
  if (from_device) {
    SRT_HIP(hipSetDevice(pt->device));
    SRT_HIP(hipDeviceSynchronize());
    if (!mats.empty()) SRT_HIP(hipMemcpy(mats.data(), pt->d_mats, mats.size() * sizeof(Material), hipMemcpyDeviceToHost));
    if (!lights.empty()) SRT_HIP(hipMemcpy(lights.data(), pt->d_dlights, lights.size() * sizeof(DeltaLight), hipMemcpyDeviceToHost));
  }
  counts[0] = (uint32_t)mats.size(); counts[1] = (uint32_t)lights.size();
  for (size_t k = 0; k < mats.size() && k < cap_materials; k++) {
    materials[k].type = mats[k].type;
    for (int i = 0; i < 3; i++) { materials[k].a[i] = mats[k].a[i]; materials[k].b[i] = mats[k].b[i]; }
    materials[k].ior = mats[k].ior;
  }
  for (size_t j = 0; j < lights.size() && j < cap_lights; j++) {
    const DeltaLight& L = lights[j];
    light_heads[2 * j] = L.type; light_heads[2 * j + 1] = L.has_trans;
    float* o = light_values + 37 * j;
    for (int i = 0; i < 3; i++) o[i] = L.radiance[i];
    o[3] = L.angle_bounds[0]; o[4] = L.angle_bounds[1];
    std::memcpy(o + 5, &L.trans, 16 * sizeof(float));
    std::memcpy(o + 21, &L.itrans, 16 * sizeof(float));
  }
  if (env_type) *env_type = pt->env_type;
  if (env_radiance)
    for (int i = 0; i < 3; i++) env_radiance[i] = pt->env_radiance[i];
  return SRT_OK;
}

int srt_pt_scene_tree_cost(srt_pt* pt, double* cost) {
  if (!pt || !cost) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_tree_cost: NULL argument");
  { const int ready = need_committed(pt, "srt_pt_scene_tree_cost"); if (ready != SRT_OK) return ready; }
  if (!pt->built.flat.use_bvh) return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_scene_tree_cost: the scene was committed without BVHs, it has no tree");
  *cost = tree_cost(pt->built.tlas);
  return SRT_OK;
}

int srt_pt_top_refit_pending(srt_pt* pt, uint64_t out[2]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_top_refit_pending: NULL argument");
  out[0] = pt->top_pending;
  out[1] = pt->top_pending_objects.size();
  return SRT_OK;
}

int srt_pt_top_refit_count(srt_pt* pt, uint64_t* refits) {
  if (!pt || !refits) return srt::fail(SRT_ERR_INVALID, "srt_pt_top_refit_count: NULL argument");
  { const int settled = settle(pt); if (settled != SRT_OK) return settled; }
  *refits = pt->top_refits;
  return SRT_OK;
}

int srt_pt_particle_transforms_device(srt_pt* pt, void* stream, const float* d_pos, uint32_t n, float scale, float* d_trans_out) {
  int st = need_device(pt, "srt_pt_particle_transforms_device");
  if (st != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!d_pos || !d_trans_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_particle_transforms_device: NULL argument");
  launch_particle_transforms(stream, d_pos, n, scale, d_trans_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_live_resources(uint64_t out[3]) {
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_live_resources: NULL argument");
  for (int k = 0; k < 3; k++) out[k] = owned_live((OwnedKind)k).load(std::memory_order_relaxed);
  return SRT_OK;
}

int srt_pt_scene_counts(srt_pt* pt, uint64_t out[8]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_counts: NULL argument");
  { const int settled = settle(pt); if (settled != SRT_OK) return settled; }
  const FlatScene& F = pt->built.flat;
  const bool have = pt->committed;
  out[0] = have ? F.objects.size() : 0;
  out[1] = have ? F.tris.size() : 0;
  out[2] = have ? F.nodes.size() - F.tlas_nodes : 0;
  out[3] = have ? F.blas_recs.size() : 0;
  out[4] = pt->blas_builds;
  out[5] = 0;
  if (have && pt->device >= 0)
    out[5] = F.nodes.size() * sizeof(Node) + F.tris.size() * sizeof(Tri) + F.tri_nrm.size() * sizeof(TriNrm) + F.tri_packed.size() * sizeof(float) +
             F.objects.size() * sizeof(Object) + F.lights.size() * sizeof(Light) + F.light_tris.size() * sizeof(LightTri) +
             F.materials.size() * sizeof(Material) + F.wave_tlas.size() * sizeof(WaveInterior) + F.blas_recs.size() * sizeof(WaveInterior) +
             F.wave_lazy.size() * sizeof(uint32_t) + F.delta_lights.size() * sizeof(DeltaLight) + pt->env_map.size() * sizeof(float) +
             pt->idx_words * sizeof(uint32_t);
  out[6] = pt->bytes_uploaded;
  out[7] = pt->tri_bytes_uploaded;
  return SRT_OK;
}

}  // extern "C"

