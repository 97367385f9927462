// New vertices for a committed mesh: srt_pt_update_mesh[_device] rebuilds its BVH<Triangle>, srt_pt_refit_mesh[_device] refits it in
// place, srt_pt_refit_mesh_inplace[_device] refits it and the BVH<Object> above it - the device form only enqueues, and settle_mesh
// brings the host's record up to date later - (the skin poses of pt_update_skin.cpp end in one of the three), and the figures about them.  Host code only: the kernels are in
// pt_mesh_update.hip, pt_light_update.hip and pt_bvh_device.hip, what the update units share in pt_update.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "pt_light_update.h"
#include "pt_mesh_update.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

namespace {

// The light tables of an emissive mesh after new vertices (the verdict is in, the host mirror is true, nothing is in flight):
// the device forms rewrite them with the kernel from the arrays where they are, the host forms upload them.
int write_light_mesh_device(srt_pt* pt, hipStream_t s, uint32_t object, bool device_form, const float* d_pos, const float* d_nrm) {
  const int32_t li = light_of(pt->built, object);
  if (li < 0) return SRT_OK;
  if (!device_form) return upload_light(pt, (uint32_t)li, true);
  const FlatScene& F = pt->built.flat;
  const Light& L = F.lights[(size_t)li];
  launch_light_triangles(s, d_pos, d_nrm, pt->mesh.d_idx + pt->mesh.idx_off[object], L.ntri, pt->d_lights + li, pt->d_tris + L.tri_base, pt->d_nrm + L.tri_base,
                         pt->d_tri_packed + 9 * (size_t)L.tri_base, pt->d_ltris + (L.tri_base - F.light_tri_first));
  SRT_HIP(hipStreamSynchronize(s));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
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
    if ((st = pt->mesh.d_vpos.ensure(vfloats)) || (st = pt->mesh.d_vnrm.ensure(vfloats))) return st;
    SRT_HIP(hipMemcpy(pt->mesh.d_vpos, V->h_pos, vfloats * sizeof(float), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->mesh.d_vnrm, V->h_nrm, vfloats * sizeof(float), hipMemcpyHostToDevice));
    *staged_bytes = 2 * vfloats * sizeof(float);
    V->d_pos = pt->mesh.d_vpos; V->d_nrm = pt->mesh.d_vnrm;
  } else {
    V->back_pos.resize(vfloats); V->back_nrm.resize(vfloats);
    SRT_HIP(hipMemcpyAsync(V->back_pos.data(), V->d_pos, vfloats * sizeof(float), hipMemcpyDeviceToHost, s));
    SRT_HIP(hipMemcpyAsync(V->back_nrm.data(), V->d_nrm, vfloats * sizeof(float), hipMemcpyDeviceToHost, s));
    V->h_pos = V->back_pos.data(); V->h_nrm = V->back_nrm.data();
  }
  return SRT_OK;
}

}  // namespace

namespace srt {

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
  const uint32_t* d_mesh_idx = on_device ? pt->mesh.d_idx + pt->mesh.idx_off[object] : nullptr;
  HostBVH device_tree;
  const bool device_wanted = device_builder && use_bvh && ntri >= pt->bvh_device_min && ntri > 4u;
  bool device_built = false;
  if (device_wanted && bvh_workspace_reserve(&pt->mesh.bvh_ws, ntri, false)) {
    launch_mesh_boxes(s, V.d_pos, d_mesh_idx, ntri, pt->mesh.bvh_ws.d_boxes);
    device_built = build_bvh_device_core(&pt->mesh.bvh_ws, s, pt->mesh.bvh_ws.d_boxes, ntri, 4, &device_tree);
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
    if (!bvh_workspace_reserve(&pt->mesh.bvh_ws, ntri, true)) return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
    SRT_HIP(hipMemcpy(pt->mesh.bvh_ws.d_prim, U.blas.prim.data(), (size_t)ntri * 4, hipMemcpyHostToDevice));
    pt->bytes_uploaded += (uint64_t)ntri * 4;
  }
  // the verdict is in: from here on the new arrays replace the old ones, on the host and then on the device
  const size_t old_tlas = pt->built.flat.tlas_nodes, old_nodes = pt->built.flat.nodes.size(), old_recs = pt->built.flat.blas_recs.size();
  apply_mesh_update(&pt->built, &U);
  if (on_device) drop_update_tables(pt, object);          // they describe the tree and the boxes that were just replaced
  if (use_bvh) pt->blas_builds++;
  pt->drop_cast_shapes();
  if (!on_device) return SRT_OK;
  pt->bytes_uploaded += pt->mesh.idx_uncounted;
  pt->mesh.idx_uncounted = 0;
  // the record kernel over the mesh's triangle range, the nodes and records that are new or moved, the tables of object order
  auto write = [&]() -> int {
    const FlatScene& F = pt->built.flat;
    const MeshStore now = pt->built.store[object];
    launch_mesh_records(s, V.d_pos, V.d_nrm, d_mesh_idx, use_bvh ? pt->mesh.bvh_ws.d_prim : nullptr, ntri, pt->d_tris + now.tri_base, pt->d_nrm + now.tri_base,
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

// The refit tables of mesh `object`, made from its host tree at its first refit after a commit or a rebuild (blocking).
static int mesh_refit_tables(srt_pt* pt, uint32_t object, RefitTables** T) {
  auto it = pt->mesh.refit_tables.find(object);
  if (it == pt->mesh.refit_tables.end()) {
    RefitTables fresh;
    const int st = make_refit_tables(pt->built.blas[object], "srt_pt_refit_mesh", object, &fresh);
    if (st != SRT_OK) return st;
    it = pt->mesh.refit_tables.emplace(object, std::move(fresh)).first;
  }
  *T = &it->second;
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
    if ((st = mesh_refit_tables(pt, object, &T)) != SRT_OK) { (void)hipStreamSynchronize(s); return st; }   // (the read-back is on s)
    // the new boxes, aside: triangle boxes, leaves, levels.  They come back (24 B per node) with the arrays of the device form
    // (24 B per vertex): the host checks those, takes the root box and keeps its own tree true.
    launch_mesh_boxes(s, V.d_pos, pt->mesh.d_idx + pt->mesh.idx_off[object], m.ntri, T->d_tri_boxes);
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
  pt->mesh.refits++;
  pt->drop_cast_shapes();
  if (!on_device) return SRT_OK;
  pt->pose.drop();                                        // the object-space boxes changed
  pt->top.drop_tables();                                  // the BVH<Object> was rebuilt
  pt->bytes_uploaded += staged_bytes + T->uncounted_bytes + pt->mesh.idx_uncounted;   // the vertices of the host form; the tables, at the mesh's first successful refit
  T->uncounted_bytes = 0;
  pt->mesh.idx_uncounted = 0;
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_level(pt, s, old_tlas))) return w;
    launch_refit_write(s, *T, T->d_node_boxes, pt->d_nodes + pt->built.flat.tlas_nodes + m.node_off, pt->d_blas + m.rec_base);
    launch_mesh_records(s, V.d_pos, V.d_nrm, pt->mesh.d_idx + pt->mesh.idx_off[object], T->d_prim, m.ntri, pt->d_tris + m.tri_base, pt->d_nrm + m.tri_base,
                        pt->d_tri_packed + 9 * (size_t)m.tri_base);
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    if ((w = upload_object_tables(pt))) return w;
    return write_light_mesh_device(pt, s, object, device_form, V.d_pos, V.d_nrm);
  };
  return written(pt, write());
}


// srt_pt_refit_mesh_inplace: the host form.  Blocks; the definition is prepare_mesh_refit_inplace / apply_mesh_refit_inplace.
int refit_mesh_inplace(srt_pt* pt, const char* what, uint32_t object, const float* pos, const float* nrm, uint32_t nverts) {
  int st;
  if ((st = check_mesh_call(pt, what, object, nverts, pos))) return st;
  MeshVertices V{pos, nrm, nullptr, nullptr, {}, {}};
  if (!pt->built.flat.use_bvh) return update_mesh(pt, what, pt->stream, object, V, nverts);   // a list has no trees: the update
  const bool on_device = pt->device >= 0;
  hipStream_t s = pt->stream;
  const MeshStore m = pt->built.store[object];
  std::vector<float> node_boxes;
  RefitTables* T = nullptr;
  uint64_t staged_bytes = 0;                              // (counted with the verdict: a refused refit adds nothing to the figures)
  if (on_device) {
    if ((st = stage_vertices(pt, what, s, object, nverts, true, &V, &staged_bytes))) return st;
    if ((st = mesh_refit_tables(pt, object, &T)) != SRT_OK) return st;
    // the new boxes, aside, and back (24 B per node): the host takes the root box and keeps its own tree true
    launch_mesh_boxes(s, V.d_pos, pt->mesh.d_idx + pt->mesh.idx_off[object], m.ntri, T->d_tri_boxes);
    launch_refit_boxes(s, *T, T->d_tri_boxes, T->d_node_boxes);
    node_boxes.resize(6 * (size_t)T->nnodes);
    SRT_HIP(hipMemcpyAsync(node_boxes.data(), T->d_node_boxes, node_boxes.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
  }
  MeshRefit R;
  const std::string err = prepare_mesh_refit_inplace(pt->built, object, V.h_pos, V.h_nrm, nverts, on_device ? node_boxes.data() : nullptr, true, &R);
  if (!err.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, err.c_str());
  // nothing fails on the host side from here on: boxes and records change in place, and both trees keep their shape
  apply_mesh_refit_inplace(&pt->built, &R);
  pt->mesh.refits++;
  if (!on_device) return SRT_OK;
  pt->pose.drop();                                        // the object-space boxes changed (the trees' tables stay: the trees did)
  pt->bytes_uploaded += staged_bytes + T->uncounted_bytes + pt->mesh.idx_uncounted;
  T->uncounted_bytes = 0;
  pt->mesh.idx_uncounted = 0;
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_refit(pt, nullptr, 0))) return w;  // the top-level nodes and the sweep records, no object record
    launch_refit_write(s, *T, T->d_node_boxes, pt->d_nodes + pt->built.flat.tlas_nodes + m.node_off, pt->d_blas + m.rec_base);
    launch_mesh_records(s, V.d_pos, V.d_nrm, pt->mesh.d_idx + pt->mesh.idx_off[object], T->d_prim, m.ntri, pt->d_tris + m.tri_base, pt->d_nrm + m.tri_base,
                        pt->d_tri_packed + 9 * (size_t)m.tri_base);
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    return write_light_mesh_device(pt, s, object, false, V.d_pos, V.d_nrm);
  };
  return written(pt, write());
}

// What srt_pt_refit_mesh_inplace_device keeps per mesh beside its refit tables, made at the mesh's first such call after a commit or a
// rebuild (blocking; 4 B per member of the family go up): the vertex buffers, the family, and an emissive mesh's index buffer.
static int ensure_inplace(srt_pt* pt, const char* what, uint32_t object, uint32_t nverts, srt_pt::MeshState::Inplace** out) {
  auto it = pt->mesh.inplace.find(object);
  if (it != pt->mesh.inplace.end()) { *out = &it->second; return SRT_OK; }
  int st;
  if (pt->mesh.idx_off[object] == SIZE_MAX) {             // an emissive mesh under srt_pt_set_dynamic_lights: its index buffer goes up now
    SRT_HIP(quiesce(pt));
    if ((st = ensure_mesh_idx(pt, object))) return st;
  }
  std::vector<uint32_t> family(1, object);
  for (uint32_t i = 0; i < (uint32_t)pt->built.inputs.size(); i++)
    if (pt->built.inputs[i].kind == OBJ_MESH && pt->built.inputs[i].source == (int32_t)object) family.push_back(i);
  srt_pt::MeshState::Inplace fresh;
  const size_t vfloats = 3 * (size_t)(nverts ? nverts : 1);
  if (fresh.d_pos.ensure(vfloats) || fresh.d_nrm.ensure(vfloats) || fresh.d_family.upload(family)) {
    (void)hipGetLastError();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  fresh.nfamily = (uint32_t)family.size();
  pt->bytes_uploaded += family.size() * sizeof(uint32_t);
  *out = &pt->mesh.inplace.emplace(object, std::move(fresh)).first->second;
  return SRT_OK;
}

// srt_pt_refit_mesh_inplace_device / srt_pt_skin_pose_inplace[_at].
int refit_mesh_inplace_device(srt_pt* pt, const char* what, hipStream_t s, uint32_t object, const float* d_pos, const float* d_nrm, uint32_t nverts) {
  if (!pt->committed) return not_committed(what);         // (no settle(): this call only adds to what is pending)
  const std::string refused = check_mesh_update(pt->built, object, nverts);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the refit is enqueued on the device only; this context is host-only (srt_pt_refit_mesh_inplace takes host arrays)", what);
  if (!pt->built.flat.use_bvh) return refit_mesh(pt, what, s, object, {nullptr, nullptr, d_pos, d_nrm, {}, {}}, nverts);   // a list has no trees: the update, which blocks
  SRT_HIP(hipSetDevice(pt->device));
  // First call after a commit or after a call that replaced one of the trees (blocking, counted once): the pose tables and the
  // BVH<Object>'s refit tables, the mesh's refit tables, its family and its vertex buffers.  Nothing is pending then.
  int st;
  RefitTables* T = nullptr;
  srt_pt::MeshState::Inplace* I = nullptr;
  if ((st = ensure_top_tables(pt, s, what)) || (st = mesh_refit_tables(pt, object, &T)) || (st = ensure_inplace(pt, what, object, nverts, &I))) return st;
  pt->bytes_uploaded += T->uncounted_bytes + pt->mesh.idx_uncounted;
  T->uncounted_bytes = 0;
  pt->mesh.idx_uncounted = 0;
  // Everything below only enqueues on `s`: the vertices into the context's own buffers, the triangle boxes, the leaves and levels
  // of the mesh's tree, its live nodes and records, its triangle records in the kept order, an emissive mesh's light tables, the
  // link - the family's object-space and posed boxes - and the BVH<Object>'s own refit.  No verdict is needed: depth, counts,
  // orders, kernel form and stack sizes are those of the committed trees.
  const FlatScene& F = pt->built.flat;
  const MeshStore m = pt->built.store[object];
  const uint32_t* d_idx = pt->mesh.d_idx + pt->mesh.idx_off[object];
  const size_t vbytes = 3 * (size_t)nverts * sizeof(float);
  hipError_t he;
  if (vbytes && ((he = hipMemcpyAsync(I->d_pos, d_pos, vbytes, hipMemcpyDeviceToDevice, s)) != hipSuccess ||
                 (he = hipMemcpyAsync(I->d_nrm, d_nrm, vbytes, hipMemcpyDeviceToDevice, s)) != hipSuccess))
    return top_hip_broken(pt, what, he, "the copy of the vertices");
  launch_mesh_boxes(s, I->d_pos, d_idx, m.ntri, T->d_tri_boxes);
  launch_refit_boxes(s, *T, T->d_tri_boxes, T->d_node_boxes);
  launch_refit_write(s, *T, T->d_node_boxes, pt->d_nodes + F.tlas_nodes + m.node_off, pt->d_blas + m.rec_base);
  launch_mesh_records(s, I->d_pos, I->d_nrm, d_idx, T->d_prim, m.ntri, pt->d_tris + m.tri_base, pt->d_nrm + m.tri_base, pt->d_tri_packed + 9 * (size_t)m.tri_base);
  const int32_t li = light_of(pt->built, object);
  if (li >= 0) {
    const Light& L = F.lights[(size_t)li];
    launch_light_triangles(s, I->d_pos, I->d_nrm, d_idx, L.ntri, pt->d_lights + li, pt->d_tris + L.tri_base, pt->d_nrm + L.tri_base,
                           pt->d_tri_packed + 9 * (size_t)L.tri_base, pt->d_ltris + (L.tri_base - F.light_tri_first));
  }
  launch_mesh_link(s, I->d_family, I->nfamily, (uint32_t)pt->built.inputs.size(), T->d_node_boxes, pt->pose.d_records, pt->pose.d_local_boxes,
                   pt->pose.d_posed_boxes);
  enqueue_top_boxes(pt, s);
  if ((st = record_top_pending(pt, s, what))) return st;
  pt->mesh.pending++;
  if (std::find(pt->mesh.pending_meshes.begin(), pt->mesh.pending_meshes.end(), object) == pt->mesh.pending_meshes.end()) pt->mesh.pending_meshes.push_back(object);
  return SRT_OK;
}

// The host's record catches up with the device after srt_pt_refit_mesh_inplace_device calls (the head of settle_top): one wait for the
// event behind the last pending call and, per mesh they touched - however many calls - one read-back of its vertices (24 B each, from the context's buffers) and
// node boxes (24 B per node), applied through the definition without the finiteness check and with the boxes as read.  The BVH<Object>'s
// boxes the definition writes here are the host's own fold; settle_top then reads the device's back over them.
int settle_mesh(srt_pt* pt) {
  if (!pt->mesh.pending) return SRT_OK;
  const uint64_t calls = pt->mesh.pending;
  const std::vector<uint32_t> meshes = pt->mesh.pending_meshes;
  pt->mesh.forget_pending();
  auto broken = [&](const char* why) {
    return top_broken(pt, srt::fail(SRT_ERR_HIP, "settling srt_pt_refit_mesh_inplace_device: %s; the scene has to be committed again", why));
  };
  if (hipSetDevice(pt->device) != hipSuccess || hipEventSynchronize(pt->top.event) != hipSuccess) return broken(hipGetErrorString(hipGetLastError()));
  for (uint32_t object : meshes) {
    auto I = pt->mesh.inplace.find(object);
    auto T = pt->mesh.refit_tables.find(object);
    if (I == pt->mesh.inplace.end() || T == pt->mesh.refit_tables.end()) return broken("the mesh's device tables are gone");
    const size_t vfloats = pt->built.inputs[object].mesh.pos.size();
    std::vector<float> pos(vfloats), nrm(vfloats), boxes(6 * (size_t)T->second.nnodes);
    if ((vfloats && (hipMemcpy(pos.data(), I->second.d_pos, vfloats * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                     hipMemcpy(nrm.data(), I->second.d_nrm, vfloats * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) ||
        (!boxes.empty() && hipMemcpy(boxes.data(), T->second.d_node_boxes, boxes.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess))
      return broken(hipGetErrorString(hipGetLastError()));
    MeshRefit R;
    const std::string err = prepare_mesh_refit_inplace(pt->built, object, pos.data(), nrm.data(), (uint32_t)(vfloats / 3), boxes.data(), false, &R);
    if (!err.empty()) return broken(err.c_str());
    apply_mesh_refit_inplace(&pt->built, &R);
  }
  pt->mesh.refits += calls;
  return SRT_OK;
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

int srt_pt_refit_mesh_inplace(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts) {
  if (!pt || !positions || !normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_mesh_inplace: NULL argument");
  return refit_mesh_inplace(pt, "srt_pt_refit_mesh_inplace", object, positions, normals, nverts);
}

int srt_pt_refit_mesh_inplace_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts) {
  if (!pt || !d_positions || !d_normals) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_mesh_inplace_device: NULL argument");
  return refit_mesh_inplace_device(pt, "srt_pt_refit_mesh_inplace_device", (hipStream_t)stream, object, d_positions, d_normals, nverts);
}

int srt_pt_mesh_refit_pending(srt_pt* pt, uint64_t out[2]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_mesh_refit_pending: NULL argument");
  out[0] = pt->mesh.pending;
  out[1] = pt->mesh.pending_meshes.size();
  return SRT_OK;
}

int srt_pt_mesh_tree_cost(srt_pt* pt, uint32_t object, double* cost) {
  if (!pt || !cost) return srt::fail(SRT_ERR_INVALID, "srt_pt_mesh_tree_cost: NULL argument");
  { const int ready = need_committed(pt, "srt_pt_mesh_tree_cost"); if (ready != SRT_OK) return ready; }   // (settles: the cost is the tree's as refitted)
  const std::string refused = check_mesh_update(pt->built, object, (uint32_t)(object < pt->built.inputs.size() ? pt->built.inputs[object].mesh.pos.size() / 3 : 0));
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "srt_pt_mesh_tree_cost: %s", refused.c_str());
  if (!pt->built.flat.use_bvh) return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_mesh_tree_cost: the scene was committed without BVHs, the mesh has no tree");
  *cost = tree_cost(pt->built.blas[object]);
  return SRT_OK;
}

int srt_pt_refit_count(srt_pt* pt, uint64_t* refits) {
  if (!pt || !refits) return srt::fail(SRT_ERR_INVALID, "srt_pt_refit_count: NULL argument");
  { const int settled = settle(pt); if (settled != SRT_OK) return settled; }
  *refits = pt->mesh.refits;
  return SRT_OK;
}

}  // extern "C"
