// New poses for a committed scene: srt_pt_repose[_device] rebuild the BVH<Object>, srt_pt_repose_refit[_device] refit it in place - the
// device form only enqueues, and settle_top brings the host's record up to date later - and srt_pt_timeline_* evaluates Animate-mode
// keys into either; with them the figures about the tree and its refits and the particles' transforms.  Host code only: the kernels are
// in pt_pose.hip, pt_anim.hip, pt_light_update.hip, pt_mesh_update.hip and pt_bvh_device.hip, the key arithmetic in pt_anim.h.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_anim.h"
#include "pt_light_update.h"
#include "pt_mesh_update.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

// ---- srt_pt_timeline: Anim_Pose::at(t) and Pose::transform() of listed objects (pt_anim.h, pt_anim.hip) ----
struct srt_pt_timeline : SceneHandle {
  std::vector<uint32_t> objects, track_offsets;           // insertion indices; 3 tracks per object, CSR
  std::vector<float> knot_times, knot_values;
  DeviceBuffer<uint32_t> d_track_offsets;
  DeviceBuffer<float> d_knot_times, d_knot_values, d_trans;   // d_trans: the frame's transforms, 16 floats per object
};

namespace {

int timeline_usable(const srt_pt_timeline* tl, const char* what) {
  if (!tl) return srt::fail(SRT_ERR_INVALID, "%s: NULL timeline", what);
  if (tl->stale()) return srt::fail(SRT_ERR_STATE, "%s: the timeline is stale - its context's scene was begun or committed again after srt_pt_timeline_create", what);
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

std::vector<Mat4> matrices(const float* trans, uint32_t n) {
  static_assert(sizeof(Mat4) == 16 * sizeof(float), "Mat4 is sixteen floats");
  std::vector<Mat4> T(n);
  if (n) std::memcpy(T.data(), trans, (size_t)n * sizeof(Mat4));
  return T;
}

// The tables the pose kernels work in, made at the first device-form repose after a commit or after a call that dropped them: the
// records by insertion index come from the live records (a kernel on `s`; nothing goes up), the posed boxes from them and the
// object-space boxes (24 B per object up, added to *bytes).
int ensure_pose_tables(srt_pt* pt, hipStream_t s, const char* what, uint64_t* bytes) {
  if (pt->pose.valid) return SRT_OK;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  const size_t room = nobj ? nobj : 1;
  pt->pose.drop();
  if (pt->pose.d_records.ensure(room) || pt->pose.d_local_boxes.ensure(room * 6) || pt->pose.d_posed_boxes.ensure(room * 6) || pt->pose.d_active.ensure(room)) {
    (void)hipGetLastError();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  // (blocking copy, then kernels on `s` that read what the last commit or repose left in d_objects: all of it done by now)
  if (nobj) SRT_HIP(hipMemcpy(pt->pose.d_local_boxes, pt->built.local_boxes.data(), (size_t)nobj * 6 * sizeof(float), hipMemcpyHostToDevice));
  *bytes += (uint64_t)nobj * 6 * sizeof(float);
  // srt_pt_set_active's table: the host's (1 B per object up) while an object is inactive, otherwise a fill on the device
  if (nobj && any_inactive(pt->built)) {
    SRT_HIP(hipMemcpy(pt->pose.d_active, pt->built.active.data(), nobj, hipMemcpyHostToDevice));
    *bytes += nobj;
  } else if (nobj) {
    SRT_HIP(hipMemsetAsync(pt->pose.d_active, 1, nobj, s));
  }
  launch_pose_tables(s, pt->d_objects, nobj, pt->built.flat.tlas_nodes, pt->pose.d_records, pt->pose.d_local_boxes, pt->pose.d_posed_boxes);
  pt->pose.valid = true;
  return SRT_OK;
}

// A pinned staging buffer of at least `words` words whose last copy has left it (or a new one).
int pinned_list(srt_pt* pt, size_t words, srt_pt::TopLevel::PinnedList** out) {
  for (auto& pl : pt->top.pinned) {
    if (pl.h.capacity() < words) continue;
    const hipError_t left = hipEventQuery(pl.done);
    (void)hipGetLastError();                              // (hipErrorNotReady of a query is no error: not left behind for the launch check)
    if (left == hipSuccess) { *out = &pl; return SRT_OK; }
  }
  srt_pt::TopLevel::PinnedList pl;
  if (pl.h.ensure(std::max<size_t>(words, 1024))) return srt::fail(SRT_ERR_HIP, "out of pinned host memory");
  if (pl.done.create(hipEventDisableTiming)) return srt::fail(SRT_ERR_HIP, "event creation failed");
  pt->top.pinned.push_back(std::move(pl));
  *out = &pt->top.pinned.back();
  return SRT_OK;
}

}  // namespace

namespace srt {

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

// What the device forms of srt_pt_repose_refit and srt_pt_set_active share.
// A HIP failure after the first enqueue may leave tables, lists or live arrays half written: the scene is no longer committed, what was
// pending is forgotten (settle() has no record to bring up to date) and the tables go; the scene has to be committed again.
int top_broken(srt_pt* pt, int status) {
  pt->committed = false;
  if (hipSetDevice(pt->device) == hipSuccess) (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  pt->top.forget_pending();
  pt->mesh.forget_pending();
  pt->pose.drop();
  pt->top.drop_tables();
  return status;
}
int top_hip_broken(srt_pt* pt, const char* what, hipError_t e, const char* step) {
  return top_broken(pt, srt::fail(SRT_ERR_HIP, "%s: %s failed (%s); the scene has to be committed again", what, step, hipGetErrorString(e)));
}

// First call after a commit or after a call that replaced the BVH<Object> (blocking, counted once): the pose tables as
// srt_pt_repose_device makes them (24 B per object up), the tree's refit tables (about 28 B per object up) and the slot of
// every object (a kernel).  Nothing is pending then - every call that drops these tables settles first.
int ensure_top_tables(srt_pt* pt, hipStream_t s, const char* what) {
  int st;
  if ((st = ensure_pose_tables(pt, s, what, &pt->bytes_uploaded))) return st;
  if (!pt->built.flat.use_bvh || pt->top.have_tables) return SRT_OK;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  pt->top.drop_tables();
  RefitTables fresh;
  if ((st = make_refit_tables(pt->built.tlas, what, UINT32_MAX, &fresh)) != SRT_OK) return st;
  pt->top.tables = std::move(fresh);
  pt->top.have_tables = true;
  pt->bytes_uploaded += pt->top.tables.uncounted_bytes;
  pt->top.tables.uncounted_bytes = 0;
  if (pt->top.d_slot_of.ensure(nobj ? nobj : 1)) {
    (void)hipGetLastError();
    pt->top.drop_tables();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  launch_top_slots(s, pt->top.tables.d_prim, nobj, pt->top.d_slot_of);
  return SRT_OK;
}

// The list (4 B per listed object, 8 B more per listed light) into pose.d_list, through pinned memory so that the copy is only
// enqueued - unless the device holds this very list already.
static int stage_top_list(srt_pt* pt, hipStream_t s, const char* what, const uint32_t* objects, uint32_t n) {
  if (!n || (pt->top.list_valid && pt->top.list.size() == n && std::memcmp(pt->top.list.data(), objects, (size_t)n * 4) == 0)) return SRT_OK;
  int st;
  hipError_t he;
  const ListedLights lights = listed_lights(pt->built, objects, n);
  pt->top.forget_list();
  // (growing one of these arrays frees the old one, which waits for what reads it: first calls and longer lists only)
  if ((st = pt->pose.d_list.ensure(n)) || (st = pt->pose.d_out.ensure(n)) || (!lights.pairs.empty() && (st = pt->pose.d_light_list.ensure(lights.pairs.size()))))
    return top_broken(pt, st);
  srt_pt::TopLevel::PinnedList* pl = nullptr;
  if ((st = pinned_list(pt, (size_t)n + lights.pairs.size(), &pl)) != SRT_OK) return top_broken(pt, st);
  uint32_t* const h = pl->h;
  std::memcpy(h, objects, (size_t)n * 4);
  if (!lights.pairs.empty()) std::memcpy(h + n, lights.pairs.data(), lights.pairs.size() * 4);
  if ((he = hipMemcpyAsync(pt->pose.d_list, h, (size_t)n * 4, hipMemcpyHostToDevice, s)) != hipSuccess) return top_hip_broken(pt, what, he, "the copy of the list");
  if (!lights.pairs.empty() && (he = hipMemcpyAsync(pt->pose.d_light_list, h + n, lights.pairs.size() * 4, hipMemcpyHostToDevice, s)) != hipSuccess)
    return top_hip_broken(pt, what, he, "the copy of the light list");
  if ((he = hipEventRecord(pl->done, s)) != hipSuccess) return top_hip_broken(pt, what, he, "hipEventRecord");
  pt->bytes_uploaded += (uint64_t)n * 4 + lights.pairs.size() * 4;
  pt->top.list.assign(objects, objects + n);
  pt->top.lights = (uint32_t)(lights.pairs.size() / 2);
  pt->top.light_max_ntri = lights.max_ntri;
  pt->top.list_valid = true;
  return SRT_OK;
}

// The leaves from the effective boxes (the posed boxes, BBox() for what the active table switches off), the levels, the live boxes.
void enqueue_top_boxes(srt_pt* pt, hipStream_t s) {
  launch_refit_boxes(s, pt->top.tables, pt->pose.d_posed_boxes, pt->top.tables.d_node_boxes, pt->pose.d_active);   // the tree's primitives are the objects: their boxes are the pose tables'
  launch_refit_write(s, pt->top.tables, pt->top.tables.d_node_boxes, pt->d_nodes, pt->d_wave);
}

// The launches went in, the event behind them is recorded, and the host's record is behind by one more call until settle().
int record_top_pending(srt_pt* pt, hipStream_t s, const char* what) {
  hipError_t he;
  if ((he = hipGetLastError()) != hipSuccess) return top_hip_broken(pt, what, he, "a launch");
  if (pt->top.event.create(hipEventDisableTiming)) return top_hip_broken(pt, what, hipGetLastError(), "hipEventCreate");
  if ((he = hipEventRecord(pt->top.event, s)) != hipSuccess) return top_hip_broken(pt, what, he, "hipEventRecord");
  pt->top.pending++;
  if (pt->top.pending_flag.size() != pt->built.inputs.size()) pt->top.pending_flag.assign(pt->built.inputs.size(), 0);   // (nothing is pending across a commit)
  return SRT_OK;
}

// srt_pt_set_active[_device]: the scene layer's verdict on the list, as a status.
static int active_list_usable(srt_pt* pt, const char* what, const uint32_t* objects, uint32_t n) {
  bool unsupported = false;
  const std::string refused = check_active_list(pt->built, objects, n, &unsupported);
  return refused.empty() ? SRT_OK : srt::fail(unsupported ? SRT_ERR_UNSUPPORTED : SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
}

// The host's record catches up with the device after srt_pt_repose_refit_device calls: one wait for the event behind the last of
// them, one read-back (176 B per object: the records by insertion index; 24 B per node: the top-level boxes), and the scene
// layer's own apply_top_refit - the lights' records come from the host's light_record / light_area_term.  With nothing pending it
// does nothing.
int settle_top(srt_pt* pt) {
  if (!pt->top.pending) return SRT_OK;
  if (!pt->committed) { discard_pending(pt); return SRT_OK; }   // (a failure took the scene away: there is no record to bring up to date)
  const uint64_t calls = pt->top.pending, flag_calls = pt->top.pending_active, mesh_calls = pt->mesh.pending;
  { const int st = settle_mesh(pt); if (st != SRT_OK) return st; }   // the mesh half first: the boxes read back below lie over what it folds
  std::vector<uint32_t> objects = pt->top.pending_objects;
  pt->top.forget_pending();
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  const bool use_bvh = pt->built.flat.use_bvh;
  std::vector<Object> records(nobj);
  std::vector<uint8_t> active(flag_calls ? nobj : 0);     // (srt_pt_set_active_device: 1 B per object, only behind such a call)
  TopRefit R;
  if (use_bvh) R.boxes.resize(6 * (size_t)pt->top.tables.nnodes);
  if (hipSetDevice(pt->device) != hipSuccess || hipEventSynchronize(pt->top.event) != hipSuccess ||
      (nobj && hipMemcpy(records.data(), pt->pose.d_records, (size_t)nobj * sizeof(Object), hipMemcpyDeviceToHost) != hipSuccess) ||
      (!active.empty() && hipMemcpy(active.data(), pt->pose.d_active, active.size(), hipMemcpyDeviceToHost) != hipSuccess) ||
      (!R.boxes.empty() && hipMemcpy(R.boxes.data(), pt->top.tables.d_node_boxes, R.boxes.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
    pt->committed = false;
    return srt::fail(SRT_ERR_HIP, "settling srt_pt_repose_refit_device: %s; the scene has to be committed again", hipGetErrorString(hipGetLastError()));
  }
  if (!active.empty()) pt->built.active.swap(active);     // (the boxes read back are the masked fold's already)
  for (uint32_t i : objects) {                            // (every object once: top.pending_flag)
    R.listed.push_back(i);
    R.trans.push_back(records[i].trans);
    R.itrans.push_back(records[i].itrans);
    R.has_trans.push_back(records[i].has_trans);
  }
  apply_top_refit(&pt->built, &R);
  if (flag_calls) write_top_counts(&pt->built);           // (what launch_top_counts left in the live nodes and sweep records)
  pt->top.refits += calls - flag_calls - mesh_calls;
  return SRT_OK;
}

}  // namespace srt

extern "C" {

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
  pt->drop_cast_shapes();
  if (!on_device) return SRT_OK;
  pt->pose.drop();                                        // srt_pt_repose_device's tables mirror the poses that were just replaced
  pt->top.drop_tables();                                  // srt_pt_repose_refit_device's describe the tree that was just replaced
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
  pt->top.forget_list();                                  // pose.d_list and pose.d_light_list are about to hold this call's lists
  hipStream_t s = (hipStream_t)stream;
  const bool use_bvh = pt->built.flat.use_bvh;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  uint64_t staged_bytes = 0;                              // (counted with the verdict: a refused repose adds nothing to the figures)
  if ((st = ensure_pose_tables(pt, s, what, &staged_bytes))) return st;
  // From here to the verdict only these tables and the staging are written; a refusal drops the tables (the next call makes them
  // again from the committed records, which are not touched).
  auto refuse = [&](int status) { pt->pose.drop(); return status; };
  auto copy_failed = [&] { return refuse(srt::fail(SRT_ERR_HIP, "%s: copy failed", what)); };
  std::vector<PoseOut> posed(n);
  std::vector<float> boxes;
  if (n) {
    if ((st = pt->pose.d_list.ensure(n)) || (st = pt->pose.d_out.ensure(n))) return refuse(st);
    if (hipMemcpyAsync(pt->pose.d_list, objects, (size_t)n * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
    staged_bytes += (uint64_t)n * 4;
    launch_pose_objects(s, pt->pose.d_list, d_trans, n, nobj, pt->pose.d_local_boxes, pt->pose.d_out, pt->pose.d_records, pt->pose.d_posed_boxes);
    if (hipMemcpyAsync(posed.data(), pt->pose.d_out, (size_t)n * sizeof(PoseOut), hipMemcpyDeviceToHost, s) != hipSuccess) return copy_failed();
  }
  if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return refuse(srt::fail(SRT_ERR_HIP, "%s: the pose kernel failed", what));
  // The BVH<Object> build goes where srt_pt_repose's does: on the device, over the boxes where they are, for a scene at or above
  // the device builder's threshold; anything else - and a device build that failed: the host build gives the verdict - on the host,
  // over the boxes read back (24 B per object).
  HostBVH device_tree;
  bool device_built = false;
  if (use_bvh && device_builds(pt) && nobj >= pt->bvh_device_min && nobj > 1u && bvh_workspace_reserve(&pt->mesh.bvh_ws, nobj, false)) {
    device_built = build_bvh_device_core(&pt->mesh.bvh_ws, s, pt->pose.d_posed_boxes, nobj, 1, &device_tree);   // over the posed boxes where they are
  }
  if (use_bvh && !device_built) {
    boxes.resize((size_t)nobj * 6);
    if (hipMemcpyAsync(boxes.data(), pt->pose.d_posed_boxes, boxes.size() * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
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
      if (!bvh_workspace_reserve(&pt->mesh.bvh_ws, nobj, true)) return refuse(srt::fail(SRT_ERR_HIP, "%s: out of device memory", what));
      if (hipMemcpyAsync(pt->mesh.bvh_ws.d_prim, top.tlas.prim.data(), (size_t)nobj * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
      staged_bytes += (uint64_t)nobj * 4;
    }
    d_prim = pt->mesh.bvh_ws.d_prim;
    if (!top.lazy_objects.empty()) {
      ordinal.assign(nobj, 0u);
      for (size_t q = 0; q < top.lazy_objects.size(); q++) ordinal[top.lazy_objects[q]] = (uint32_t)q << 8;
      if ((st = pt->pose.d_slot_ordinal.ensure(nobj))) return refuse(st);
      if (hipMemcpyAsync(pt->pose.d_slot_ordinal, ordinal.data(), (size_t)nobj * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
      staged_bytes += (uint64_t)nobj * 4;
      d_ordinal = pt->pose.d_slot_ordinal;
    }
  }
  // the listed area lights (srt_pt_set_dynamic_lights), still aside
  const ListedLights lights = listed_lights(pt->built, objects, n);
  if (!lights.pairs.empty()) {
    if ((st = pt->pose.d_light_list.ensure(lights.pairs.size()))) return refuse(st);
    if (hipMemcpyAsync(pt->pose.d_light_list, lights.pairs.data(), lights.pairs.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess) return copy_failed();
    staged_bytes += (uint64_t)lights.pairs.size() * 4;
  }
  // the verdict is in; nothing of the context may be in flight while the live arrays change
  const size_t old_tlas_nodes = pt->built.flat.tlas_nodes;
  if (hipStreamSynchronize(s) != hipSuccess || quiesce(pt) != hipSuccess) return refuse(srt::fail(SRT_ERR_HIP, "%s: synchronisation failed", what));
  apply_repose(&pt->built, &top);
  pt->top.drop_tables();                                  // srt_pt_repose_refit_device's describe the tree that was just replaced
  pt->drop_cast_shapes();
  pt->bytes_uploaded += staged_bytes;
  auto write = [&]() -> int {
    int w;
    if ((w = write_top_level(pt, s, old_tlas_nodes))) return w;
    // the records in place (the object count never changes): gathered on the device by the new order
    launch_pose_records(s, pt->pose.d_records, d_prim, d_ordinal, nobj, pt->built.flat.tlas_nodes, pt->d_objects);
    if (!lights.pairs.empty()) launch_listed_lights(pt, s, (uint32_t)(lights.pairs.size() / 2), lights.max_ntri, n);
    SRT_HIP(hipStreamSynchronize(s));
    SRT_HIP(hipGetLastError());
    return upload_object_tables(pt, false);
  };
  st = written(pt, write());
  if (st != SRT_OK) pt->pose.drop();
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
  pt->top.refits++;
  if (pt->device < 0) return SRT_OK;
  pt->pose.drop();                                        // they mirror the poses that were just replaced (the tree's tables stay: the tree did)
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
  const bool use_bvh = pt->built.flat.use_bvh;
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  int st;
  if ((st = ensure_top_tables(pt, s, what)) || (st = stage_top_list(pt, s, what, objects, n))) return st;
  // Everything below only enqueues on `s`: the poses, the leaves through the tree's primitive order (an inactive object's as
  // BBox(): srt_pt_set_active), the levels deepest first, the boxes into the live nodes and sweep records, the listed records'
  // matrices, the listed lights.  No verdict is needed: depth, counts, order, kernel form and stack sizes are those of the committed tree.
  if (n) launch_pose_objects(s, pt->pose.d_list, d_trans, n, nobj, pt->pose.d_local_boxes, pt->pose.d_out, pt->pose.d_records, pt->pose.d_posed_boxes);
  if (use_bvh) enqueue_top_boxes(pt, s);
  if (n) {
    launch_top_objects(s, pt->pose.d_list, n, nobj, use_bvh ? pt->top.d_slot_of : nullptr, pt->pose.d_records, pt->d_objects);
    if (pt->top.lights) launch_listed_lights(pt, s, pt->top.lights, pt->top.light_max_ntri, n);
  }
  if ((st = record_top_pending(pt, s, what))) return st;
  // the objects this call listed that no pending call had listed
  for (uint32_t k = 0; k < n; k++)
    if (!pt->top.pending_flag[objects[k]]) { pt->top.pending_flag[objects[k]] = 1; pt->top.pending_objects.push_back(objects[k]); }
  return SRT_OK;
}

int srt_pt_set_active(srt_pt* pt, const uint32_t* objects, const uint8_t* active, uint32_t n) {
  const char* what = "srt_pt_set_active";
  if (!pt || (n && (!objects || !active))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  if ((st = active_list_usable(pt, what, objects, n))) return st;
  bool changes = false;
  for (uint32_t k = 0; k < n && !changes; k++) changes = pt->built.active[objects[k]] != (active[k] ? 1 : 0);
  if (!changes) return SRT_OK;                            // nothing is written and nothing goes up
  // nothing fails on the host side from here on: the table and the boxes change in place
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  apply_set_active(&pt->built, objects, active, n);
  if (pt->device < 0) return SRT_OK;
  pt->pose.drop();                                        // (its copy of the table is behind; the tree's tables stay: the tree did)
  return written(pt, write_top_refit(pt, objects, 0));    // the top-level nodes and the sweep records, no object record
}

int srt_pt_set_active_device(srt_pt* pt, void* stream, const uint32_t* objects, const uint8_t* d_active, uint32_t n) {
  const char* what = "srt_pt_set_active_device";
  if (!pt || (n && (!objects || !d_active))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (!pt->committed) return not_committed(what);         // (no settle(): this call only adds to what is pending)
  int st;
  if ((st = active_list_usable(pt, what, objects, n))) return st;
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the flags are read on the device only; this context is host-only (srt_pt_set_active takes host flags)", what);
  SRT_HIP(hipSetDevice(pt->device));
  hipStream_t s = (hipStream_t)stream;
  if ((st = ensure_top_tables(pt, s, what)) || (st = stage_top_list(pt, s, what, objects, n))) return st;
  // only enqueues on `s`: the listed flags into the table, then the refit's own stages with the table as the leaf stage's mask
  const uint32_t nobj = (uint32_t)pt->built.inputs.size();
  launch_active_scatter(s, pt->pose.d_list, d_active, n, nobj, pt->pose.d_active);
  enqueue_top_boxes(pt, s);
  launch_top_counts(s, pt->top.tables, pt->pose.d_active, nobj, pt->d_nodes, pt->d_wave);   // a hidden leaf holds nothing for the walks
  if ((st = record_top_pending(pt, s, what))) return st;
  pt->top.pending_active++;
  return SRT_OK;
}

int srt_pt_get_active(srt_pt* pt, uint8_t* active_out, uint32_t cap) {
  if (!pt || (cap && !active_out)) return srt::fail(SRT_ERR_INVALID, "srt_pt_get_active: NULL argument");
  const int st = need_committed(pt, "srt_pt_get_active");
  if (st != SRT_OK) return st;
  const size_t nobj = pt->built.active.size();
  if (cap < nobj) return srt::fail(SRT_ERR_INVALID, "srt_pt_get_active: room for %u flags, the scene has %zu objects", cap, nobj);
  if (nobj) std::memcpy(active_out, pt->built.active.data(), nobj);
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
  return handle_publish(tl, timeline, [&]() -> int {
    SRT_HIP(hipSetDevice(pt->device));
    int w;
    if ((w = tl->d_track_offsets.upload(tl->track_offsets)) || (w = tl->d_knot_times.upload(tl->knot_times)) || (w = tl->d_knot_values.upload(tl->knot_values)))
      return w;
    pt->bytes_uploaded += tl->track_offsets.size() * sizeof(uint32_t) + 5 * nk * sizeof(float);
    return tl->d_trans.ensure((nobjects ? (size_t)nobjects : 1) * 16);
  });
}

int srt_pt_timeline_destroy(srt_pt_timeline* timeline) { return handle_destroy(timeline); }

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

int srt_pt_scene_tree_cost(srt_pt* pt, double* cost) {
  if (!pt || !cost) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_tree_cost: NULL argument");
  { const int ready = need_committed(pt, "srt_pt_scene_tree_cost"); if (ready != SRT_OK) return ready; }
  if (!pt->built.flat.use_bvh) return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_scene_tree_cost: the scene was committed without BVHs, it has no tree");
  *cost = tree_cost(pt->built.tlas);
  return SRT_OK;
}

int srt_pt_top_refit_pending(srt_pt* pt, uint64_t out[2]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_top_refit_pending: NULL argument");
  out[0] = pt->top.pending;
  out[1] = pt->top.pending_objects.size();
  return SRT_OK;
}

int srt_pt_top_refit_count(srt_pt* pt, uint64_t* refits) {
  if (!pt || !refits) return srt::fail(SRT_ERR_INVALID, "srt_pt_top_refit_count: NULL argument");
  { const int settled = settle(pt); if (settled != SRT_OK) return settled; }
  *refits = pt->top.refits;
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

}  // extern "C"
