// Skins and rigs on a committed mesh: Skeleton::find_joints once (srt_pt_skin_create), Skeleton::skin per frame from the caller's
// matrices, from the rig's keys (srt_pt_skin_set_rig) or from the current pose that IK handles drive (srt_pt_skin_step_ik), into the
// caller's arrays or - through update_mesh / refit_mesh - into the scene.  Host code only: the kernels are in pt_skin.hip, pt_anim.hip
// and pt_ik.hip, the joint arithmetic both sides share in pt_skin.h, pt_anim.h and pt_ik.h.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_anim.h"
#include "pt_ik.h"
#include "pt_skin.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

// ---- srt_pt_skin: Skeleton::find_joints once, Skeleton::skin per frame (pt_skin.h, pt_skin.hip) ----
struct srt_pt_skin : SceneHandle {
  uint32_t object = 0, nverts = 0, ntri = 0, njoints = 0, ninf = 0;
  std::vector<float> inv;                   // Mat4::inverse(joint_to_bind(j)), 16 floats per joint
  // The frame's posed_j * inverse_j on their way up: pinned, one buffer per frame still on its way (its event tells), so that the copy is
  // only enqueued and an enqueue-only pose never rewrites what an earlier one's copy has yet to read.
  struct Mats { PinnedBuffer<float> h; Event done; };
  std::vector<Mats> mats;
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
  // The current Joint::pose, 3 floats per joint (srt_pt_skin_set_rig: the rest pose), which srt_pt_skin_set_time and srt_pt_skin_step_ik*
  // change and the *_current calls read; the `_at` calls neither read nor write it.  `pose` is the host's mirror: an enqueue-only call
  // leaves it behind (pose_lags) and the next host read settles it.  The IK handles: their joints in do_ik's order and, per joint, the
  // handles whose chain holds it (ik_build_csr), on both sides.
  std::vector<float> pose;
  bool pose_lags = false;
  std::vector<uint32_t> ik_joints, ik_off, ik_list;
  DeviceBuffer<float> d_pose, d_ik_scratch, d_ik_targets;
  DeviceBuffer<uint8_t> d_ik_enabled;
  DeviceBuffer<uint32_t> d_ik_joints, d_ik_off, d_ik_list;
};

namespace {

void skin_drop_handles(srt_pt_skin* k) {
  k->ik_joints.clear(); k->ik_off.clear(); k->ik_list.clear();
  k->d_ik_joints.reset(); k->d_ik_off.reset(); k->d_ik_list.reset(); k->d_ik_targets.reset(); k->d_ik_enabled.reset();
}

// What srt_pt_skin_set_rig put on the device goes (the caller has waited for what reads it).
void skin_drop_rig(srt_pt_skin* k) {
  k->d_parent.reset(); k->d_knot_offsets.reset(); k->d_base.reset(); k->d_rest_pose.reset(); k->d_knot_times.reset(); k->d_knot_quats.reset(); k->d_local.reset();
  k->d_pose.reset(); k->d_ik_scratch.reset();
  k->rigged = false;
  skin_drop_handles(k);
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
  launch_skin_last_triangle(s, pt->mesh.d_idx + pt->mesh.idx_off[k->object], k->ntri, k->nverts, k->d_last);
  SRT_HIP(hipStreamSynchronize(s));
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int skin_usable(const srt_pt_skin* k, const char* what) {
  if (!k) return srt::fail(SRT_ERR_INVALID, "%s: NULL skin", what);
  if (k->stale()) return srt::fail(SRT_ERR_STATE, "%s: the skin is stale - its context's scene was begun or committed again after srt_pt_skin_create", what);
  return SRT_OK;
}

// The skinning kernels on s, behind whatever wrote the frame's matrices into d_mats there.
void skin_launch(srt_pt_skin* k, hipStream_t s, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  launch_skin_vertices(s, k->d_pos, k->d_nrm, k->nverts, k->d_mats, k->njoints, k->d_off, k->d_jidx, k->d_w, d_pos_out, flat_normals ? nullptr : d_nrm_out);
  if (flat_normals)
    launch_skin_flat_normals(s, d_pos_out, k->d_nrm, k->pt->mesh.d_idx + k->pt->mesh.idx_off[k->object], k->ntri, k->d_last, k->nverts, d_nrm_out);
}

// Enqueues the frame's matrices and the skinning kernels on s, for a skin that is usable.
int skin_enqueue(srt_pt_skin* k, const char* what, hipStream_t s, const float* posed, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  const int usable = skin_usable(k, what);
  if (usable != SRT_OK) return usable;
  SRT_HIP(hipSetDevice(k->pt->device));
  srt_pt_skin::Mats* m = nullptr;
  for (auto& c : k->mats) {
    const hipError_t left = hipEventQuery(c.done);
    (void)hipGetLastError();                              // (hipErrorNotReady of a query is no error: not left behind for the launch check)
    if (left == hipSuccess) { m = &c; break; }
  }
  if (!m) {
    srt_pt_skin::Mats fresh;
    if (fresh.h.ensure(k->inv.size())) return srt::fail(SRT_ERR_HIP, "%s: out of pinned host memory", what);
    if (fresh.done.create(hipEventDisableTiming)) return srt::fail(SRT_ERR_HIP, "%s: event creation failed", what);
    k->mats.push_back(std::move(fresh));
    m = &k->mats.back();
  }
  float* const h = m->h;
  for (uint32_t j = 0; j < k->njoints; j++) skin_mat4_mul(posed + 16 * (size_t)j, &k->inv[16 * (size_t)j], h + 16 * (size_t)j);
  SRT_HIP(hipMemcpyAsync(k->d_mats, h, k->inv.size() * sizeof(float), hipMemcpyHostToDevice, s));   // 64 B per joint
  SRT_HIP(hipEventRecord(m->done, s));
  k->pt->bytes_uploaded += k->inv.size() * sizeof(float);
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

// What srt_pt_skin_set_rig refuses about its arrays, as a message (empty: nothing).
std::string check_parents(uint32_t njoints, const int32_t* parent) {
  for (uint32_t j = 0; j < njoints; j++)
    if (parent[j] < -1 || parent[j] >= (int32_t)j)
      return "joint " + std::to_string(j) + " has parent " + std::to_string(parent[j]) + " (-1, or a joint in front of it: parents come first, as Skeleton::for_joints visits them)";
  return std::string();
}

std::string check_rig(uint32_t njoints, const int32_t* parent, const uint32_t* knot_offsets, const float* knot_times) {
  const std::string refused = check_parents(njoints, parent);
  if (!refused.empty()) return refused;
  return anim_check_tracks(knot_offsets, njoints, 1, knot_times, false, "joint");
}

// The host's mirror of the current pose, read back when an enqueue-only call has left it behind (waits).
int pose_settle(srt_pt_skin* k) {
  if (!k->pose_lags) return SRT_OK;
  SRT_HIP(quiesce(k->pt));
  SRT_HIP(hipMemcpy(k->pose.data(), k->d_pose, k->pose.size() * sizeof(float), hipMemcpyDeviceToHost));
  k->pose_lags = false;
  return SRT_OK;
}

// The skin's matrices from the current pose on s, then the skinning kernels: skin_enqueue_at with another source of Euler angles.
int skin_enqueue_current(srt_pt_skin* k, const char* what, hipStream_t s, int flat_normals, float* d_pos_out, float* d_nrm_out) {
  const int rigged = skin_rigged(k, what);
  if (rigged != SRT_OK) return rigged;
  SRT_HIP(hipSetDevice(k->pt->device));
  launch_anim_joints_pose(s, k->d_parent, k->d_cap, k->d_base, k->d_pose, k->njoints, k->d_local, k->d_inv, k->d_mats, nullptr);
  skin_launch(k, s, flat_normals, d_pos_out, d_nrm_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

// A rigged skin with handles, for srt_pt_skin_step_ik*.
int skin_has_handles(const srt_pt_skin* k, const char* what) {
  const int rigged = skin_rigged(k, what);
  if (rigged != SRT_OK) return rigged;
  if (k->ik_joints.empty()) return srt::fail(SRT_ERR_STATE, "%s: the skin has no IK handles (srt_pt_skin_set_ik_handles)", what);
  return SRT_OK;
}

void ik_launch(srt_pt_skin* k, hipStream_t s, const float* d_targets, const uint8_t* d_enabled) {
  launch_ik_step(s, k->d_parent, k->d_cap, k->njoints, k->d_ik_joints, (uint32_t)k->ik_joints.size(), k->d_ik_off, k->d_ik_list, d_targets, d_enabled, k->d_ik_scratch, k->d_pose);
  k->pose_lags = true;
}

}  // namespace

extern "C" {

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
  return handle_publish(k, skin, [&]() -> int {
    if (pt->mesh.idx_off[object] == SIZE_MAX) {           // an emissive mesh under srt_pt_set_dynamic_lights: its index buffer goes up now
      if (quiesce(pt) != hipSuccess) return srt::fail(SRT_ERR_HIP, "srt_pt_skin_create: synchronisation failed");
      const int st = ensure_mesh_idx(pt, object);
      if (st != SRT_OK) return st;
      pt->bytes_uploaded += pt->mesh.idx_uncounted;
      pt->mesh.idx_uncounted = 0;
    }
    return skin_build(k, bind_positions, bind_normals, joints);
  });
}

int srt_pt_skin_destroy(srt_pt_skin* skin) { return handle_destroy(skin); }

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
  // the current pose starts as the rest pose (device to device: nothing more goes up)
  if (skin->d_pose.ensure(3 * (size_t)nj) || skin->d_ik_scratch.ensure((size_t)kIkJointFloats * nj)) {
    (void)hipGetLastError();
    return srt::fail(SRT_ERR_HIP, "%s: out of device memory", what);
  }
  SRT_HIP(hipMemcpy(skin->d_pose, skin->d_rest_pose, 3 * (size_t)nj * sizeof(float), hipMemcpyDeviceToDevice));
  skin->pose = skin->rest_pose;
  skin->pose_lags = false;
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

int srt_pt_skin_pose_inplace(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals) {
  const char* what = "srt_pt_skin_pose_inplace";
  if (!skin || !posed) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_enqueue(skin, what, (hipStream_t)stream, posed, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  return refit_mesh_inplace_device(skin->pt, what, (hipStream_t)stream, skin->object, skin->d_pos_out, skin->d_nrm_out, skin->nverts);
}

int srt_pt_skin_pose_inplace_at(srt_pt_skin* skin, void* stream, float t, int flat_normals) {
  const char* what = "srt_pt_skin_pose_inplace_at";
  if (!skin) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_enqueue_at(skin, what, (hipStream_t)stream, t, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  return refit_mesh_inplace_device(skin->pt, what, (hipStream_t)stream, skin->object, skin->d_pos_out, skin->d_nrm_out, skin->nverts);
}

int srt_pt_skin_set_ik_handles(srt_pt_skin* skin, const uint32_t* joints, uint32_t n) {
  const char* what = "srt_pt_skin_set_ik_handles";
  if (!skin || (n && !joints)) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st = skin_rigged(skin, what);
  if (st != SRT_OK) return st;
  if (!ik_supported(skin->njoints, n)) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: %u handles (at most %u per skin)", what, n, kIkMaxHandles);
  const std::string refused = ik_check_handles(joints, n, skin->njoints);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt* pt = skin->pt;
  SRT_HIP(quiesce(pt));                                   // (the handles set before may still be read)
  skin_drop_handles(skin);
  if (!n) return SRT_OK;
  skin->ik_joints.assign(joints, joints + n);
  ik_build_csr(skin->parent.data(), skin->njoints, joints, n, skin->ik_off, skin->ik_list);
  if ((st = skin->d_ik_joints.upload(skin->ik_joints)) || (st = skin->d_ik_off.upload(skin->ik_off)) || (st = skin->d_ik_list.upload(skin->ik_list)) ||
      (st = skin->d_ik_targets.ensure(3 * (size_t)n)) || (st = skin->d_ik_enabled.ensure(n))) {
    skin_drop_handles(skin);
    return st;
  }
  pt->bytes_uploaded += (skin->ik_joints.size() + skin->ik_off.size() + skin->ik_list.size()) * sizeof(uint32_t);
  return SRT_OK;
}

int srt_pt_skin_set_joint_pose(srt_pt_skin* skin, const float* euler3) {
  const char* what = "srt_pt_skin_set_joint_pose";
  if (!skin || !euler3) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_rigged(skin, what);
  if (st != SRT_OK) return st;
  SRT_HIP(quiesce(skin->pt));                             // (an enqueued call may still read or write the pose)
  SRT_HIP(hipMemcpy(skin->d_pose, euler3, skin->pose.size() * sizeof(float), hipMemcpyHostToDevice));
  skin->pose.assign(euler3, euler3 + skin->pose.size());
  skin->pose_lags = false;
  skin->pt->bytes_uploaded += skin->pose.size() * sizeof(float);
  return SRT_OK;
}

int srt_pt_skin_joint_pose(srt_pt_skin* skin, float* euler3_out) {
  const char* what = "srt_pt_skin_joint_pose";
  if (!skin || !euler3_out) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st = skin_rigged(skin, what);
  if (st != SRT_OK || (st = pose_settle(skin)) != SRT_OK) return st;
  std::memcpy(euler3_out, skin->pose.data(), skin->pose.size() * sizeof(float));
  return SRT_OK;
}

int srt_pt_skin_set_time(srt_pt_skin* skin, void* stream, float t) {
  const char* what = "srt_pt_skin_set_time";
  if (!skin) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_rigged(skin, what);
  if (st != SRT_OK) return st;
  SRT_HIP(hipSetDevice(skin->pt->device));
  launch_ik_set_time((hipStream_t)stream, skin->d_knot_offsets, skin->d_knot_times, skin->d_knot_quats, skin->njoints, t, skin->d_pose);
  skin->pose_lags = true;
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_skin_step_ik(srt_pt_skin* skin, const float* targets3, const uint8_t* enabled) {
  const char* what = "srt_pt_skin_step_ik";
  if (!skin || !targets3) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_has_handles(skin, what);
  if (st != SRT_OK) return st;
  srt_pt* pt = skin->pt;
  SRT_HIP(quiesce(pt));                                   // (an enqueue-only call on another stream may still use the pose or the staging)
  hipStream_t s = pt->stream;
  const size_t n = skin->ik_joints.size();
  SRT_HIP(hipMemcpyAsync(skin->d_ik_targets, targets3, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
  if (enabled) SRT_HIP(hipMemcpyAsync(skin->d_ik_enabled, enabled, n, hipMemcpyHostToDevice, s));
  pt->bytes_uploaded += 3 * n * sizeof(float) + (enabled ? n : 0);
  ik_launch(skin, s, skin->d_ik_targets, enabled ? skin->d_ik_enabled.get() : nullptr);
  SRT_HIP(hipGetLastError());
  SRT_HIP(hipStreamSynchronize(s));
  return pose_settle(skin);
}

int srt_pt_skin_step_ik_device(srt_pt_skin* skin, void* stream, const float* d_targets3, const uint8_t* d_enabled) {
  const char* what = "srt_pt_skin_step_ik_device";
  if (!skin || !d_targets3) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_has_handles(skin, what);
  if (st != SRT_OK) return st;
  SRT_HIP(hipSetDevice(skin->pt->device));
  ik_launch(skin, (hipStream_t)stream, d_targets3, d_enabled);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_skin_posed_current(srt_pt_skin* skin, float* posed_out) {
  const char* what = "srt_pt_skin_posed_current";
  if (!skin || !posed_out) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st = skin_rigged(skin, what);
  if (st != SRT_OK || (st = pose_settle(skin)) != SRT_OK) return st;
  std::vector<float> local(16 * (size_t)skin->njoints);
  for (uint32_t j = 0; j < skin->njoints; j++) anim_mat4_euler(anim_v3(&skin->pose[3 * (size_t)j]), &local[16 * (size_t)j]);
  for (uint32_t j = 0; j < skin->njoints; j++)
    anim_joint_to_posed(skin->parent.data(), skin->cap.data(), skin->base, local.data(), skin->njoints, j, posed_out + 16 * (size_t)j);
  return SRT_OK;
}

int srt_pt_skin_posed_current_device(srt_pt_skin* skin, void* stream, float* d_posed_out) {
  const char* what = "srt_pt_skin_posed_current_device";
  if (!skin || !d_posed_out) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  const int st = skin_rigged(skin, what);
  if (st != SRT_OK) return st;
  SRT_HIP(hipSetDevice(skin->pt->device));
  launch_anim_joints_pose((hipStream_t)stream, skin->d_parent, skin->d_cap, skin->d_base, skin->d_pose, skin->njoints, skin->d_local, skin->d_inv, nullptr, d_posed_out);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_skin_vertices_current_device(srt_pt_skin* skin, void* stream, int flat_normals, float* d_positions_out, float* d_normals_out) {
  if (!skin || !d_positions_out || !d_normals_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_skin_vertices_current_device: NULL argument");
  return skin_enqueue_current(skin, "srt_pt_skin_vertices_current_device", (hipStream_t)stream, flat_normals, d_positions_out, d_normals_out);
}

int srt_pt_skin_pose_current(srt_pt_skin* skin, void* stream, int flat_normals, int how) {
  const char* what = "srt_pt_skin_pose_current";
  if (!skin) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (how != SRT_PT_SKIN_UPDATE && how != SRT_PT_SKIN_REFIT && how != SRT_PT_SKIN_INPLACE)
    return srt::fail(SRT_ERR_INVALID, "%s: how = %d (SRT_PT_SKIN_UPDATE, SRT_PT_SKIN_REFIT or SRT_PT_SKIN_INPLACE)", what, how);
  const int st = skin_enqueue_current(skin, what, (hipStream_t)stream, flat_normals, skin->d_pos_out, skin->d_nrm_out);
  if (st != SRT_OK) return st;
  if (how == SRT_PT_SKIN_INPLACE)
    return refit_mesh_inplace_device(skin->pt, what, (hipStream_t)stream, skin->object, skin->d_pos_out, skin->d_nrm_out, skin->nverts);
  return (how == SRT_PT_SKIN_UPDATE ? update_mesh : refit_mesh)(skin->pt, what, (hipStream_t)stream, skin->object,
                                                               {nullptr, nullptr, skin->d_pos_out, skin->d_nrm_out, {}, {}}, skin->nverts);
}

int srt_pt_rig_step_ik_host(uint32_t njoints, const int32_t* parent, const float* extents, float* pose_inout, const uint32_t* handle_joints,
                            const float* targets, const uint8_t* enabled, uint32_t nhandles, uint32_t calls) {
  const char* what = "srt_pt_rig_step_ik_host";
  if (!parent || !extents || !pose_inout || (nhandles && (!handle_joints || !targets))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (!ik_supported(njoints, nhandles))
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: %u joints and %u handles (at most %u and %u)", what, njoints, nhandles, kSkinMaxJoints, kIkMaxHandles);
  std::string refused = check_parents(njoints, parent);
  if (refused.empty()) refused = ik_check_handles(handle_joints, nhandles, njoints);
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<float> cap(4 * (size_t)njoints, 0.0f), scratch((size_t)kIkJointFloats * njoints);
  for (uint32_t j = 0; j < njoints; j++)
    for (int a = 0; a < 3; a++) cap[4 * (size_t)j + a] = extents[3 * (size_t)j + a];
  std::vector<uint32_t> off, list;
  ik_build_csr(parent, njoints, handle_joints, nhandles, off, list);
  for (uint32_t c = 0; c < calls; c++) ik_step_host(parent, cap.data(), njoints, handle_joints, off.data(), list.data(), targets, enabled, scratch.data(), pose_inout);
  return SRT_OK;
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

}  // extern "C"
