// Skeleton::step_ik (student/skeleton.cpp:165-191) with Joint::compute_gradient (:117-163) as functions for the device and the
// host: 50 iterations of Jacobian-transpose gradient descent on Joint::pose, restated operation for operation.  pt_ik.hip runs one
// workgroup per skeleton; the host runs the same functions (ik_step_host: srt_pt_rig_step_ik_host, the definition the kernel is held
// to) and the host emulation (tests/host_emu/ik_host.cpp) compiles this header with g++ -ffp-contract=off.
//
// One iteration, as the reference orders it:
//   (A) local_j = Mat4::euler(pose_j);
//   (B) J_j = Joint::joint_to_posed of joint j - the walk of anim_joint_chain, skeleton space, no translate(base_pos) - and from
//       it the four points compute_gradient takes from J: J * Vec3(0,0,0), J * Vec3(1,0,0), J * Vec3(0,1,0), J * Vec3(0,0,1), each
//       a full Mat4 * Vec3 (translation and the projection's three divisions included, as written there); for the joint of a
//       handle, current = J * extent.  Poses do not change between (A) and (C), so every handle of an iteration sees the same
//       matrices: the four points are computed once per joint and iteration, not once per handle;
//   (C) angle_gradient_j = the sum, from 0.0f, over the enabled handles whose chain (the handle's joint and its ancestors) holds
//       joint j, IN HANDLE ORDER, of dot(cross(axis, current_h - origin_j), current_h - target_h) per axis; then
//       pose_j = pose_j - tau * angle_gradient_j with tau = 1 / 50.0f.
// The order of (C)'s sum is the order Skeleton::do_ik collected the handles in and is part of the result: floats do not associate.
// Hence no tree reduction and no float atomics: each joint's sum is one lane's loop over a CSR list the host made once per handle
// set (ik_build_csr: per joint, the handles whose chain holds it, ascending).  A joint no enabled handle reaches is left alone: the
// reference computes pose - tau * Vec3(), which is the same bits.
//
// sin / cos are SRT-MATH v2's (pt_anim.h): bit-equal to the reference while every angle stays below 6875 degrees, NaN beyond.
#ifndef SRT_PT_IK_H
#define SRT_PT_IK_H

#include <string>
#include <vector>

#include "pt_anim.h"

namespace srt {

constexpr uint32_t kIkIterations = 50;      // `float frames = 50.0f; while(frames--)`
// Limits: kSkinMaxJoints joints (pt_skin.h) and kIkMaxHandles handles per skin (SRT_ERR_UNSUPPORTED beyond): the CSR holds one
// entry per (handle, joint of its chain), at most kIkMaxHandles * kSkinMaxJoints = 4 Mi entries of 4 B.
constexpr uint32_t kIkMaxHandles = 1024;
constexpr uint32_t kIkBlock = 256;          // lanes of the one workgroup; joints are strided over them
constexpr uint32_t kIkLdsJoints = 256;      // up to here the per-joint values live in LDS (156 B per joint), beyond in the skin's device scratch
constexpr uint32_t kIkJointFloats = 16 + 12 + 3;   // per joint: local, {origin, x, y, z}, current

// Mat4 * Vec3 (lib/mat4.h:149-156): v0 * col0 + v1 * col1 + v2 * col2 + 1.0f * col3, then Vec4::project - three divisions by w.
SRT_ANIM_FN AnimV3 ik_mat_point(const float* m, AnimV3 p) {
  float r[4];
  for (int a = 0; a < 4; a++) r[a] = ((p.x * m[a] + p.y * m[4 + a]) + p.z * m[8 + a]) + 1.0f * m[12 + a];
  return {r[0] / r[3], r[1] / r[3], r[2] / r[3]};
}

// dot and cross of lib/vec3.h:209-216; dot associates (a + b) + c
SRT_ANIM_FN float ik_dot(AnimV3 l, AnimV3 r) { return (l.x * r.x + l.y * r.y) + l.z * r.z; }
SRT_ANIM_FN AnimV3 ik_cross(AnimV3 l, AnimV3 r) { return {l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x}; }

// What compute_gradient takes from J = joint_to_posed(): frame[0..3) = J * Vec3(0,0,0), then J * the three unit vectors.
SRT_ANIM_FN void ik_joint_frame(const float* J, float* frame) {
  const AnimV3 pts[4] = {{0.0f, 0.0f, 0.0f}, {1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};
  for (int k = 0; k < 4; k++) {
    const AnimV3 q = ik_mat_point(J, pts[k]);
    frame[3 * k] = q.x; frame[3 * k + 1] = q.y; frame[3 * k + 2] = q.z;
  }
}

// One handle's contribution to one joint's angle_gradient (:127-141).
SRT_ANIM_FN AnimV3 ik_gradient_term(const float* frame, AnimV3 current, AnimV3 target) {
  const AnimV3 p = current - anim_v3(frame);
  const AnimV3 d = current - target;
  return {ik_dot(ik_cross(anim_v3(frame + 3), p), d), ik_dot(ik_cross(anim_v3(frame + 6), p), d), ik_dot(ik_cross(anim_v3(frame + 9), p), d)};
}

// enabled: one byte per handle, nonzero = enabled (srt_pt_set_active_device's convention); NULL = every handle.
SRT_ANIM_FN bool ik_enabled(const uint8_t* enabled, uint32_t h) { return !enabled || enabled[h] != 0; }

// Bit 0: an enabled handle's chain holds joint j; bit 1: j is itself the joint of an enabled handle (its `current` is needed).
SRT_ANIM_FN uint32_t ik_joint_flags(const uint32_t* csr_off, const uint32_t* csr_list, const uint32_t* handle_joint, const uint8_t* enabled, uint32_t j) {
  uint32_t f = 0;
  for (uint32_t k = csr_off[j]; k < csr_off[j + 1u]; k++) {
    const uint32_t h = csr_list[k];
    if (ik_enabled(enabled, h)) f |= handle_joint[h] == j ? 3u : 1u;
  }
  return f;
}

// Phases (A), (B), (C) for one joint.  pose: 3 floats per joint; local: 16; frame: 12; current: 3; cap: the skin's {extent, radius}.
SRT_ANIM_FN void ik_phase_local(const float* pose, uint32_t j, float* local) {
  float m[16];
  anim_mat4_euler(anim_v3(pose + 3 * (size_t)j), m);
  for (int i = 0; i < 16; i++) local[16 * (size_t)j + i] = m[i];
}

SRT_ANIM_FN void ik_phase_chain(const int32_t* parent, const float* cap, const float* local, uint32_t njoints, uint32_t j, bool tip, float* frame,
                                float* current) {
  float J[16], f[12];
  anim_joint_chain(parent, cap, local, njoints, j, J);
  ik_joint_frame(J, f);
  for (int i = 0; i < 12; i++) frame[12 * (size_t)j + i] = f[i];
  if (tip) {
    const AnimV3 c = ik_mat_point(J, anim_v3(cap + 4 * (size_t)j));
    current[3 * (size_t)j] = c.x; current[3 * (size_t)j + 1] = c.y; current[3 * (size_t)j + 2] = c.z;
  }
}

SRT_ANIM_FN void ik_phase_update(const uint32_t* csr_off, const uint32_t* csr_list, const uint32_t* handle_joint, const uint8_t* enabled, const float* targets,
                                 const float* frame, const float* current, uint32_t j, float* pose) {
  AnimV3 g = {0.0f, 0.0f, 0.0f};
  for (uint32_t k = csr_off[j]; k < csr_off[j + 1u]; k++) {
    const uint32_t h = csr_list[k];
    if (!ik_enabled(enabled, h)) continue;
    const AnimV3 t = ik_gradient_term(frame + 12 * (size_t)j, anim_v3(current + 3 * (size_t)handle_joint[h]), anim_v3(targets + 3 * (size_t)h));
    g.x += t.x; g.y += t.y; g.z += t.z;
  }
  const float frames = 50.0f;
  const float tau = 1 / frames;
  const AnimV3 p = anim_v3(pose + 3 * (size_t)j) - g * tau;
  pose[3 * (size_t)j] = p.x; pose[3 * (size_t)j + 1] = p.y; pose[3 * (size_t)j + 2] = p.z;
}

// The documented limits (SRT_ERR_UNSUPPORTED beyond them).
inline bool ik_supported(uint32_t njoints, uint32_t nhandles) { return njoints <= kSkinMaxJoints && nhandles <= kIkMaxHandles; }

// What srt_pt_skin_set_ik_handles refuses about its list, as a message (empty: nothing).  The count is checked first (ik_supported).
inline std::string ik_check_handles(const uint32_t* joints, uint32_t n, uint32_t njoints) {
  for (uint32_t h = 0; h < n; h++)
    if (joints[h] >= njoints) return "handle " + std::to_string(h) + " names joint " + std::to_string(joints[h]) + " of " + std::to_string(njoints);
  return std::string();
}

// Per joint, the handles whose chain holds it, ascending: off[njoints + 1], list[off[njoints]].  parent[j] < j or -1 (check_rig).
inline void ik_build_csr(const int32_t* parent, uint32_t njoints, const uint32_t* handle_joint, uint32_t nhandles, std::vector<uint32_t>& off,
                         std::vector<uint32_t>& list) {
  off.assign((size_t)njoints + 1, 0u);
  for (uint32_t h = 0; h < nhandles; h++)
    for (int32_t c = (int32_t)handle_joint[h]; c >= 0; c = parent[c]) off[(size_t)c + 1]++;
  for (uint32_t j = 0; j < njoints; j++) off[(size_t)j + 1] += off[j];
  list.assign(off[njoints], 0u);
  std::vector<uint32_t> at(off.begin(), off.end() - 1);
  for (uint32_t h = 0; h < nhandles; h++)
    for (int32_t c = (int32_t)handle_joint[h]; c >= 0; c = parent[c]) list[at[c]++] = h;
}

// Skeleton::do_ik once: step_ik's 50 iterations on pose (3 floats per joint, in place) when a handle is enabled, nothing otherwise.
// scratch: njoints * kIkJointFloats floats.
inline void ik_step_host(const int32_t* parent, const float* cap, uint32_t njoints, const uint32_t* handle_joint, const uint32_t* csr_off,
                         const uint32_t* csr_list, const float* targets, const uint8_t* enabled, float* scratch, float* pose) {
  float* local = scratch;
  float* frame = local + 16 * (size_t)njoints;
  float* current = frame + 12 * (size_t)njoints;
  std::vector<uint32_t> flags(njoints);
  for (uint32_t j = 0; j < njoints; j++) flags[j] = ik_joint_flags(csr_off, csr_list, handle_joint, enabled, j);
  for (uint32_t it = 0; it < kIkIterations; it++) {
    for (uint32_t j = 0; j < njoints; j++)
      if (flags[j]) ik_phase_local(pose, j, local);
    for (uint32_t j = 0; j < njoints; j++)
      if (flags[j]) ik_phase_chain(parent, cap, local, njoints, j, (flags[j] & 2u) != 0, frame, current);
    for (uint32_t j = 0; j < njoints; j++)
      if (flags[j]) ik_phase_update(csr_off, csr_list, handle_joint, enabled, targets, frame, current, j, pose);
  }
}

// The launches of pt_ik.hip.  Plain device pointers; `stream` is a hipStream_t; every call only enqueues.
// One workgroup, one whole step_ik on d_pose.  d_scratch: njoints * kIkJointFloats floats, used beyond kIkLdsJoints joints.
// d_enabled may be NULL (every handle enabled).
void launch_ik_step(void* stream, const int32_t* d_parent, const float* d_cap, uint32_t njoints, const uint32_t* d_handle_joint, uint32_t nhandles,
                    const uint32_t* d_csr_off, const uint32_t* d_csr_list, const float* d_targets, const uint8_t* d_enabled, float* d_scratch, float* d_pose);
// Skeleton::set_time on the current pose: a keyed joint takes anim.at(t).to_euler(), one without keys keeps what it has.
void launch_ik_set_time(void* stream, const uint32_t* d_knot_offsets, const float* d_times, const float* d_quats, uint32_t njoints, float t, float* d_pose);

}  // namespace srt

#endif
