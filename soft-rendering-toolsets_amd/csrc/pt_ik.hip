// Skeleton::step_ik on the device: one launch, one workgroup, all 50 iterations of pt_ik.h's phases with workgroup barriers between
// them - no host round trip, no cooperative launch, no float atomics.  Joints are strided over the workgroup's lanes; a lane walks
// its own joint's chain in the reference's order and sums its own joint's gradient in handle order (the CSR lists ascend), so the
// association of every float sum is the reference's.  What the phases hand each other - local_j for the chains of other lanes,
// {origin, axes}_j and current_j for the update - lives in LDS for a rig of up to kIkLdsJoints joints, together with the poses, the
// hierarchy and the extents, and in the skin's device scratch (poses: in d_pose itself) beyond; the scratch is written and read by the
// waves of one workgroup only, with a barrier - which orders global memory at workgroup scope too - between the writers and the
// readers.  The handles' joints, flags and targets and every joint's flags are in LDS for a rig of any size.
//
// Every index is inside its table: csr_list holds handles < nhandles and handle_joint joints < njoints (validated on the host
// before the upload), a lane touches records j < njoints only, and the chain walk stops at the root or after njoints steps.
#include <hip/hip_runtime.h>

#include "pt_ik.h"

namespace srt {
namespace {

template <bool kLds>
__global__ __launch_bounds__(kIkBlock) void ik_step_kernel(const int32_t* __restrict__ g_parent, const float* __restrict__ g_cap, uint32_t njoints,
                                                          const uint32_t* __restrict__ g_handle_joint, uint32_t nhandles, const uint32_t* __restrict__ csr_off,
                                                          const uint32_t* __restrict__ csr_list, const float* __restrict__ g_targets,
                                                          const uint8_t* __restrict__ g_enabled, float* scratch, float* d_pose) {
  // What every iteration reads again and a lane reaches through dependent loads - the handles' joints, flags and targets, each joint's
  // flags, and for a rig that fits the hierarchy and the extents - is copied into LDS once: a chain walk is as many dependent loads
  // as the joint is deep, and 50 iterations of them at global-memory latency were most of the kernel's time.
  __shared__ float lds[kLds ? (kIkJointFloats + 3) * kIkLdsJoints : 1];
  __shared__ int32_t s_parent[kLds ? kIkLdsJoints : 1];
  __shared__ float s_cap[kLds ? 4 * kIkLdsJoints : 1];
  __shared__ uint32_t s_handle_joint[kIkMaxHandles];
  __shared__ float s_targets[3 * kIkMaxHandles];
  __shared__ uint8_t s_enabled[kIkMaxHandles];
  __shared__ uint8_t s_flags[kSkinMaxJoints];
  float* const local = kLds ? lds : scratch;
  float* const frame = local + 16 * (size_t)njoints;
  float* const current = frame + 12 * (size_t)njoints;
  float* const pose = kLds ? current + 3 * (size_t)njoints : d_pose;
  const int32_t* const parent = kLds ? s_parent : g_parent;
  const float* const cap = kLds ? s_cap : g_cap;
  const uint32_t lane = threadIdx.x;
  for (uint32_t h = lane; h < nhandles && h < kIkMaxHandles; h += kIkBlock) {
    s_handle_joint[h] = g_handle_joint[h];
    s_enabled[h] = ik_enabled(g_enabled, h) ? (uint8_t)1 : (uint8_t)0;
    for (int a = 0; a < 3; a++) s_targets[3 * h + a] = g_targets[3 * (size_t)h + a];
  }
  if (kLds)
    for (uint32_t j = lane; j < njoints; j += kIkBlock) {
      s_parent[j] = g_parent[j];
      for (int a = 0; a < 4; a++) s_cap[4 * j + a] = g_cap[4 * (size_t)j + a];
      for (int a = 0; a < 3; a++) pose[3 * j + a] = d_pose[3 * (size_t)j + a];
    }
  __syncthreads();
  for (uint32_t j = lane; j < njoints && j < kSkinMaxJoints; j += kIkBlock) s_flags[j] = (uint8_t)ik_joint_flags(csr_off, csr_list, s_handle_joint, s_enabled, j);
  // (a lane reads and writes the poses and the flags of its own joints only: no barrier is needed for them)
  for (uint32_t it = 0; it < kIkIterations; it++) {
    for (uint32_t j = lane; j < njoints; j += kIkBlock)
      if (s_flags[j]) ik_phase_local(pose, j, local);
    __syncthreads();
    for (uint32_t j = lane; j < njoints; j += kIkBlock)
      if (s_flags[j]) ik_phase_chain(parent, cap, local, njoints, j, (s_flags[j] & 2u) != 0, frame, current);
    __syncthreads();
    for (uint32_t j = lane; j < njoints; j += kIkBlock)
      if (s_flags[j]) ik_phase_update(csr_off, csr_list, s_handle_joint, s_enabled, s_targets, frame, current, j, pose);
    // (the next iteration's first phase writes local only, which the third phase does not read; its barrier stands between this
    // phase's reads of frame / current and the second phase's next writes)
  }
  if (kLds)
    for (uint32_t j = lane; j < njoints; j += kIkBlock)
      for (int a = 0; a < 3; a++) d_pose[3 * (size_t)j + a] = pose[3 * j + a];
}

__global__ __launch_bounds__(64) void ik_set_time_kernel(const uint32_t* __restrict__ knot_offsets, const float* __restrict__ times,
                                                        const float* __restrict__ quats, uint32_t njoints, float t, float* __restrict__ pose) {
  const uint32_t j = blockIdx.x * 64u + threadIdx.x;
  if (j >= njoints) return;
  const uint32_t b = knot_offsets[j], e = knot_offsets[j + 1u];
  if (e <= b) return;                                                // `if(j->anim.any())`: a joint without keys keeps its pose
  const AnimV3 p = anim_quat_to_euler(anim_spline_quat(times, quats, b, e, t));
  pose[3 * (size_t)j] = p.x; pose[3 * (size_t)j + 1] = p.y; pose[3 * (size_t)j + 2] = p.z;
}

}  // namespace

void launch_ik_step(void* stream, const int32_t* d_parent, const float* d_cap, uint32_t njoints, const uint32_t* d_handle_joint, uint32_t nhandles,
                    const uint32_t* d_csr_off, const uint32_t* d_csr_list, const float* d_targets, const uint8_t* d_enabled, float* d_scratch, float* d_pose) {
  if (!njoints || njoints > kSkinMaxJoints || nhandles > kIkMaxHandles) return;   // (refused by the callers: the kernel's tables are this large)
  if (njoints <= kIkLdsJoints)
    ik_step_kernel<true><<<dim3(1), dim3(kIkBlock), 0, (hipStream_t)stream>>>(d_parent, d_cap, njoints, d_handle_joint, nhandles, d_csr_off, d_csr_list, d_targets,
                                                                             d_enabled, d_scratch, d_pose);
  else
    ik_step_kernel<false><<<dim3(1), dim3(kIkBlock), 0, (hipStream_t)stream>>>(d_parent, d_cap, njoints, d_handle_joint, nhandles, d_csr_off, d_csr_list, d_targets,
                                                                              d_enabled, d_scratch, d_pose);
}

void launch_ik_set_time(void* stream, const uint32_t* d_knot_offsets, const float* d_times, const float* d_quats, uint32_t njoints, float t, float* d_pose) {
  if (!njoints) return;
  ik_set_time_kernel<<<dim3((njoints + 63u) / 64u), dim3(64), 0, (hipStream_t)stream>>>(d_knot_offsets, d_times, d_quats, njoints, t, d_pose);
}

}  // namespace srt
