// The Animate mode's timeline on the device: the launches around the per-object and per-joint functions of pt_anim.h.  One lane
// per object or joint.  The kernels are small and latency-bound - a lane's work is three binary searches over its own knots, a
// handful of transcendentals and a few 4 x 4 products from registers - and their point is that the frame's transforms are made
// where the refit reads them: nothing here waits for the host or reads host memory.  Knot tables are CSR, read at per-lane
// indices; every index a lane forms lies inside its own tracks [offsets[i], offsets[i + 1]), which the host validated against the
// table sizes before the upload.  The chain of a joint is walked by its own lane, parent by parent, in the reference's order: a
// parallel prefix over the hierarchy would re-associate float matrix products, which do not associate.
#include <hip/hip_runtime.h>

#include "pt_anim.h"
#include "pt_pose.h"

namespace srt {
namespace {

constexpr uint32_t kBlock = 64;           // one wave per block: a rig has a few dozen joints, a timeline a few thousand objects

__global__ __launch_bounds__(kBlock) void anim_pose_kernel(const uint32_t* __restrict__ track_offsets, const float* __restrict__ times,
                                                          const float* __restrict__ values, uint32_t nobjects, float t, float* __restrict__ trans_out) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= nobjects) return;
  float m[16];
  anim_object_transform(track_offsets, times, values, k, t, nullptr, m);
  for (int i = 0; i < 16; i++) trans_out[16 * (size_t)k + i] = m[i];
}

__global__ __launch_bounds__(kBlock) void anim_joint_local_kernel(const float* __restrict__ rest_pose, const uint32_t* __restrict__ knot_offsets,
                                                                 const float* __restrict__ times, const float* __restrict__ quats, uint32_t njoints, float t,
                                                                 float* __restrict__ local) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= njoints) return;
  float m[16];
  anim_mat4_euler(anim_joint_pose(rest_pose, knot_offsets, times, quats, j, t), m);
  for (int i = 0; i < 16; i++) local[16 * (size_t)j + i] = m[i];
}

// The same from the skin's current Joint::pose (srt_pt_skin_*_current): only the source of the Euler angles differs.
__global__ __launch_bounds__(kBlock) void anim_joint_local_pose_kernel(const float* __restrict__ pose, uint32_t njoints, float* __restrict__ local) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= njoints) return;
  float m[16];
  anim_mat4_euler(anim_v3(pose + 3 * (size_t)j), m);
  for (int i = 0; i < 16; i++) local[16 * (size_t)j + i] = m[i];
}

__global__ __launch_bounds__(kBlock) void anim_joint_chain_kernel(const int32_t* __restrict__ parent, const float* __restrict__ cap,
                                                                 const float* __restrict__ base, const float* __restrict__ local, uint32_t njoints,
                                                                 const float* __restrict__ inv, float* __restrict__ mats, float* __restrict__ posed_out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= njoints) return;
  float posed[16], m[16];
  anim_joint_to_posed(parent, cap, base, local, njoints, j, posed);
  if (mats) {
    skin_mat4_mul(posed, inv + 16 * (size_t)j, m);                   // M_j = joint_to_posed(j) * inverse(joint_to_bind(j))
    for (int i = 0; i < 16; i++) mats[16 * (size_t)j + i] = m[i];
  }
  if (posed_out)
    for (int i = 0; i < 16; i++) posed_out[16 * (size_t)j + i] = posed[i];
}

// srt_pt_shading_timeline_apply.  Materials first, then lights: a wave at the boundary runs both branches once, every other wave
// one.  A lane reads and writes its own record only (the host refused duplicate indices), at an index the host checked against
// the table; the matrices of a light take the arithmetic launch_pose_objects gives an object's (pose_inverse, pose_ne_identity).
__global__ __launch_bounds__(kBlock) void anim_shading_kernel(const uint32_t* __restrict__ track_offsets, const float* __restrict__ times,
                                                             const float* __restrict__ values, const uint32_t* __restrict__ materials, uint32_t nmaterials,
                                                             const uint32_t* __restrict__ lights, uint32_t nlights, float t, Material* __restrict__ mats,
                                                             DeltaLight* __restrict__ dlights) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k < nmaterials) {
    Material* dst = mats + materials[k];
    Material m;
    m.type = dst->type;
    anim_material_item(track_offsets, times, values, k, t, &m);
    anim_material_store(&m);
    for (int i = 0; i < 3; i++) { dst->a[i] = m.a[i]; dst->b[i] = m.b[i]; }
    dst->ior = m.ior;
    return;
  }
  const uint32_t j = k - nmaterials;
  if (j >= nlights) return;
  DeltaLight* dst = dlights + lights[j];
  AnimLightOut out;
  anim_light_item(track_offsets + 6 * (size_t)nmaterials + 6 * (size_t)j, times, values, t, &out);
  if (out.options) {
    for (int i = 0; i < 3; i++) dst->radiance[i] = out.radiance[i];
    dst->angle_bounds[0] = out.angle_bounds[0]; dst->angle_bounds[1] = out.angle_bounds[1];
  }
  if (out.pose) {
    float inv[16];
    pose_inverse(out.trans, inv);
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) { dst->trans.c[c][r] = out.trans[4 * c + r]; dst->itrans.c[c][r] = inv[4 * c + r]; }
    dst->has_trans = pose_ne_identity(out.trans) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void anim_hypot_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = srt_hypotf(x[i], y[i]);
}

dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1u) / kBlock); }

}  // namespace

void launch_anim_pose(void* stream, const uint32_t* d_track_offsets, const float* d_times, const float* d_values, uint32_t nobjects, float t, float* d_trans_out) {
  if (!nobjects) return;
  anim_pose_kernel<<<grid_for(nobjects), dim3(kBlock), 0, (hipStream_t)stream>>>(d_track_offsets, d_times, d_values, nobjects, t, d_trans_out);
}

void launch_anim_joints(void* stream, const int32_t* d_parent, const float* d_cap, const float* d_base, const float* d_rest_pose, const uint32_t* d_knot_offsets,
                        const float* d_times, const float* d_quats, uint32_t njoints, float t, float* d_local, const float* d_inv, float* d_mats,
                        float* d_posed_out) {
  if (!njoints) return;
  anim_joint_local_kernel<<<grid_for(njoints), dim3(kBlock), 0, (hipStream_t)stream>>>(d_rest_pose, d_knot_offsets, d_times, d_quats, njoints, t, d_local);
  anim_joint_chain_kernel<<<grid_for(njoints), dim3(kBlock), 0, (hipStream_t)stream>>>(d_parent, d_cap, d_base, d_local, njoints, d_inv, d_mats, d_posed_out);
}

void launch_anim_joints_pose(void* stream, const int32_t* d_parent, const float* d_cap, const float* d_base, const float* d_pose, uint32_t njoints,
                             float* d_local, const float* d_inv, float* d_mats, float* d_posed_out) {
  if (!njoints) return;
  anim_joint_local_pose_kernel<<<grid_for(njoints), dim3(kBlock), 0, (hipStream_t)stream>>>(d_pose, njoints, d_local);
  anim_joint_chain_kernel<<<grid_for(njoints), dim3(kBlock), 0, (hipStream_t)stream>>>(d_parent, d_cap, d_base, d_local, njoints, d_inv, d_mats, d_posed_out);
}

void launch_anim_shading(void* stream, const uint32_t* d_track_offsets, const float* d_times, const float* d_values, const uint32_t* d_materials,
                         uint32_t nmaterials, const uint32_t* d_lights, uint32_t nlights, float t, Material* d_mats, DeltaLight* d_dlights) {
  if (!(nmaterials + nlights)) return;
  anim_shading_kernel<<<grid_for(nmaterials + nlights), dim3(kBlock), 0, (hipStream_t)stream>>>(d_track_offsets, d_times, d_values, d_materials, nmaterials,
                                                                                             d_lights, nlights, t, d_mats, d_dlights);
}

void launch_anim_hypot(void* stream, const float* d_x, const float* d_y, size_t n, float* d_out) {
  if (!n) return;
  anim_hypot_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(d_x, d_y, n, d_out);
}

}  // namespace srt
