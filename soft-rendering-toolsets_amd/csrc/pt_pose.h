// Per-object work of srt_pt_repose_device as device functions: what the Object ctor and Object::bbox make of one transform
// (rays/object.h:18-21, 51-55) - itrans = trans.inverse(), has_trans = trans != I, the posed box - and the transform of one particle
// (rays/pathtracer.cpp:149).  pt_pose.hip runs them one lane per object; the host emulation (tests/host_emu/pose_host.cpp) compiles
// this header with g++ and compares with mat_inverse / mat_ne_identity / Box::transform / mat_mul of pt_scene.cpp, which stay the
// definition: the same products in the same order, the same sums in the same order, the same divide, the same a < b branch (the
// sign of a zero bound is part of the contract of pt_bvh_device.hip).  The library's flags are part of it too: -ffp-contract=off,
// so that no product is fused into a sum, and the IEEE divide - no reciprocal.
// A matrix is sixteen floats in Mat4::data order: m[4 * col + row].
#ifndef SRT_PT_POSE_H
#define SRT_PT_POSE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_scene.h"

namespace srt {

// Mat4::inverse (lib/mat4.h:296-343): sixteen sums of six signed triple products and the determinant's twenty-four quadruple
// products (kInverseTerms / kDetTerms of pt_scene.cpp, written out: mCR is m[col C][row R]); an expression a * b * c - d * e * f + ..
// is evaluated as signed_products walks a table - a product left to right, the sum in order starting from the first product -
// and every element is then divided by det.  A singular matrix gives the infinities and NaNs the reference's gives.
__device__ __forceinline__ void pose_inverse(const float m[16], float r[16]) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3];
  const float m10 = m[4], m11 = m[5], m12 = m[6], m13 = m[7];
  const float m20 = m[8], m21 = m[9], m22 = m[10], m23 = m[11];
  const float m30 = m[12], m31 = m[13], m32 = m[14], m33 = m[15];
  r[0] = m12 * m23 * m31 - m13 * m22 * m31 + m13 * m21 * m32 - m11 * m23 * m32 - m12 * m21 * m33 + m11 * m22 * m33;
  r[1] = m03 * m22 * m31 - m02 * m23 * m31 - m03 * m21 * m32 + m01 * m23 * m32 + m02 * m21 * m33 - m01 * m22 * m33;
  r[2] = m02 * m13 * m31 - m03 * m12 * m31 + m03 * m11 * m32 - m01 * m13 * m32 - m02 * m11 * m33 + m01 * m12 * m33;
  r[3] = m03 * m12 * m21 - m02 * m13 * m21 - m03 * m11 * m22 + m01 * m13 * m22 + m02 * m11 * m23 - m01 * m12 * m23;
  r[4] = m13 * m22 * m30 - m12 * m23 * m30 - m13 * m20 * m32 + m10 * m23 * m32 + m12 * m20 * m33 - m10 * m22 * m33;
  r[5] = m02 * m23 * m30 - m03 * m22 * m30 + m03 * m20 * m32 - m00 * m23 * m32 - m02 * m20 * m33 + m00 * m22 * m33;
  r[6] = m03 * m12 * m30 - m02 * m13 * m30 - m03 * m10 * m32 + m00 * m13 * m32 + m02 * m10 * m33 - m00 * m12 * m33;
  r[7] = m02 * m13 * m20 - m03 * m12 * m20 + m03 * m10 * m22 - m00 * m13 * m22 - m02 * m10 * m23 + m00 * m12 * m23;
  r[8] = m11 * m23 * m30 - m13 * m21 * m30 + m13 * m20 * m31 - m10 * m23 * m31 - m11 * m20 * m33 + m10 * m21 * m33;
  r[9] = m03 * m21 * m30 - m01 * m23 * m30 - m03 * m20 * m31 + m00 * m23 * m31 + m01 * m20 * m33 - m00 * m21 * m33;
  r[10] = m01 * m13 * m30 - m03 * m11 * m30 + m03 * m10 * m31 - m00 * m13 * m31 - m01 * m10 * m33 + m00 * m11 * m33;
  r[11] = m03 * m11 * m20 - m01 * m13 * m20 - m03 * m10 * m21 + m00 * m13 * m21 + m01 * m10 * m23 - m00 * m11 * m23;
  r[12] = m12 * m21 * m30 - m11 * m22 * m30 - m12 * m20 * m31 + m10 * m22 * m31 + m11 * m20 * m32 - m10 * m21 * m32;
  r[13] = m01 * m22 * m30 - m02 * m21 * m30 + m02 * m20 * m31 - m00 * m22 * m31 - m01 * m20 * m32 + m00 * m21 * m32;
  r[14] = m02 * m11 * m30 - m01 * m12 * m30 - m02 * m10 * m31 + m00 * m12 * m31 + m01 * m10 * m32 - m00 * m11 * m32;
  r[15] = m01 * m12 * m20 - m02 * m11 * m20 + m02 * m10 * m21 - m00 * m12 * m21 - m01 * m10 * m22 + m00 * m11 * m22;
  const float det = m03 * m12 * m21 * m30 - m02 * m13 * m21 * m30 - m03 * m11 * m22 * m30 + m01 * m13 * m22 * m30 + m02 * m11 * m23 * m30
                   - m01 * m12 * m23 * m30 - m03 * m12 * m20 * m31 + m02 * m13 * m20 * m31 + m03 * m10 * m22 * m31 - m00 * m13 * m22 * m31
                   - m02 * m10 * m23 * m31 + m00 * m12 * m23 * m31 + m03 * m11 * m20 * m32 - m01 * m13 * m20 * m32 - m03 * m10 * m21 * m32
                   + m00 * m13 * m21 * m32 + m01 * m10 * m23 * m32 - m00 * m11 * m23 * m32 - m02 * m11 * m20 * m33 + m01 * m12 * m20 * m33
                   + m02 * m10 * m21 * m33 - m00 * m12 * m21 * m33 - m01 * m10 * m22 * m33 + m00 * m11 * m22 * m33;
  for (int e = 0; e < 16; e++) r[e] = r[e] / det;
}

// Mat4::operator!= against the identity: a value compare, so -0.0f equals 0.0f and a NaN entry differs.
__device__ __forceinline__ bool pose_ne_identity(const float m[16]) {
  bool ne = false;
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++)
      if (m[4 * c + r] != (c == r ? 1.0f : 0.0f)) ne = true;
  return ne;
}

// BBox::transform (lib/bbox.h:57-73) as Box::transform of pt_scene.cpp states it, applied to box6 = {mn[3], mx[3]} in place.
__device__ __forceinline__ void pose_box(const float t[16], float box6[6]) {
  float amin[3], amax[3];
  for (int i = 0; i < 3; i++) { amin[i] = box6[i]; amax[i] = box6[3 + i]; box6[i] = box6[3 + i] = t[12 + i]; }
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const float a = t[4 * j + i] * amin[j], b = t[4 * j + i] * amax[j];
      if (a < b) { box6[i] += a; box6[3 + i] += b; } else { box6[i] += b; box6[3 + i] += a; }
    }
}

// Mat4::translate(pos) * Mat4::scale(Vec3{scale}) through Mat4::operator* (lib/mat4.h:136-147) as mat_mul(translate, scale) forms
// it: every element a sum of four products accumulated from 0.0f - which is what decides the sign of the zeros.
__device__ __forceinline__ void pose_translate_scale(const float pos[3], float scale, float out[16]) {
  float T[16], S[16];
  for (int e = 0; e < 16; e++) T[e] = S[e] = (e % 5 == 0) ? 1.0f : 0.0f;
  T[12] = pos[0]; T[13] = pos[1]; T[14] = pos[2];
  S[0] = S[5] = S[10] = scale;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.0f;
      for (int k = 0; k < 4; k++) acc += S[4 * i + k] * T[4 * k + j];
      out[4 * i + j] = acc;
    }
}

// What srt_pt_repose_device reads back per listed object (156 B): the values the host's record of the scene takes as they are.
struct PoseOut {
  float trans[16], itrans[16];
  uint32_t has_trans;
  float box[6];
};
static_assert(sizeof(PoseOut) == 156, "pose read-back layout");

// One listed object: its new transform, its object-space box -> the record of what the pose decides.
__device__ __forceinline__ void pose_object(const float trans[16], const float local_box6[6], PoseOut* out) {
  for (int e = 0; e < 16; e++) out->trans[e] = trans[e];
  pose_inverse(trans, out->itrans);
  const bool ne = pose_ne_identity(trans);
  out->has_trans = ne ? 1u : 0u;
  for (int a = 0; a < 6; a++) out->box[a] = local_box6[a];
  if (ne) pose_box(trans, out->box);              // Object::bbox poses the box only when has_trans
}

// ---- launchers (pt_pose.hip); every one only enqueues on `stream` ----
// The committed records (object order) as a table by insertion index, without what follows object order: use_bvh keeps bit 0
// only and node_base counts from the end of the BVH<Object>'s nodes.  Then every object's posed box from its object-space box.
void launch_pose_tables(void* stream, const Object* d_objects, uint32_t nobj, uint32_t tlas_nodes, Object* d_by_index, const float* d_local_boxes6,
                        float* d_posed_boxes6);
// One lane per listed object k < n: d_trans[16 k ..] and the object-space box of object d_listed[k] -> d_out[k], the matrices and
// has_trans of d_by_index[d_listed[k]], d_posed_boxes6[6 d_listed[k] ..].  Nothing a render kernel reads.
void launch_pose_objects(void* stream, const uint32_t* d_listed, const float* d_trans, uint32_t n, uint32_t nobj, const float* d_local_boxes6,
                         PoseOut* d_out, Object* d_by_index, float* d_posed_boxes6);
// The live records, in place: slot k takes the record of object d_prim[k] (k itself when NULL), its node_base counted from
// tlas_nodes again and its mesh ordinal d_ordinal[k] (already shifted to bits 8 and up; none when NULL).
void launch_pose_records(void* stream, const Object* d_by_index, const uint32_t* d_prim, const uint32_t* d_ordinal, uint32_t nobj, uint32_t tlas_nodes,
                         Object* d_objects);
// srt_pt_repose_refit_device: d_slot_of[d_prim[slot]] = slot for the nobj slots of the BVH<Object>'s primitive order (made once per tree,
// on the device: nothing goes up for it).
void launch_top_slots(void* stream, const uint32_t* d_prim, uint32_t nobj, uint32_t* d_slot_of);
// The n listed objects' trans, itrans and has_trans from d_by_index (where launch_pose_objects left them) into their live records
// d_objects[d_slot_of[i]] (slot i when d_slot_of is NULL: a list scene).  Copies only; no other field of a live record is written.
void launch_top_objects(void* stream, const uint32_t* d_listed, uint32_t n, uint32_t nobj, const uint32_t* d_slot_of, const Object* d_by_index,
                        Object* d_objects);
// srt_pt_set_active_device: d_table[d_listed[k]] = d_flags[k] != 0 for k < n - the table holds one byte per object by insertion index
// (nobj of them), which the leaf stage of the BVH<Object>'s refit takes as its mask (launch_refit_boxes, pt_bvh_device.h).
void launch_active_scatter(void* stream, const uint32_t* d_listed, const uint8_t* d_flags, uint32_t n, uint32_t nobj, uint8_t* d_table);
// Behind it, and behind the refit's box stages: the count a leaf of the BVH<Object> holds for the walks - the count word of the live
// top-level nodes and the l_cnt / r_cnt of the live sweep records - 0 while every object of the leaf is inactive (two launches: leaves,
// then records).  T: the BVH<Object>'s refit tables.
struct RefitTables;
void launch_top_counts(void* stream, const RefitTables& T, const uint8_t* d_table, uint32_t nobj, Node* d_nodes, WaveInterior* d_wave);
// srt_pt_refit_mesh_inplace_device: one lane per member k < n of a refitted mesh's family (d_family: the mesh and its instances, by
// insertion index).  Node 0 of d_node_boxes6 (the mesh's refitted boxes) -> d_local_boxes6[6 i ..], and its Object::bbox under the
// unchanged transform of d_by_index[i] -> d_posed_boxes6[6 i ..].  Nothing a render kernel reads; the top-level refit's stages follow.
void launch_mesh_link(void* stream, const uint32_t* d_family, uint32_t n, uint32_t nobj, const float* d_node_boxes6, const Object* d_by_index,
                      float* d_local_boxes6, float* d_posed_boxes6);
// One lane per particle: d_trans_out[16 k ..] = translate(d_pos[3 k ..]) * scale(scale).
void launch_particle_transforms(void* stream, const float* d_pos, uint32_t n, float scale, float* d_trans_out);

}  // namespace srt

#endif
