// Skeleton::find_joints and Skeleton::skin (student/skeleton.cpp:195-307) and the flat-normal loop of Scene_Object::sync_anim_mesh
// (scene/object.cpp:114-126) as device functions: the capsule test of one (vertex, joint) pair, a vertex's influence list and
// weights, a vertex's skinned position, a triangle's unit normal.  pt_skin.hip runs them one lane per vertex; the host emulation
// (tests/host_emu/skin_host.cpp) compiles this header with g++ -ffp-contract=off and compares with results recorded from the
// reference.  Every function restates the reference operation for operation - one rounding per operator, sums in the order the
// reference's expressions associate, divisions and square roots correctly rounded (hipcc's default, as for Triangle::hit) - and
// the library is built without contraction, so the results equal the reference's bit for bit.  The two matrix routines the host
// runs once per joint (Mat4::inverse, Mat4::operator*) are in here too, for the same two compilers.
//
// Matrices are Mat4::data: 16 floats, column-major, m[4 * c + r] = cols[c][r].
#ifndef SRT_PT_SKIN_H
#define SRT_PT_SKIN_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace srt {

// Limits of srt_pt_skin_create (SRT_ERR_UNSUPPORTED beyond them): the joint matrices of a skin are meant to stay L2-resident
// (4096 * 64 B = 256 KiB), and vertex * joint pairs - the bound of the influence count - fit the 32-bit offsets of the map.
constexpr uint32_t kSkinMaxJoints = 4096;
constexpr uint64_t kSkinMaxPairs = 1ull << 31;

struct SkinV3 { float x, y, z; };

// Mat4::inverse (lib/mat4.h:299-351): the sixteen cofactor sums as written there, then `r /= m.det()` - sixteen divisions by the
// brute-force determinant (:211-236), not a multiplication by its reciprocal.  NaN / inf when m is singular, as in the reference.
inline void skin_mat4_inverse(const float* m, float* r) {
#define M(c, k) m[4 * (c) + (k)]
  r[0] = M(1, 2) * M(2, 3) * M(3, 1) - M(1, 3) * M(2, 2) * M(3, 1) + M(1, 3) * M(2, 1) * M(3, 2) - M(1, 1) * M(2, 3) * M(3, 2) - M(1, 2) * M(2, 1) * M(3, 3) + M(1, 1) * M(2, 2) * M(3, 3);
  r[1] = M(0, 3) * M(2, 2) * M(3, 1) - M(0, 2) * M(2, 3) * M(3, 1) - M(0, 3) * M(2, 1) * M(3, 2) + M(0, 1) * M(2, 3) * M(3, 2) + M(0, 2) * M(2, 1) * M(3, 3) - M(0, 1) * M(2, 2) * M(3, 3);
  r[2] = M(0, 2) * M(1, 3) * M(3, 1) - M(0, 3) * M(1, 2) * M(3, 1) + M(0, 3) * M(1, 1) * M(3, 2) - M(0, 1) * M(1, 3) * M(3, 2) - M(0, 2) * M(1, 1) * M(3, 3) + M(0, 1) * M(1, 2) * M(3, 3);
  r[3] = M(0, 3) * M(1, 2) * M(2, 1) - M(0, 2) * M(1, 3) * M(2, 1) - M(0, 3) * M(1, 1) * M(2, 2) + M(0, 1) * M(1, 3) * M(2, 2) + M(0, 2) * M(1, 1) * M(2, 3) - M(0, 1) * M(1, 2) * M(2, 3);
  r[4] = M(1, 3) * M(2, 2) * M(3, 0) - M(1, 2) * M(2, 3) * M(3, 0) - M(1, 3) * M(2, 0) * M(3, 2) + M(1, 0) * M(2, 3) * M(3, 2) + M(1, 2) * M(2, 0) * M(3, 3) - M(1, 0) * M(2, 2) * M(3, 3);
  r[5] = M(0, 2) * M(2, 3) * M(3, 0) - M(0, 3) * M(2, 2) * M(3, 0) + M(0, 3) * M(2, 0) * M(3, 2) - M(0, 0) * M(2, 3) * M(3, 2) - M(0, 2) * M(2, 0) * M(3, 3) + M(0, 0) * M(2, 2) * M(3, 3);
  r[6] = M(0, 3) * M(1, 2) * M(3, 0) - M(0, 2) * M(1, 3) * M(3, 0) - M(0, 3) * M(1, 0) * M(3, 2) + M(0, 0) * M(1, 3) * M(3, 2) + M(0, 2) * M(1, 0) * M(3, 3) - M(0, 0) * M(1, 2) * M(3, 3);
  r[7] = M(0, 2) * M(1, 3) * M(2, 0) - M(0, 3) * M(1, 2) * M(2, 0) + M(0, 3) * M(1, 0) * M(2, 2) - M(0, 0) * M(1, 3) * M(2, 2) - M(0, 2) * M(1, 0) * M(2, 3) + M(0, 0) * M(1, 2) * M(2, 3);
  r[8] = M(1, 1) * M(2, 3) * M(3, 0) - M(1, 3) * M(2, 1) * M(3, 0) + M(1, 3) * M(2, 0) * M(3, 1) - M(1, 0) * M(2, 3) * M(3, 1) - M(1, 1) * M(2, 0) * M(3, 3) + M(1, 0) * M(2, 1) * M(3, 3);
  r[9] = M(0, 3) * M(2, 1) * M(3, 0) - M(0, 1) * M(2, 3) * M(3, 0) - M(0, 3) * M(2, 0) * M(3, 1) + M(0, 0) * M(2, 3) * M(3, 1) + M(0, 1) * M(2, 0) * M(3, 3) - M(0, 0) * M(2, 1) * M(3, 3);
  r[10] = M(0, 1) * M(1, 3) * M(3, 0) - M(0, 3) * M(1, 1) * M(3, 0) + M(0, 3) * M(1, 0) * M(3, 1) - M(0, 0) * M(1, 3) * M(3, 1) - M(0, 1) * M(1, 0) * M(3, 3) + M(0, 0) * M(1, 1) * M(3, 3);
  r[11] = M(0, 3) * M(1, 1) * M(2, 0) - M(0, 1) * M(1, 3) * M(2, 0) - M(0, 3) * M(1, 0) * M(2, 1) + M(0, 0) * M(1, 3) * M(2, 1) + M(0, 1) * M(1, 0) * M(2, 3) - M(0, 0) * M(1, 1) * M(2, 3);
  r[12] = M(1, 2) * M(2, 1) * M(3, 0) - M(1, 1) * M(2, 2) * M(3, 0) - M(1, 2) * M(2, 0) * M(3, 1) + M(1, 0) * M(2, 2) * M(3, 1) + M(1, 1) * M(2, 0) * M(3, 2) - M(1, 0) * M(2, 1) * M(3, 2);
  r[13] = M(0, 1) * M(2, 2) * M(3, 0) - M(0, 2) * M(2, 1) * M(3, 0) + M(0, 2) * M(2, 0) * M(3, 1) - M(0, 0) * M(2, 2) * M(3, 1) - M(0, 1) * M(2, 0) * M(3, 2) + M(0, 0) * M(2, 1) * M(3, 2);
  r[14] = M(0, 2) * M(1, 1) * M(3, 0) - M(0, 1) * M(1, 2) * M(3, 0) - M(0, 2) * M(1, 0) * M(3, 1) + M(0, 0) * M(1, 2) * M(3, 1) + M(0, 1) * M(1, 0) * M(3, 2) - M(0, 0) * M(1, 1) * M(3, 2);
  r[15] = M(0, 1) * M(1, 2) * M(2, 0) - M(0, 2) * M(1, 1) * M(2, 0) + M(0, 2) * M(1, 0) * M(2, 1) - M(0, 0) * M(1, 2) * M(2, 1) - M(0, 1) * M(1, 0) * M(2, 2) + M(0, 0) * M(1, 1) * M(2, 2);
  const float det = M(0, 3) * M(1, 2) * M(2, 1) * M(3, 0)
                   - M(0, 2) * M(1, 3) * M(2, 1) * M(3, 0) - M(0, 3) * M(1, 1) * M(2, 2) * M(3, 0)
                   + M(0, 1) * M(1, 3) * M(2, 2) * M(3, 0) + M(0, 2) * M(1, 1) * M(2, 3) * M(3, 0)
                   - M(0, 1) * M(1, 2) * M(2, 3) * M(3, 0) - M(0, 3) * M(1, 2) * M(2, 0) * M(3, 1)
                   + M(0, 2) * M(1, 3) * M(2, 0) * M(3, 1) + M(0, 3) * M(1, 0) * M(2, 2) * M(3, 1)
                   - M(0, 0) * M(1, 3) * M(2, 2) * M(3, 1) - M(0, 2) * M(1, 0) * M(2, 3) * M(3, 1)
                   + M(0, 0) * M(1, 2) * M(2, 3) * M(3, 1) + M(0, 3) * M(1, 1) * M(2, 0) * M(3, 2)
                   - M(0, 1) * M(1, 3) * M(2, 0) * M(3, 2) - M(0, 3) * M(1, 0) * M(2, 1) * M(3, 2)
                   + M(0, 0) * M(1, 3) * M(2, 1) * M(3, 2) + M(0, 1) * M(1, 0) * M(2, 3) * M(3, 2)
                   - M(0, 0) * M(1, 1) * M(2, 3) * M(3, 2) - M(0, 2) * M(1, 1) * M(2, 0) * M(3, 3)
                   + M(0, 1) * M(1, 2) * M(2, 0) * M(3, 3) + M(0, 2) * M(1, 0) * M(2, 1) * M(3, 3)
                   - M(0, 0) * M(1, 2) * M(2, 1) * M(3, 3) - M(0, 1) * M(1, 0) * M(2, 2) * M(3, 3)
                   + M(0, 0) * M(1, 1) * M(2, 2) * M(3, 3);
#undef M
  for (int i = 0; i < 16; i++) r[i] /= det;
}

// Mat4::operator* (lib/mat4.h:136-147), ret = a * b: ret[i][j] = sum over k, from 0.0f, of b[i][k] * a[k][j] - the loop runs
// over the RIGHT operand's column i and the left operand's row j.
__host__ __device__ inline void skin_mat4_mul(const float* a, const float* b, float* ret) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float s = 0.0f;
      for (int k = 0; k < 4; k++) s += b[4 * i + k] * a[4 * k + j];
      ret[4 * i + j] = s;
    }
}

// Mat4 * Vec3 (lib/mat4.h:149-156): v0 * col0 + v1 * col1 + v2 * col2 + 1.0f * col3, then Vec4::project - three divisions by w.
__device__ __forceinline__ SkinV3 skin_mat_point(const float* __restrict__ m, SkinV3 p) {
  float r[4];
  for (int a = 0; a < 4; a++) r[a] = ((p.x * m[a] + p.y * m[4 + a]) + p.z * m[8 + a]) + 1.0f * m[12 + a];
  return {r[0] / r[3], r[1] / r[3], r[2] / r[3]};
}

__device__ __forceinline__ float skin_dot(SkinV3 l, SkinV3 r) { return (l.x * r.x + l.y * r.y) + l.z * r.z; }
__device__ __forceinline__ float skin_norm(SkinV3 v) { return sqrtf(skin_dot(v, v)); }
__device__ __forceinline__ SkinV3 skin_sub(SkinV3 l, SkinV3 r) { return {l.x - r.x, l.y - r.y, l.z - r.z}; }

// closest_on_line_segment (student/skeleton.cpp:195-217) as written: `<= 0` returns start; the projection is
// ((dot / norm) * v) / norm; the end test compares squared norms; and the last return is proj, NOT start + proj.
__device__ __forceinline__ SkinV3 skin_closest_on_line_segment(SkinV3 start, SkinV3 end, SkinV3 point) {
  const SkinV3 start_p = skin_sub(point, start);
  const SkinV3 start_end = skin_sub(end, start);
  const float d = skin_dot(start_p, start_end);
  if (d <= 0) return start;
  const float n = skin_norm(start_end);
  const float s = d / n;
  const SkinV3 proj = {(start_end.x * s) / n, (start_end.y * s) / n, (start_end.z * s) / n};
  if (skin_dot(proj, proj) > skin_dot(start_end, start_end)) return end;
  return proj;
}

// The distance find_joints compares with Joint::radius (:237-241) and skin inverts (:286-290): the vertex through the inverse
// bind matrix into joint space, the closest point on the bone from Vec3{0} to Vec3{0} + extent, the norm of the difference.
// (skin subtracts the other way round; the norm of a vector and of its negation are the same float.)
__device__ __forceinline__ float skin_bone_distance(const float* __restrict__ inv, const float* __restrict__ extent, SkinV3 pos) {
  const SkinV3 p = skin_mat_point(inv, pos);
  const SkinV3 zero = {0.0f, 0.0f, 0.0f};
  const SkinV3 end = {0.0f + extent[0], 0.0f + extent[1], 0.0f + extent[2]};
  return skin_norm(skin_sub(p, skin_closest_on_line_segment(zero, end, p)));
}

// find_joints for one vertex, counting pass: how many joints' capsules hold it.  inv: njoints * 16; cap: njoints * 4 =
// {extent, radius}.  Every lane of a wave reads the same joint, so the joint data come through scalar loads.
__device__ __forceinline__ uint32_t skin_count_joints(const float* __restrict__ inv, const float* __restrict__ cap, uint32_t njoints, SkinV3 pos) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < njoints; j++)
    if (skin_bone_distance(inv + 16 * (size_t)j, cap + 4 * (size_t)j, pos) <= cap[4 * (size_t)j + 3]) c++;
  return c;
}

// find_joints for one vertex, filling pass: the joints in ascending index into jidx[begin, end) and skin's weights (:280-299),
// which do not depend on the pose, into w[begin, end): inv_dist = 1.0f / distance, summed from 0.0f in list order, then
// inv_dist / sum.  end - begin is what skin_count_joints returned; nothing is written outside the range whatever it is.
__device__ __forceinline__ void skin_fill_joints(const float* __restrict__ inv, const float* __restrict__ cap, uint32_t njoints, SkinV3 pos,
                                                 uint32_t begin, uint32_t end, uint32_t* jidx, float* w) {
  uint32_t k = begin;
  float sum_of_inv_dis = 0.0f;
  for (uint32_t j = 0; j < njoints && k < end; j++) {
    const float d = skin_bone_distance(inv + 16 * (size_t)j, cap + 4 * (size_t)j, pos);
    if (d <= cap[4 * (size_t)j + 3]) {
      const float inv_dist = 1.0f / d;
      jidx[k] = j;
      w[k] = inv_dist;
      sum_of_inv_dis += inv_dist;
      k++;
    }
  }
  for (uint32_t q = begin; q < k; q++) w[q] = w[q] / sum_of_inv_dis;
}

// skin for one vertex (:293-302): sum, from Vec3{0} in list order, of w_ij * (M_j * pos) with M_j = joint_to_posed(j) *
// inverse(joint_to_bind(j)) formed on the host; a vertex without joints keeps its bind position.
__device__ __forceinline__ SkinV3 skin_vertex(const float* __restrict__ mats, const uint32_t* __restrict__ off, const uint32_t* __restrict__ jidx,
                                              const float* __restrict__ w, uint32_t njoints, SkinV3 pos, uint32_t v) {
  const uint32_t begin = off[v], end = off[v + 1];
  if (begin == end) return pos;
  SkinV3 sum = {0.0f, 0.0f, 0.0f};
  for (uint32_t k = begin; k < end; k++) {
    const uint32_t j = jidx[k];
    if (j >= njoints) continue;   // (never, by construction: no address outside the matrices)
    const SkinV3 p = skin_mat_point(mats + 16 * (size_t)j, pos);
    const float wk = w[k];
    sum.x += p.x * wk;
    sum.y += p.y * wk;
    sum.z += p.z * wk;
  }
  return sum;
}

// cross(v1 - v0, v2 - v0).unit() of triangle t (scene/object.cpp:118-121); NaN for a degenerate triangle, as there.
__device__ __forceinline__ SkinV3 skin_flat_normal(const float* __restrict__ pos, const uint32_t* __restrict__ idx, uint32_t t) {
  const float* p0 = pos + 3 * (size_t)idx[3 * (size_t)t];
  const float* p1 = pos + 3 * (size_t)idx[3 * (size_t)t + 1];
  const float* p2 = pos + 3 * (size_t)idx[3 * (size_t)t + 2];
  const SkinV3 l = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const SkinV3 r = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
  const SkinV3 c = {l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x};
  const float n = skin_norm(c);
  return {c.x / n, c.y / n, c.z / n};
}

// The launches of pt_skin.hip.  Plain pointers; `stream` is a hipStream_t; every call only enqueues.
// find_joints: counts[v]; then the exclusive scan of counts into off[0, nverts] (sums: one word per 256 vertices); then the lists
// and weights.  The caller reads off[nverts] between the scan and the fill to size jidx / w.
void launch_skin_count(void* stream, const float* d_pos, uint32_t nverts, const float* d_inv, const float* d_cap, uint32_t njoints, uint32_t* d_counts);
void launch_skin_scan(void* stream, const uint32_t* d_counts, uint32_t nverts, uint32_t* d_off, uint32_t* d_sums);
void launch_skin_fill(void* stream, const float* d_pos, uint32_t nverts, const float* d_inv, const float* d_cap, uint32_t njoints, const uint32_t* d_off,
                      uint32_t* d_jidx, float* d_w);
// d_last[v] = 1 + the last triangle in index order that names vertex v, 0 when none does (d_last zeroed by the caller on the stream)
void launch_skin_last_triangle(void* stream, const uint32_t* d_idx, uint32_t ntri, uint32_t nverts, uint32_t* d_last);
// skin: d_pos_out[v]; with d_nrm_out, the bind normals are copied along (flat_normals == 0)
void launch_skin_vertices(void* stream, const float* d_pos, const float* d_nrm, uint32_t nverts, const float* d_mats, uint32_t njoints, const uint32_t* d_off,
                          const uint32_t* d_jidx, const float* d_w, float* d_pos_out, float* d_nrm_out);
// the flat normals of the skinned positions: one lane per vertex, from the triangle d_last names
void launch_skin_flat_normals(void* stream, const float* d_pos_out, const float* d_nrm, const uint32_t* d_idx, uint32_t ntri, const uint32_t* d_last,
                              uint32_t nverts, float* d_nrm_out);

}  // namespace srt

#endif
