// The Animate mode's timeline as functions for the device and the host: Spline<Vec3>::at and cubic_unit_spline
// (student/spline.inl:5-72), Spline<Quat>::at (geometry/spline.inl:4-15) with slerp (lib/quat.h:177-189), Quat::to_euler
// (lib/quat.h:124-135, lib/mat4.h:163-199), Mat4::euler / rotate / translate / scale (lib/mat4.h:382-418), Pose::transform
// (scene/pose.cpp:4-10), Anim_Pose::at (:54-57) and Joint::joint_to_posed (student/skeleton.cpp:26-52) under
// Skeleton::joint_to_posed (:106-115).  pt_anim.hip runs them one lane per object or joint; the pt_update_*.cpp units run the same functions on
// the host (srt_pt_timeline_transforms, srt_pt_skin_posed: the definition the kernels are held to) and the host emulation
// (tests/host_emu/anim_host.cpp) compiles this header with g++ -ffp-contract=off.  Every function restates the reference
// operation for operation - one rounding per operator, sums in the order the reference's expressions associate, true divisions -
// and nothing is built with contraction, so the results equal the reference's bit for bit; where the reference yields NaN (a zero
// quaternion) so do these, up to the NaN's sign and payload.
//
// Transcendentals are SRT-MATH v2 (pt_device.h): srt_sincosf2, srt_acosf, srt_atan2f, and srt_hypotf below.  The sin / cos
// restatement is valid for |x| < 120 radians - Euler angles below 6875 degrees - and returns NaN beyond, where libm returns a
// value; to_euler yields angles within +-180 degrees, so only a caller's rest pose can be out of range.  Nothing is refused on
// that account.
//
// Matrices are Mat4::data: 16 floats, column-major, m[4 * c + r] = cols[c][r].  Knot tables are CSR: times[k] ascending inside a
// track, values[4 k ..] = xyz_ (Vec3) or xyzw (Quat).
#ifndef SRT_PT_ANIM_H
#define SRT_PT_ANIM_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "pt_device.h"
#include "pt_scene.h"
#include "pt_skin.h"

namespace srt {

#define SRT_ANIM_FN __host__ __device__ inline

struct AnimV3 { float x, y, z; };
struct AnimQ { float x, y, z, w; };

// SRT-MATH v2, hypotf: glibc 2.35 __hypotf (sysdeps/ieee754/flt-32/e_hypotf.c): infinities first, then
// (float)sqrt((double)x * x + (double)y * y) - the products are exact, the sum and the root round once each in fp64, the narrowing
// once more.  Bit-identical to the host libm (tests/test_pt_anim_host.py).
SRT_ANIM_FN float srt_hypotf(float x, float y) {
  const uint32_t ax = f2u(x) & 0x7fffffffu, ay = f2u(y) & 0x7fffffffu;
  if (ax >= 0x7f800000u || ay >= 0x7f800000u) {
    const bool sx = ax > 0x7f800000u && !(ax & 0x00400000u), sy = ay > 0x7f800000u && !(ay & 0x00400000u);   // issignaling
    if ((ax == 0x7f800000u || ay == 0x7f800000u) && !sx && !sy) return u2f(0x7f800000u);
    return x + y;
  }
  return (float)sqrt((double)x * (double)x + (double)y * (double)y);
}

SRT_ANIM_FN AnimV3 anim_v3(const float* p) { return {p[0], p[1], p[2]}; }
SRT_ANIM_FN AnimV3 operator+(AnimV3 a, AnimV3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
SRT_ANIM_FN AnimV3 operator-(AnimV3 a, AnimV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
SRT_ANIM_FN AnimV3 operator*(AnimV3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }       // Vec3 * float and float * Vec3
SRT_ANIM_FN AnimV3 operator/(AnimV3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }       // three true divisions

// std::map<float, T>::upper_bound over times[lo, hi): the first knot whose time is greater than `time`, hi when there is none (a NaN `time` included).
SRT_ANIM_FN uint32_t anim_upper_bound(const float* times, uint32_t lo, uint32_t hi, float time) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (time < times[mid]) hi = mid; else lo = mid + 1u;
  }
  return lo;
}

// Spline<Vec3>::cubic_unit_spline (student/spline.inl:5-22)
SRT_ANIM_FN AnimV3 anim_cubic_unit_spline(float time, AnimV3 position0, AnimV3 position1, AnimV3 tangent0, AnimV3 tangent1) {
  const float t_squared = time * time;
  const float t_cubic = t_squared * time;
  const float h00 = (2.0f * t_cubic - 3.0f * t_squared) + 1.0f;
  const float h10 = (t_cubic - 2.0f * t_squared) + time;
  const float h01 = -2.0f * t_cubic + 3.0f * t_squared;
  const float h11 = t_cubic - t_squared;
  return ((position0 * h00 + tangent0 * h10) + position1 * h01) + tangent1 * h11;
}

// Spline<Vec3>::at (:24-72) over the knots [b, e) of the tables, as the fork wrote it: T() without knots, the one value of one knot,
// the end values at and beyond the ends, a missing k0 / k3 mirrored in time and value.
SRT_ANIM_FN AnimV3 anim_spline_vec3(const float* times, const float* values, uint32_t b, uint32_t e, float time) {
  if (e <= b) return {0.0f, 0.0f, 0.0f};
  if (e - b == 1u) return anim_v3(values + 4 * (size_t)b);
  if (time <= times[b]) return anim_v3(values + 4 * (size_t)b);
  if (time >= times[e - 1u]) return anim_v3(values + 4 * (size_t)(e - 1u));
  const uint32_t k2 = anim_upper_bound(times, b, e, time);
  if (k2 == b) return anim_v3(values + 4 * (size_t)b);              // (never: time > times[b] here; kept as the restatement of student/spline.inl:43)
  if (k2 == e) return anim_v3(values + 4 * (size_t)(e - 1u));       // (a NaN time)
  const uint32_t k1 = k2 - 1u;
  const bool has_k3 = k2 != e - 1u, has_k0 = k1 != b;
  const float t1 = times[k1], t2 = times[k2];
  const AnimV3 p1 = anim_v3(values + 4 * (size_t)k1), p2 = anim_v3(values + 4 * (size_t)k2);
  const float t0 = has_k0 ? times[k1 - 1u] : (t1 - (t2 - t1));
  const AnimV3 p0 = has_k0 ? anim_v3(values + 4 * (size_t)(k1 - 1u)) : (p1 - (p2 - p1));
  const float t3 = has_k3 ? times[k2 + 1u] : (t2 + (t2 - t1));
  const AnimV3 p3 = has_k3 ? anim_v3(values + 4 * (size_t)(k2 + 1u)) : (p2 + (p2 - p1));
  const float interval = t2 - t1;
  const AnimV3 m1 = ((p2 - p0) / (t2 - t0)) * interval;
  const AnimV3 m2 = ((p3 - p1) / (t3 - t1)) * interval;
  const float t_normalized = (time - t1) / interval;
  return anim_cubic_unit_spline(t_normalized, p1, p2, m1, m2);
}

SRT_ANIM_FN AnimQ anim_q(const float* p) { return {p[0], p[1], p[2], p[3]}; }
SRT_ANIM_FN AnimQ anim_q_scale(float s, AnimQ q) { return {s * q.x, s * q.y, s * q.z, s * q.w}; }
SRT_ANIM_FN AnimQ anim_q_add(AnimQ a, AnimQ b) { return {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// slerp (lib/quat.h:177-189): q0 flipped when the dot is negative, the lerp at |dot| >= 1.0f - EPS_F, otherwise acos of |dot|,
// two sines and a multiplication by 1.0f / sin(a).
SRT_ANIM_FN AnimQ anim_slerp(AnimQ q0, AnimQ q1, float t) {
  const float hcos = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
  const AnimQ shortest = hcos < 0 ? AnimQ{-q0.x, -q0.y, -q0.z, -q0.w} : q0;
  if (fabsf(hcos) >= 1.0f - kEps) return anim_q_add(anim_q_scale(1.0f - t, shortest), anim_q_scale(t, q1));
  const float a = srt_acosf(fabsf(hcos));
  const float s0 = srt_sincosf((1.0f - t) * a, 0), s1 = srt_sincosf(t * a, 0);
  return anim_q_scale(1.0f / srt_sincosf(a, 0), anim_q_add(anim_q_scale(s0, shortest), anim_q_scale(s1, q1)));
}

// Spline<Quat>::at (geometry/spline.inl:4-15): Quat() without knots; the strict test before the first knot; the last value from
// the last knot on.
SRT_ANIM_FN AnimQ anim_spline_quat(const float* times, const float* values, uint32_t b, uint32_t e, float time) {
  if (e <= b) return {0.0f, 0.0f, 0.0f, 1.0f};
  if (e - b == 1u) return anim_q(values + 4 * (size_t)b);
  if (times[b] > time) return anim_q(values + 4 * (size_t)b);
  const uint32_t k2 = anim_upper_bound(times, b, e, time);
  if (k2 == e) return anim_q(values + 4 * (size_t)(e - 1u));
  // (k2 > b: times[b] <= time here, and a NaN time has gone to k2 == e)
  const uint32_t k1 = k2 - 1u;
  const float t = (time - times[k1]) / (times[k2] - times[k1]);
  return anim_slerp(anim_q(values + 4 * (size_t)k1), anim_q(values + 4 * (size_t)k2), t);
}

// Quat::to_euler = unit().to_mat().to_euler() (lib/quat.h:100-135, lib/mat4.h:163-199), in degrees.
SRT_HD AnimV3 anim_quat_to_euler(AnimQ q) {
  const float n = sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w);
  const float x = q.x / n, y = q.y / n, z = q.z / n, w = q.w / n;
  float c[3][4];
  c[0][0] = (1 - 2 * y * y) - 2 * z * z; c[0][1] = 2 * x * y + 2 * z * w;     c[0][2] = 2 * x * z - 2 * y * w;     c[0][3] = 0.0f;
  c[1][0] = 2 * x * y - 2 * z * w;     c[1][1] = (1 - 2 * x * x) - 2 * z * z; c[1][2] = 2 * y * z + 2 * x * w;     c[1][3] = 0.0f;
  c[2][0] = 2 * x * z + 2 * y * w;     c[2][1] = 2 * y * z - 2 * x * w;     c[2][2] = (1 - 2 * x * x) - 2 * y * y; c[2][3] = 0.0f;
  const float singularity[12] = {1.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
  bool single = true;                                                // (the reference's loops stop at the first failure; the verdict is the same)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) single = single && fabsf(c[i][j] - singularity[i * 4 + j]) < kEps;
  if (single) return {0.0f, 0.0f, 180.0f};
  float e1[3], e2[3];
  const float cy = srt_hypotf(c[0][0], c[0][1]);
  if (cy > kEps) {
    e1[0] = srt_atan2f(c[1][2], c[2][2]);
    e1[1] = srt_atan2f(-c[0][2], cy);
    e1[2] = srt_atan2f(c[0][1], c[0][0]);
    e2[0] = srt_atan2f(-c[1][2], -c[2][2]);
    e2[1] = srt_atan2f(-c[0][2], -cy);
    e2[2] = srt_atan2f(-c[0][1], -c[0][0]);
  } else {
    e1[0] = srt_atan2f(-c[2][1], c[1][1]);
    e1[1] = srt_atan2f(-c[0][2], cy);
    e1[2] = 0;
    e2[0] = e1[0]; e2[1] = e1[1]; e2[2] = e1[2];
  }
  const float d1 = (fabsf(e1[0]) + fabsf(e1[1])) + fabsf(e1[2]);
  const float d2 = (fabsf(e2[0]) + fabsf(e2[1])) + fabsf(e2[2]);
  const float deg = 180.0f / kPi;                                    // Degrees(v) = v * (180.0f / PI_F)
  if (d1 > d2) return {e2[0] * deg, e2[1] * deg, e2[2] * deg};
  return {e1[0] * deg, e1[1] * deg, e1[2] * deg};
}

SRT_ANIM_FN void anim_mat4_identity(float* m) {
  for (int i = 0; i < 16; i++) m[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}

// Mat4::rotate(t, axis) (lib/mat4.h:389-405), the general-axis expressions as written - axis.normalize() included: for the unit
// axes the terms that multiply a zero stay, and with them the signs of the zeros they produce.
SRT_ANIM_FN void anim_mat4_rotate(float t, float ax, float ay, float az, float* m) {
  anim_mat4_identity(m);
  float c, s;
  srt_sincosf2(t * (kPi / 180.0f), c, s);                            // Radians(v) = v * (PI_F / 180.0f)
  const float n = sqrtf((ax * ax + ay * ay) + az * az);
  const float axis[3] = {ax / n, ay / n, az / n};
  const float k = 1.0f - c;
  const float temp[3] = {axis[0] * k, axis[1] * k, axis[2] * k};
  m[0] = c + temp[0] * axis[0];
  m[1] = temp[0] * axis[1] + s * axis[2];
  m[2] = temp[0] * axis[2] - s * axis[1];
  m[4] = temp[1] * axis[0] - s * axis[2];
  m[5] = c + temp[1] * axis[1];
  m[6] = temp[1] * axis[2] + s * axis[0];
  m[8] = temp[2] * axis[0] + s * axis[1];
  m[9] = temp[2] * axis[1] - s * axis[0];
  m[10] = c + temp[2] * axis[2];
}

// Mat4::euler (:383-387): (rotate(z, Z) * rotate(y, Y)) * rotate(x, X) through Mat4::operator*.
SRT_ANIM_FN void anim_mat4_euler(AnimV3 angles, float* m) {
  float rz[16], ry[16], rx[16], zy[16];
  anim_mat4_rotate(angles.z, 0.0f, 0.0f, 1.0f, rz);
  anim_mat4_rotate(angles.y, 0.0f, 1.0f, 0.0f, ry);
  anim_mat4_rotate(angles.x, 1.0f, 0.0f, 0.0f, rx);
  skin_mat4_mul(rz, ry, zy);
  skin_mat4_mul(zy, rx, m);
}

SRT_ANIM_FN void anim_mat4_translate(AnimV3 t, float* m) {
  anim_mat4_identity(m);
  m[12] = t.x; m[13] = t.y; m[14] = t.z;
}

// Pose::transform (scene/pose.cpp:4-6): (translate(pos) * euler(euler)) * scale(scale)
SRT_ANIM_FN void anim_pose_transform(AnimV3 pos, AnimV3 euler, AnimV3 scale, float* m) {
  float t[16], r[16], s[16], tr[16];
  anim_mat4_translate(pos, t);
  anim_mat4_euler(euler, r);
  anim_mat4_identity(s);
  s[0] = scale.x; s[5] = scale.y; s[10] = scale.z;
  skin_mat4_mul(t, r, tr);
  skin_mat4_mul(tr, s, m);
}

// Anim_Pose::at(t) (:54-57) of object k of a timeline: track_offsets[3 k ..] = its position, rotation and scale tracks.  pose9
// (may be NULL) takes the pose's position, Euler angles and scale; trans the 16 floats of Pose::transform().
SRT_ANIM_FN void anim_object_transform(const uint32_t* track_offsets, const float* times, const float* values, uint32_t k, float t, float* pose9,
                                       float* trans) {
  const uint32_t* o = track_offsets + 3 * (size_t)k;
  const AnimV3 p = anim_spline_vec3(times, values, o[0], o[1], t);
  const AnimV3 r = anim_quat_to_euler(anim_spline_quat(times, values, o[1], o[2], t));
  const AnimV3 s = anim_spline_vec3(times, values, o[2], o[3], t);
  if (pose9) { pose9[0] = p.x; pose9[1] = p.y; pose9[2] = p.z; pose9[3] = r.x; pose9[4] = r.y; pose9[5] = r.z; pose9[6] = s.x; pose9[7] = s.y; pose9[8] = s.z; }
  anim_pose_transform(p, r, s, trans);
}

// Skeleton::set_time for joint j (scene/skeleton.cpp:47-54): a joint with keys takes anim.at(t).to_euler(), one without keeps its
// rest pose.
SRT_ANIM_FN AnimV3 anim_joint_pose(const float* rest_pose, const uint32_t* knot_offsets, const float* times, const float* quats, uint32_t j, float t) {
  const uint32_t b = knot_offsets[j], e = knot_offsets[j + 1u];
  if (e <= b) return anim_v3(rest_pose + 3 * (size_t)j);
  return anim_quat_to_euler(anim_spline_quat(times, quats, b, e, t));
}

// Skeleton::joint_to_posed(j) (student/skeleton.cpp:106-115) = translate(base_pos) * Joint::joint_to_posed (:26-52): from
// iter = euler(pose_j), for every ancestor from the parent up to the root iter = translate(extent) * iter, then iter = euler(pose) *
// iter.  local: Mat4::euler(pose) per joint, 16 floats each; cap: the skin's {extent, radius}, 4 floats per joint; parent[j] < j or -1.  The walk is as long
// as the joint is deep and never longer than njoints.  anim_joint_chain is the walk alone - Joint::joint_to_posed, skeleton space,
// what Skeleton::step_ik reads (pt_ik.h).
SRT_ANIM_FN void anim_joint_chain(const int32_t* parent, const float* cap, const float* local, uint32_t njoints, uint32_t j, float* iter) {
  float next[16], tr[16];
  for (int i = 0; i < 16; i++) iter[i] = local[16 * (size_t)j + i];
  int32_t cur = parent[j];
  for (uint32_t step = 0; cur >= 0 && (uint32_t)cur < njoints && step < njoints; step++) {
    anim_mat4_translate(anim_v3(cap + 4 * (size_t)cur), tr);
    skin_mat4_mul(tr, iter, next);
    skin_mat4_mul(local + 16 * (size_t)cur, next, iter);
    cur = parent[cur];
  }
}

SRT_ANIM_FN void anim_joint_to_posed(const int32_t* parent, const float* cap, const float* base, const float* local, uint32_t njoints, uint32_t j,
                                     float* posed) {
  float iter[16], tr[16];
  anim_joint_chain(parent, cap, local, njoints, j, iter);
  anim_mat4_translate(anim_v3(base), tr);
  skin_mat4_mul(tr, iter, posed);
}

// ---- shading timelines: Material::Anim_Material::at (scene/material.cpp:44-52), Scene_Light::Anim_Light::at (scene/light.cpp:139-144)
// and Scene_Light::set_time (:30-38) ----
// Spline<Spectrum>, Spline<Vec2> and Spline<float> are the fork's Spline<T>::at (student/spline.inl:5-72) over types whose operators
// work channel by channel with one rounding each and true divisions (lib/spectrum.h:84-102,136-138, lib/vec2.h:83-107,175-177): they
// are anim_spline_vec3 on components padded with zeros (xyz_, xy__, x___), and an empty track gives T() - a zero Spectrum, 0.0f.
//
// Spectrum::to_linear (lib/spectrum.h:54-60), both branches.  The host form calls libm's powf, as the reference does; the device
// form calls srt_powf (SRT-MATH v2, glibc 2.35's powf restated), whose argument (f + 0.055f) / 1.055f with f > 0.04045f is a positive
// normal number for every finite f.  Non-finite channels: NaN takes the division and stays NaN, -inf takes the division and stays
// -inf, and +inf - the one input outside srt_powf's domain - is answered here with libm's +inf, so both forms agree on every input.
SRT_ANIM_FN float anim_to_linear(float f) {
  if (f > 0.04045f) {
    const float x = (f + 0.055f) / 1.055f;
#if defined(__HIP_DEVICE_COMPILE__)
    if (f2u(x) == 0x7f800000u) return x;
    return srt_powf(x, 2.4f);
#else
    return powf(x, 2.4f);
#endif
  }
  return f / 12.92f;
}

// Material::Options after Anim_Material::at(t): the tuple's order - albedo, reflectance, transmittance, emissive, intensity, ior.
struct AnimMaterialOptions { AnimV3 albedo, reflectance, transmittance, emissive; float intensity, ior; };

// o: the seven offsets of one material's six tracks.
SRT_ANIM_FN AnimMaterialOptions anim_material_options(const uint32_t* o, const float* times, const float* values, float t) {
  AnimMaterialOptions p;
  p.albedo = anim_spline_vec3(times, values, o[0], o[1], t);
  p.reflectance = anim_spline_vec3(times, values, o[1], o[2], t);
  p.transmittance = anim_spline_vec3(times, values, o[2], o[3], t);
  p.emissive = anim_spline_vec3(times, values, o[3], o[4], t);
  p.intensity = anim_spline_vec3(times, values, o[4], o[5], t).x;
  p.ior = anim_spline_vec3(times, values, o[5], o[6], t).x;
  return p;
}

// The material as srt_pt_add_material takes it, from the options, as Pathtracer::build_scene maps them to BSDFs (rays/pathtracer.cpp:93-117):
// Lambertian a = albedo.to_linear(); Mirror a = reflectance; Glass a = transmittance, b = reflectance, ior; Diffuse light a =
// Material::emissive() = emissive * intensity (scene/material.cpp:34-36); Refract a = transmittance, ior.  Fields a type does not
// read are zero.  `type` is the committed SRT_MAT_* type.
SRT_ANIM_FN void anim_material_values(uint32_t type, const AnimMaterialOptions& p, float a[3], float b[3], float* ior) {
  AnimV3 va = {0.0f, 0.0f, 0.0f}, vb = {0.0f, 0.0f, 0.0f};
  *ior = 0.0f;
  if (type == 0u) va = {anim_to_linear(p.albedo.x), anim_to_linear(p.albedo.y), anim_to_linear(p.albedo.z)};
  else if (type == 1u) va = p.reflectance;
  else if (type == 2u) { va = p.transmittance; vb = p.reflectance; *ior = p.ior; }
  else if (type == 3u) va = p.emissive * p.intensity;
  else { va = p.transmittance; *ior = p.ior; }
  a[0] = va.x; a[1] = va.y; a[2] = va.z;
  b[0] = vb.x; b[1] = vb.y; b[2] = vb.z;
}

// The record the kernels read, from the material as srt_pt_add_material takes it: BSDF_Lambertian(albedo) : albedo(albedo / PI_F)
// (rays/bsdf.h:26), which build_scene of pt_scene.cpp applies at the commit.
SRT_ANIM_FN void anim_material_store(Material* m) {
  if (m->type == 0u)
    for (int i = 0; i < 3; i++) m->a[i] = m->a[i] / kPi;
}

// Material k of a shading timeline at time t, as srt_pt_add_material takes it (the type is the committed one and is not written).
SRT_ANIM_FN void anim_material_item(const uint32_t* track_offsets, const float* times, const float* values, uint32_t k, float t, Material* m) {
  const AnimMaterialOptions p = anim_material_options(track_offsets + 6 * (size_t)k, times, values, t);
  anim_material_values(m->type, p, m->a, m->b, &m->ior);
}

// Scene_Light::set_time for one light.  o: the seven offsets of its six tracks - spectrum, intensity, angle_bounds, then the Anim_Pose
// triple.  The option triple and the pose triple are independent: one without a key leaves its outputs untouched (options /
// pose say which were written).  radiance = Scene_Light::radiance() = spectrum * intensity (scene/light.cpp:98-100); trans =
// Pose::transform() of Anim_Pose::at(t).
struct AnimLightOut { bool options, pose; float radiance[3], angle_bounds[2], trans[16]; };
SRT_ANIM_FN void anim_light_item(const uint32_t* o, const float* times, const float* values, float t, AnimLightOut* out) {
  out->options = o[3] > o[0];
  out->pose = o[6] > o[3];
  if (out->options) {
    const AnimV3 spectrum = anim_spline_vec3(times, values, o[0], o[1], t);
    const float intensity = anim_spline_vec3(times, values, o[1], o[2], t).x;
    const AnimV3 bounds = anim_spline_vec3(times, values, o[2], o[3], t);
    const AnimV3 r = spectrum * intensity;
    out->radiance[0] = r.x; out->radiance[1] = r.y; out->radiance[2] = r.z;
    out->angle_bounds[0] = bounds.x; out->angle_bounds[1] = bounds.y;
  }
  if (out->pose) anim_object_transform(o + 3, times, values, 0u, t, nullptr, out->trans);
}

// The environment light's radiance: o: the three offsets of its two tracks (spectrum, intensity).  One item, evaluated on the host by
// every form - the radiance is a launch parameter (DScene::env_radiance), not scene memory; this is the function a kernel would run.
SRT_ANIM_FN void anim_env_item(const uint32_t* o, const float* times, const float* values, float t, float radiance[3]) {
  const AnimV3 r = anim_spline_vec3(times, values, o[0], o[1], t) * anim_spline_vec3(times, values, o[1], o[2], t).x;
  radiance[0] = r.x; radiance[1] = r.y; radiance[2] = r.z;
}

// What srt_pt_timeline_create and srt_pt_skin_set_rig refuse about their knot tables, as a message (empty: nothing).  offsets holds
// nitems * per_item + 1 entries - per_item tracks per object or joint - from 0, never descending; the times of one track ascend
// strictly and are finite; with refuse_empty_items an item whose tracks are all empty is refused (Splines::any() is false for it:
// the reference would not move it).  Knot values are not looked at.  Reads offsets[0 .. nitems * per_item] and times[0 .. last offset).
inline std::string anim_check_tracks(const uint32_t* offsets, uint32_t nitems, uint32_t per_item, const float* times, bool refuse_empty_items,
                                     const char* item) {
  const size_t ntracks = (size_t)nitems * per_item;
  if (offsets[0] != 0u) return "the offsets start at " + std::to_string(offsets[0]) + ", not 0";
  for (size_t q = 0; q < ntracks; q++)
    if (offsets[q + 1] < offsets[q]) return "the offsets descend at track " + std::to_string(q) + " (" + std::to_string(offsets[q]) + " > " + std::to_string(offsets[q + 1]) + ")";
  for (size_t q = 0; q < ntracks; q++)
    for (uint32_t k = offsets[q]; k < offsets[q + 1]; k++) {
      if (!std::isfinite(times[k])) return "knot " + std::to_string(k) + " (track " + std::to_string(q) + ") has a non-finite time";
      if (k > offsets[q] && !(times[k - 1u] < times[k])) return "the times of track " + std::to_string(q) + " do not ascend strictly at knot " + std::to_string(k);
    }
  if (refuse_empty_items)
    for (uint32_t i = 0; i < nitems; i++)
      if (offsets[(size_t)i * per_item] == offsets[(size_t)(i + 1u) * per_item])
        return std::string(item) + " " + std::to_string(i) + " of the list has no key on any track (Splines::any() is false: the reference would not move it)";
  return std::string();
}

// Skeleton::set_time(t) and Skeleton::joint_to_posed for every joint on the host: euler3 (may be NULL) takes Joint::pose, local is
// njoints * 16 floats of scratch, posed the result.  What srt_pt_skin_posed runs and anim_joint_local_kernel / anim_joint_chain_kernel
// are held to.
inline void anim_rig_posed_host(const int32_t* parent, const float* cap, const float* base, const float* rest_pose, const uint32_t* knot_offsets,
                                const float* times, const float* quats, uint32_t njoints, float t, float* euler3, float* local, float* posed) {
  for (uint32_t j = 0; j < njoints; j++) {
    const AnimV3 e = anim_joint_pose(rest_pose, knot_offsets, times, quats, j, t);
    if (euler3) { euler3[3 * (size_t)j] = e.x; euler3[3 * (size_t)j + 1] = e.y; euler3[3 * (size_t)j + 2] = e.z; }
    anim_mat4_euler(e, local + 16 * (size_t)j);
  }
  for (uint32_t j = 0; j < njoints; j++) anim_joint_to_posed(parent, cap, base, local, njoints, j, posed + 16 * (size_t)j);
}

// The launches of pt_anim.hip.  Plain device pointers; `stream` is a hipStream_t; every call only enqueues.
// d_trans_out[16 k ..] = Pose::transform() of Anim_Pose::at(t) for the nobjects objects of the tables
void launch_anim_pose(void* stream, const uint32_t* d_track_offsets, const float* d_times, const float* d_values, uint32_t nobjects, float t, float* d_trans_out);
// d_local[16 j ..] = Mat4::euler(pose_j) after Skeleton::set_time(t); then d_mats[16 j ..] = joint_to_posed(j) * d_inv[16 j ..] and, with
// d_posed_out, d_posed_out[16 j ..] = joint_to_posed(j)
void launch_anim_joints(void* stream, const int32_t* d_parent, const float* d_cap, const float* d_base, const float* d_rest_pose, const uint32_t* d_knot_offsets,
                        const float* d_times, const float* d_quats, uint32_t njoints, float t, float* d_local, const float* d_inv, float* d_mats,
                        float* d_posed_out);
// The same two kernels with Mat4::euler of d_pose (3 floats per joint: the skin's current Joint::pose) in the place of set_time(t)'s angles
void launch_anim_joints_pose(void* stream, const int32_t* d_parent, const float* d_cap, const float* d_base, const float* d_pose, uint32_t njoints,
                             float* d_local, const float* d_inv, float* d_mats, float* d_posed_out);
// srt_pt_shading_timeline_apply: one lane per item, materials first, then lights.  Lane k < nmaterials writes a, b and ior of
// d_mats[d_materials[k]] (anim_material_item, anim_material_store; the type is read from the record and stays); lane nmaterials + j
// writes radiance and angle_bounds (option keys) and trans, itrans, has_trans (pose keys) of d_dlights[d_lights[j]].  The track
// offsets are those of the timeline: 6 per material, then 6 per light.  The caller has checked every index against the tables.
void launch_anim_shading(void* stream, const uint32_t* d_track_offsets, const float* d_times, const float* d_values, const uint32_t* d_materials,
                         uint32_t nmaterials, const uint32_t* d_lights, uint32_t nlights, float t, Material* d_mats, DeltaLight* d_dlights);
// d_out[i] = srt_hypotf(d_x[i], d_y[i]) (srt_pt_math_hypot)
void launch_anim_hypot(void* stream, const float* d_x, const float* d_y, size_t n, float* d_out);

}  // namespace srt

#endif
