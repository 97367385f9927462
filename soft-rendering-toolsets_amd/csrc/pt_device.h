// Device-side arithmetic of the path tracer: vector / matrix helpers with the reference's operation
// order, SRT-RNG v1, SRT-MATH v2 (glibc's sincosf algorithm), primitive intersection.
//
// Everything here must round exactly like the x86-64 build of the reference: fp32 throughout, fp64
// only where the reference widens (unqualified sqrt/pow), no FMA contraction (-ffp-contract=off),
// IEEE divide/sqrt (hipcc default), denormals preserved.  Reference paths are relative to
// /root/reference/Assignments/Scotty3D/src/.
#ifndef SRT_PT_DEVICE_H
#define SRT_PT_DEVICE_H

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "pt_scene.h"

namespace srt {

#define SRT_DEV __device__ __forceinline__

constexpr float kEps = 0.00001f;                                   // EPS_F, lib/mathlib.h:16
constexpr float kPi = 3.14159265358979323846264338327950288f;      // PI_F,  lib/mathlib.h:17

struct V3 { float x, y, z; };
struct Spec { float r, g, b; };
struct Ray { V3 o, d; float b0, b1; };

// ---- IEEE divide / square root with the range handling hoisted out of the common case ----
// hipcc expands a correctly rounded fp32 divide to v_div_scale x2, v_rcp, a five-step FMA refinement, v_div_fmas and
// v_div_fixup, and a square root to v_sqrt plus a +-1 ulp correction wrapped in denormal scaling and a class
// fix-up.  When no operand needs scaling or fixing (every lane's operands are normal numbers well inside the
// exponent range: v_div_scale returns its input, VCC = 0, v_div_fixup and the sqrt fix-ups pass the result
// through) what remains is the refinement itself, and the part of it that only depends on the denominator can
// be shared by the quotients of one triangle test (u, v, t over det) or one normalisation (x, y, z over the norm).
// Used by the wave kernel's batch tests only (two or three rays at a time, so the serial refinement chains overlap).
// The fast path is taken when the whole wave qualifies; any other operand sends the wave through the compiler's
// own sequence, so the results are those of the plain `/` and sqrtf for every input
// (tests/test_pt_gpu.py::test_exact_division_and_sqrt_fast_paths sweeps both against them).
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SRT_PLAIN_DIV_SQRT)
#define SRT_EXACT_FAST_PATHS 1
#else
#define SRT_EXACT_FAST_PATHS 0
#endif

#if SRT_EXACT_FAST_PATHS
SRT_DEV float div_refine(float num, float den, float r) {
  float q = num * r;
  const float e1 = __builtin_fmaf(-den, q, num);
  q = __builtin_fmaf(e1, r, q);
  const float e2 = __builtin_fmaf(-den, q, num);
  return __builtin_fmaf(e2, r, q);
}
#endif
// N square roots / 3 N quotients (the N rays of a batch): one range verdict for all operands, and the
// refinement chains of the three rays are independent instruction streams inside one basic block.
// zero[r] = "x[r] is exactly +0" as the caller knows it (origin on the triangle's plane: t = 0; a ray without a hit:
// distance of a point from itself): v_sqrt(0) = 0 and neither correction applies, so a zero may take the fast path.
template <int N>
SRT_DEV void sqrtN(const float* x, const bool* zero, float* o) {
#if SRT_EXACT_FAST_PATHS
  bool bad = false;
#pragma unroll
  for (int r = 0; r < N; r++) bad = bad || (!zero[r] && !(x[r] >= 0x1p-96f && x[r] <= FLT_MAX));
  if (__ballot(bad) == 0ull) {
#pragma unroll
    for (int r = 0; r < N; r++) {
      const float s = __builtin_amdgcn_sqrtf(x[r]);
      const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
      const float rm = __builtin_fmaf(-sm, s, x[r]), rp = __builtin_fmaf(-sp, s, x[r]);
      float v = (0.0f >= rm) ? sm : s;
      v = (0.0f < rp) ? sp : v;
      o[r] = v;
    }
    return;
  }
#endif
#pragma unroll
  for (int r = 0; r < N; r++) o[r] = sqrtf(x[r]);
}
// The fast path's range verdict: every |operand| of the lane in [2^-40, 2^40] (a shared column 2 may also be exactly zero);
// div_window is the same of the whole wave, one ballot.
template <int N, bool SHARED_C2>
SRT_DEV bool div_in_range(const float (*n)[3], const float* den) {
  const float lo = 0x1p-40f, hi = 0x1p40f;     // quotient exponents stay within +-80: no scaling case of v_div_scale
  float mn = fabsf(den[0]), mx = fabsf(den[0]);
#pragma unroll
  for (int r = 1; r < N; r++) { mn = fminf(mn, fabsf(den[r])); mx = fmaxf(mx, fabsf(den[r])); }
#pragma unroll
  for (int r = 0; r < N; r++) {
    if (SHARED_C2) {
      mn = fminf(mn, fminf(fabsf(n[r][0]), fabsf(n[r][1])));
      mx = fmaxf(mx, fmaxf(fabsf(n[r][0]), fabsf(n[r][1])));
    } else {
      mn = fminf(fminf(mn, fabsf(n[r][0])), fminf(fabsf(n[r][1]), fabsf(n[r][2])));
      mx = fmaxf(fmaxf(mx, fabsf(n[r][0])), fmaxf(fabsf(n[r][1]), fabsf(n[r][2])));
    }
  }
  if (SHARED_C2) {
    const float c2 = (n[0][2] == 0.0f) ? 1.0f : fabsf(n[0][2]);
    mn = fminf(mn, c2); mx = fmaxf(mx, c2);
  }
  // (min / max skip a NaN operand: it stays a NaN through the refinement, as it would through the full sequence)
  return mn >= lo && mx <= hi;
}
#if SRT_EXACT_FAST_PATHS
template <int N, bool SHARED_C2>
SRT_DEV bool div_window(const float (*n)[3], const float* den) { return __ballot(!div_in_range<N, SHARED_C2>(n, den)) == 0ull; }
// 1 / den for the refinement: v_rcp (1 ulp) and one Newton step.
SRT_DEV float rcp_refined(float den) {
  const float rc = __builtin_amdgcn_rcpf(den);
  return __builtin_fmaf(__builtin_fmaf(-den, rc, 1.0f), rc, rc);
}
#endif
// q[r][j] = n[r][j] / den[r].  SHARED_C2: the caller passes the same numerator in column 2 for all rays (the
// numerator of t), which is exactly zero for an origin on the triangle's plane; such a lane takes the fast path as
// well and v_div_fixup gives the signed zero the full sequence would.
template <int N, bool SHARED_C2>
SRT_DEV void divNx3(const float (*n)[3], const float* den, float (*q)[3]) {
#if SRT_EXACT_FAST_PATHS
  if (div_window<N, SHARED_C2>(n, den)) {
#pragma unroll
    for (int r = 0; r < N; r++) {
      const float rc = rcp_refined(den[r]);
#pragma unroll
      for (int j = 0; j < 3; j++) q[r][j] = div_refine(n[r][j], den[r], rc);
      if (SHARED_C2) q[r][2] = __builtin_amdgcn_div_fixupf(q[r][2], den[r], n[r][2]);
    }
    return;
  }
#endif
#pragma unroll
  for (int r = 0; r < N; r++)
#pragma unroll
    for (int j = 0; j < 3; j++) q[r][j] = n[r][j] / den[r];
}

SRT_DEV V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
SRT_DEV V3 v3p(const float* p) { return v3(p[0], p[1], p[2]); }
SRT_DEV V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
SRT_DEV V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
SRT_DEV V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }   // Vec3*float == float*Vec3
SRT_DEV V3 operator/(V3 a, float s) { return v3(a.x / s, a.y / s, a.z / s); }
SRT_DEV V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
SRT_DEV float dot(V3 l, V3 r) { return l.x * r.x + l.y * r.y + l.z * r.z; }
SRT_DEV V3 cross(V3 l, V3 r) { return v3(l.y * r.z - l.z * r.y, l.z * r.x - l.x * r.z, l.x * r.y - l.y * r.x); }
SRT_DEV float norm2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
SRT_DEV float norm(V3 a) { return sqrtf(norm2(a)); }
SRT_DEV V3 unit(V3 a) { return a / norm(a); }
SRT_DEV float std_min(float a, float b) { return (b < a) ? b : a; }
SRT_DEV float std_max(float a, float b) { return (a < b) ? b : a; }

SRT_DEV Spec spec(float r, float g, float b) { Spec s; s.r = r; s.g = g; s.b = b; return s; }
SRT_DEV Spec operator+(Spec a, Spec b) { return spec(a.r + b.r, a.g + b.g, a.b + b.b); }
SRT_DEV Spec operator-(Spec a, Spec b) { return spec(a.r - b.r, a.g - b.g, a.b - b.b); }
SRT_DEV Spec operator*(Spec a, Spec b) { return spec(a.r * b.r, a.g * b.g, a.b * b.b); }
SRT_DEV Spec operator*(Spec a, float s) { return spec(a.r * s, a.g * s, a.b * s); }
SRT_DEV float luma(Spec a) { return 0.2126f * a.r + 0.7152f * a.g + 0.0722f * a.b; }   // lib/spectrum.h:111
SRT_DEV bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
SRT_DEV bool valid(Spec a) { return finite_f(a.r) && finite_f(a.g) && finite_f(a.b); }  // lib/spectrum.h:115
// finite_f as one v_cmp_class_f32 on the device
SRT_DEV bool class_finite(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_classf(v, 0x1f8);             // -normal, -denormal, -0, +0, +denormal, +normal
#else
  return finite_f(v);
#endif
}

// Mat4 * Vec3 (projective, lib/mat4.h:125-131) and Mat4::rotate (w = 0; the 0*col3 term is kept).
SRT_DEV V3 mat_point(const Mat4& m, V3 v) {
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = ((m.c[0][j] * v.x + m.c[1][j] * v.y) + m.c[2][j] * v.z) + m.c[3][j] * 1.0f;
  return v3(o[0] / o[3], o[1] / o[3], o[2] / o[3]);
}
// The same for the wave kernel: x / 1.0f == x bit for bit, so the perspective divide is skipped when w == 1 in every active
// lane (always the case for affine matrices and finite points); one lane with another w sends the wave through the divides.
// The matrix may differ from lane to lane.
SRT_DEV V3 mat_point_uniform(const Mat4& m, V3 v) {
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; j++) o[j] = ((m.c[0][j] * v.x + m.c[1][j] * v.y) + m.c[2][j] * v.z) + m.c[3][j] * 1.0f;
  if (__ballot(o[3] != 1.0f) == 0ull) return v3(o[0], o[1], o[2]);
  return v3(o[0] / o[3], o[1] / o[3], o[2] / o[3]);
}
// The same for a matrix that is the same in every lane (an object's trans / itrans in the leaf section of pt_wave.h): w is known to
// be 1 without computing it.
//   * `affine` = the bottom row is (+-0, +-0, +-0, 1) - mat_affine_row, tested once per object on the bit patterns, which for a
//     wave-uniform matrix is integer work on the scalar unit.
//   * For such a row and finite x, y, z: w = ((+-0 * x + +-0 * y) + +-0 * z) + 1 * 1 = +-0 + 1 = 1 exactly.
//   * x, y and z are finite whenever o[0] is: row 0 adds a product of each of them, a non-finite factor makes its product +-inf or
//     NaN (0 * inf included), and a sum that contains +-inf or NaN is not finite, whatever the matrix holds.
// So with an affine row and a finite o[0] in every active lane the three rows are mat_point's result bit for bit (x / 1.0f == x);
// one class compare stands in for the fourth row and its comparison.  Anything else computes w and goes on as mat_point_uniform.
#ifndef SRT_POINT_AFFINE
#define SRT_POINT_AFFINE 1
#endif
SRT_DEV bool mat_affine_row(const Mat4& m) {
  return SRT_POINT_AFFINE != 0 && ((__float_as_uint(m.c[0][3]) | __float_as_uint(m.c[1][3]) | __float_as_uint(m.c[2][3])) << 1) == 0u &&
         __float_as_uint(m.c[3][3]) == 0x3f800000u;
}
SRT_DEV V3 mat_point_affine(const Mat4& m, bool affine, V3 v, bool* w_skipped = nullptr) {   // (w_skipped: the probe's report)
  float o[4];
#pragma unroll
  for (int j = 0; j < 3; j++) o[j] = ((m.c[0][j] * v.x + m.c[1][j] * v.y) + m.c[2][j] * v.z) + m.c[3][j] * 1.0f;
  const bool skip = affine && __ballot(!class_finite(o[0])) == 0ull;
  if (w_skipped) *w_skipped = skip;
  if (skip) return v3(o[0], o[1], o[2]);
  o[3] = ((m.c[0][3] * v.x + m.c[1][3] * v.y) + m.c[2][3] * v.z) + m.c[3][3] * 1.0f;
  if (__ballot(o[3] != 1.0f) == 0ull) return v3(o[0], o[1], o[2]);
  return v3(o[0] / o[3], o[1] / o[3], o[2] / o[3]);
}
// W1: the caller is the wave kernel and takes the form above
template <bool W1>
SRT_DEV V3 mat_point_as(const Mat4& m, V3 v) { return W1 ? mat_point_uniform(m, v) : mat_point(m, v); }
SRT_DEV V3 mat_rotate(const Mat4& m, V3 v) {
  float o[3];
#pragma unroll
  for (int j = 0; j < 3; j++) o[j] = ((m.c[0][j] * v.x + m.c[1][j] * v.y) + m.c[2][j] * v.z) + m.c[3][j] * 0.0f;
  return v3(o[0], o[1], o[2]);
}
// m.T().rotate(v): component j = v.x*m[j][0] + v.y*m[j][1] + v.z*m[j][2] + 0*m[j][3]
SRT_DEV V3 mat_rotate_transposed(const Mat4& m, V3 v) {
  float o[3];
#pragma unroll
  for (int j = 0; j < 3; j++) o[j] = ((m.c[j][0] * v.x + m.c[j][1] * v.y) + m.c[j][2] * v.z) + m.c[j][3] * 0.0f;
  return v3(o[0], o[1], o[2]);
}

// Ray::transform (lib/ray.h:31-37)
template <bool W1 = false>
SRT_DEV void ray_transform(Ray& r, const Mat4& m) {
  r.o = mat_point_as<W1>(m, r.o);
  r.d = mat_rotate(m, r.d);
  const float d = norm(r.d);
  r.b0 *= d;
  r.b1 *= d;
  r.d = r.d / d;
}
SRT_DEV Ray make_ray(V3 o, V3 d, float b0, float b1) {  // explicit Ray(point, dir, bounds): dir.unit()
  Ray r; r.o = o; r.d = unit(d); r.b0 = b0; r.b1 = b1; return r;
}
SRT_DEV V3 ray_at(const Ray& r, float t) { return r.o + r.d * t; }

// ---------------------------------------------------------------------------------------------------
// SRT-RNG v1 (replaces util/rand.cpp:13-25): PCG32 XSH-RR keyed by splitmix64(seed, pixel, sample)
// ---------------------------------------------------------------------------------------------------
struct Rng {
  uint64_t state, inc;
  uint32_t draws;
  SRT_DEV void key(uint64_t seed, uint32_t pixel, uint32_t sample) {
    const uint64_t k = ((uint64_t)pixel << 32) | sample;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (k + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    inc = (k << 1) | 1;
    state = z * 6364136223846793005ull + inc;
    draws = 0;
  }
  SRT_DEV uint32_t next() {
    const uint64_t old = state;
    state = old * 6364136223846793005ull + inc;
    const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27);
    const uint32_t rot = (uint32_t)(old >> 59);
    draws++;
    return (xs >> rot) | (xs << ((32 - rot) & 31));
  }
  SRT_DEV float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }
  SRT_DEV int integer(int lo, int hi) { return lo + (int)(((uint64_t)next() * (uint64_t)(uint32_t)(hi - lo)) >> 32); }
  SRT_DEV bool coin(float p) { return unit() < p; }
};

// The SRT-MATH functions below are host functions too (SRT_HD): pt_anim.h evaluates timelines with them on both sides.  f2u / u2f
// are the bit casts for both compilers.
#define SRT_HD __host__ __device__ __forceinline__
SRT_HD uint32_t f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
SRT_HD float u2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
// ---------------------------------------------------------------------------------------------------
// SRT-MATH v2: glibc 2.35 sinf/cosf (sysdeps/ieee754/flt-32/{s_sinf,s_cosf}.c, sincosf.h, sincosf_data.c)
// evaluated in fp64 without FMA.  Valid for |x| < 120 (the renderer uses [0, 2pi] and [-1, 1]).
// ---------------------------------------------------------------------------------------------------
SRT_HD float sincos_poly(double x, double x2, bool negated_cos_table, int n) {
  const double sgn = negated_cos_table ? -1.0 : 1.0;  // table[1] negates the cosine coefficients only
  if ((n & 1) == 0) {
    const double x3 = x * x2;
    const double s1 = 0x1.1107605230bc4p-7 + x2 * -0x1.994eb3774cf24p-13;
    const double x7 = x3 * x2;
    const double s = x + x3 * -0x1.555545995a603p-3;
    return (float)(s + x7 * s1);
  } else {
    const double x4 = x2 * x2;
    const double c2 = (sgn * -0x1.6c087e89a359dp-10) + x2 * (sgn * 0x1.99343027bf8c3p-16);
    const double c1 = (sgn * 0x1p0) + x2 * (sgn * -0x1.ffffffd0c621cp-2);
    const double x6 = x4 * x2;
    const double c = c1 + x4 * (sgn * 0x1.55553e1068f19p-5);
    return (float)(c + x6 * c2);
  }
}
// glibc's control flow, kept as the form the branch-free functions below are held to (tests/test_pt_sincos_host.py compares them
// for every float in range, bit for bit), as tri_hit stays beside tri_hitN.  Nothing on a hot path calls the _plain functions.
SRT_HD float srt_sincosf_plain(float y, int want_cos) {
  double x = (double)y;
  const uint32_t top = (f2u(y) >> 20) & 0x7ffu;
  if (top < 0x3f4u) {                      // abstop12(y) < abstop12(pi/4 = 0x1.921FB6p-1f)
    if (top < 0x398u) return want_cos ? 1.0f : y;   // |y| < 2^-12
    return sincos_poly(x, x * x, false, want_cos);
  }
  if (top < 0x42fu) {                      // abstop12(120.0f)
    const double r = x * 0x1.45F306DC9C883p+23;
    const int n = ((int32_t)r + 0x800000) >> 24;
    x = x - n * 0x1.921FB54442D18p0;
    const int q = n & 3;
    const double s = (q == 1 || q == 2) ? -1.0 : 1.0;
    return sincos_poly(x * s, x * x, (n & 2) != 0, n ^ want_cos);
  }
  return u2f(0x7fc00000u);
}
// cosf(y) and sinf(y) together: both glibc routines reduce y the same way, so the reduction is shared.
SRT_HD void srt_sincosf2_plain(float y, float& c, float& s) {
  double x = (double)y;
  const uint32_t top = (f2u(y) >> 20) & 0x7ffu;
  if (top < 0x3f4u) {
    if (top < 0x398u) { c = 1.0f; s = y; return; }
    const double x2 = x * x;
    c = sincos_poly(x, x2, false, 1);
    s = sincos_poly(x, x2, false, 0);
    return;
  }
  if (top < 0x42fu) {
    const double r = x * 0x1.45F306DC9C883p+23;
    const int n = ((int32_t)r + 0x800000) >> 24;
    x = x - n * 0x1.921FB54442D18p0;
    const int q = n & 3;
    const double sg = (q == 1 || q == 2) ? -1.0 : 1.0;
    const double xs = x * sg, x2 = x * x;
    c = sincos_poly(xs, x2, (n & 2) != 0, n ^ 1);
    s = sincos_poly(xs, x2, (n & 2) != 0, n);
    return;
  }
  c = s = u2f(0x7fc00000u);
}
// The same arithmetic in one straight line: lanes of a wave hold different quadrants and both sides of pi/4, so the
// branches above are walked one after the other.  Every argument is reduced (below pi/4 the quadrant n is 0, x - 0 * hpi == x, and
// the table and sign selects fall on the short path's values), the sine form and the cosine form of the reduced argument are
// evaluated once each and the caller selects by the parity of n.  The signs are applied to the two results, not to their operands:
// the sine form is odd in x (every product and sum rounds symmetrically), and the negated cosine table negates every term.
// fs = sincos_poly(x * s, x * x, (n & 2) != 0, 0), fc = the same with an odd last argument, for y below 120 in magnitude;
// larger arguments, infinities and NaN reduce 0 in their place (the double -> int32 conversion stays defined on the host)
// and the callers override the result.
SRT_HD void sincos_both(float y, uint32_t top, float& fs, float& fc, int& n_out) {
  double x = (double)((top < 0x42fu) ? y : 0.0f);
  const double r = x * 0x1.45F306DC9C883p+23;
  const int n = ((int32_t)r + 0x800000) >> 24;
  x = x - n * 0x1.921FB54442D18p0;
  const double x2 = x * x;
  const double x3 = x * x2;
  const double s1 = 0x1.1107605230bc4p-7 + x2 * -0x1.994eb3774cf24p-13;
  const double x7 = x3 * x2;
  const double s = x + x3 * -0x1.555545995a603p-3;
  const float ps = (float)(s + x7 * s1);
  const double x4 = x2 * x2;
  const double c2 = -0x1.6c087e89a359dp-10 + x2 * 0x1.99343027bf8c3p-16;
  const double c1 = 0x1p0 + x2 * -0x1.ffffffd0c621cp-2;
  const double x6 = x4 * x2;
  const double c = c1 + x4 * 0x1.55553e1068f19p-5;
  const float pc = (float)(c + x6 * c2);
  fs = u2f(f2u(ps) ^ ((uint32_t)((n + 1) & 2) << 30));    // quadrants 1 and 2: the sine form of -x
  fc = u2f(f2u(pc) ^ ((uint32_t)(n & 2) << 30));          // quadrants 2 and 3: the negated cosine table
  n_out = n;
}
SRT_HD float srt_sincosf(float y, int want_cos) {
  const uint32_t top = (f2u(y) >> 20) & 0x7ffu;
  float fs, fc;
  int n;
  sincos_both(y, top, fs, fc, n);
  float v = (((n ^ want_cos) & 1) == 0) ? fs : fc;
  if (top < 0x398u) v = want_cos ? 1.0f : y;       // |y| < 2^-12
  if (top >= 0x42fu) v = u2f(0x7fc00000u);         // abstop12(120.0f)
  return v;
}
// cosf(y) and sinf(y) together: one sine form and one cosine form of the same operands, whichever way round.
SRT_HD void srt_sincosf2(float y, float& c, float& s) {
  const uint32_t top = (f2u(y) >> 20) & 0x7ffu;
  float fs, fc;
  int n;
  sincos_both(y, top, fs, fc, n);
  const bool odd = (n & 1) != 0;
  c = odd ? fs : fc;
  s = odd ? fc : fs;
  if (top < 0x398u) { c = 1.0f; s = y; }
  if (top >= 0x42fu) c = s = u2f(0x7fc00000u);
}
// ---------------------------------------------------------------------------------------------------
// SRT-MATH v2, atan2f: glibc 2.35 __ieee754_atan2f / __atanf (sysdeps/ieee754/flt-32/e_atan2f.c, s_atanf.c — the
// fdlibm float code), fp32 throughout, no FMA.  Bit-identical to the host libm on 2e8 arguments (random bit
// patterns and the renderer's range); used by Spot_Light::sample (rays/light.cpp:22).
// ---------------------------------------------------------------------------------------------------
SRT_HD float srt_atanf(float x) {
  const float atanhi[4] = {4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f};
  const float atanlo[4] = {5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f};
  const int32_t hx = (int32_t)f2u(x), ix = hx & 0x7fffffff;
  if (ix >= 0x4c000000) {                              // |x| >= 2^25
    if (ix > 0x7f800000) return x + x;                 // NaN
    return (hx > 0) ? (atanhi[3] + atanlo[3]) : (-atanhi[3] - atanlo[3]);
  }
  int id;
  if (ix < 0x3ee00000) {                               // |x| < 0.4375
    if (ix < 0x31000000) return x;                     // |x| < 2^-29
    id = -1;
  } else {
    x = fabsf(x);
    if (ix < 0x3f980000) {                             // |x| < 1.1875
      if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }   // 7/16 <= |x| < 11/16
      else { id = 1; x = (x - 1.0f) / (x + 1.0f); }                        // 11/16 <= |x| < 19/16
    } else {
      if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }   // |x| < 2.4375
      else { id = 3; x = -1.0f / x; }
    }
  }
  const float z = x * x, w = z * z;
  const float s1 = z * (3.3333334327e-01f + w * (1.4285714924e-01f + w * (9.0908870101e-02f + w * (6.6610731184e-02f +
                   w * (4.9768779427e-02f + w * 1.6285819933e-02f)))));
  const float s2 = w * (-2.0000000298e-01f + w * (-1.1111110449e-01f + w * (-7.6918758452e-02f + w * (-5.8335702866e-02f +
                   w * -3.6531571299e-02f))));
  if (id < 0) return x - x * (s1 + s2);
  const float hi = id == 0 ? atanhi[0] : (id == 1 ? atanhi[1] : (id == 2 ? atanhi[2] : atanhi[3]));
  const float lo = id == 0 ? atanlo[0] : (id == 1 ? atanlo[1] : (id == 2 ? atanlo[2] : atanlo[3]));
  const float r = hi - ((x * (s1 + s2) - lo) - x);
  return (hx < 0) ? -r : r;
}

SRT_HD float srt_atan2f(float y, float x) {
  const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f, pi = 3.1415927410e+00f,
              pi_lo = -8.7422776573e-08f;
  const int32_t hx = (int32_t)f2u(x), ix = hx & 0x7fffffff;
  const int32_t hy = (int32_t)f2u(y), iy = hy & 0x7fffffff;
  if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;   // NaN
  if (hx == 0x3f800000) return srt_atanf(y);               // x = 1
  const int32_t m = ((hy >> 31) & 1) | ((hx >> 30) & 2);   // 2 * sign(x) + sign(y)
  if (iy == 0) return (m < 2) ? y : (m == 2 ? pi + tiny : -pi - tiny);
  if (ix == 0) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
  if (ix == 0x7f800000) {
    if (iy == 0x7f800000)
      return m == 0 ? pi_o_4 + tiny : (m == 1 ? -pi_o_4 - tiny : (m == 2 ? 3.0f * pi_o_4 + tiny : -3.0f * pi_o_4 - tiny));
    return m == 0 ? 0.0f : (m == 1 ? -0.0f : (m == 2 ? pi + tiny : -pi - tiny));
  }
  if (iy == 0x7f800000) return (hy < 0) ? -pi_o_2 - tiny : pi_o_2 + tiny;
  const int32_t k = (iy - ix) >> 23;
  float z;
  if (k > 60) z = pi_o_2 + 0.5f * pi_lo;                   // |y / x| > 2^60
  else if (hx < 0 && k < -60) z = 0.0f;                    // |y| / x < -2^60
  else z = srt_atanf(fabsf(y / x));
  if (m == 0) return z;
  if (m == 1) return u2f(f2u(z) ^ 0x80000000u);
  if (m == 2) return pi - (z - pi_lo);
  return (z - pi_lo) - pi;
}

// SRT-MATH v2, acosf: glibc 2.35 __ieee754_acosf (sysdeps/ieee754/flt-32/e_acosf.c, fdlibm's float code), fp32, no FMA.
// Bit-identical to the host libm on 7e8 arguments covering [-1, 1]; used by Samplers::Hemisphere::Uniform.
SRT_HD float srt_acosf(float x) {
  const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
  const int32_t hx = (int32_t)f2u(x), ix = hx & 0x7fffffff;
  if (ix == 0x3f800000) return (hx > 0) ? 0.0f : pi + 2.0f * pio2_lo;
  if (ix > 0x3f800000) return (x - x) / (x - x);
  if (ix < 0x3f000000 && ix <= 0x23000000) return pio2_hi + pio2_lo;       // |x| < 2^-57
  const float z = (ix < 0x3f000000) ? x * x : ((hx < 0) ? (1.0f + x) * 0.5f : (1.0f - x) * 0.5f);
  const float p = z * (1.6666667163e-01f + z * (-3.2556581497e-01f + z * (2.0121252537e-01f + z * (-4.0055535734e-02f +
                  z * (7.9153501429e-04f + z * 3.4793309169e-05f)))));
  const float q = 1.0f + z * (-2.4033949375e+00f + z * (2.0209457874e+00f + z * (-6.8828397989e-01f + z * 7.7038154006e-02f)));
  const float r = p / q;
  if (ix < 0x3f000000) return pio2_hi - (x - (pio2_lo - x * r));           // |x| < 0.5
  const float s = sqrtf(z);
  if (hx < 0) {                                                            // x < -0.5
    const float w = r * s - pio2_lo;
    return pi - 2.0f * (s + w);
  }
  const float df = u2f(f2u(s) & 0xfffff000u);     // x > 0.5
  const float c = (z - df * df) / (s + df);
  const float w = r * s + c;
  return 2.0f * (df + w);
}

SRT_DEV float srt_cosf(float x) { return srt_sincosf(x, 1); }
SRT_DEV float srt_sinf(float x) { return srt_sincosf(x, 0); }
// (float)pow(x, 2) / (float)pow(1 - c, 5) with the float promoted to double (student/bsdf.cpp:17-21,47,150)
SRT_DEV double pow2d(float x) { return (double)x * (double)x; }
SRT_DEV double pow5d(float x) { const double d = (double)x, d2 = d * d, d4 = d2 * d2; return d4 * d; }

// ---------------------------------------------------------------------------------------------------
// SRT-MATH v2, expf / powf: glibc 2.35 e_expf.c / e_powf.c (ARM optimized routines), x86-64 configuration
// (TOINT_INTRINSICS 0: the 0x1.8p52 shift, POWF_SCALE 1), fp64 with one final rounding.  The multiply-adds are fused
// as in glibc's FMA builds (__expf_fma / __powf_fma, what an AVX2 host's ifunc selects): with them the restatement is
// identical to the host libm for every float (expf) and for every normal x at the exponents tried (powf); the
// unfused forms differ for a handful of arguments.  powf: normal x > 0, finite y != 0, NaN otherwise.
// Used by the tone-mapping epilogue only (HDR_Image::tonemap_to, Spectrum::to_srgb).
static __device__ const uint64_t kExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull,
    0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull,
    0x3feedea64c123422ull, 0x3feece086061892dull, 0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull,
    0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull, 0x3feee89f995ad3adull,
    0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
    0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
static __device__ const double kPowfLog2Tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};
SRT_DEV uint64_t dbl_bits(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
SRT_DEV double bits_dbl(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
// 2^(k/32) * 2^r from ki = bits of (k/32-scaled value + shift): table entry plus the exponent bits of ki
SRT_DEV double exp2f_scale(uint64_t ki) { return bits_dbl(kExp2fTab[ki % 32] + (ki << 47)); }
SRT_DEV float srt_expf(float x) {
  const uint32_t ux = __float_as_uint(x), abstop = (ux >> 20) & 0x7ff;
  if (abstop >= 0x42b) {                                 // |x| >= 88 or NaN
    if (ux == 0xff800000u) return 0.0f;
    if (abstop >= 0x7f8) return x + x;
    if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);
    if (x < -0x1.9fe368p6f) return 0.0f;
  }
  const double xd = (double)x, invln2n = 0x1.71547652b82fep+5, shift = 0x1.8p+52;
  const double z = invln2n * xd;
  double kd = z + shift;
  const uint64_t ki = dbl_bits(kd);
  kd -= shift;
  const double r = __builtin_fma(invln2n, xd, -kd);
  const double s = exp2f_scale(ki);
  const double p = __builtin_fma(0x1.c6af84b912394p-20, r, 0x1.ebfce50fac4f3p-13);
  const double r2 = r * r;
  double y = __builtin_fma(0x1.62e42ff0c52d6p-6, r, 1.0);
  y = __builtin_fma(p, r2, y);
  return (float)(y * s);
}
SRT_DEV float srt_powf(float x, float y) {
  const uint32_t ix = __float_as_uint(x), ay = __float_as_uint(y) & 0x7fffffffu;
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u || ay == 0 || ay >= 0x7f800000u) return __uint_as_float(0x7fc00000u);
  const uint32_t tmp = ix - 0x3f330000u;                 // log2_inline: x = 2^k z, z in [OFF, 2 OFF)
  const int i = (int)((tmp >> 19) % 16);
  const uint32_t top = tmp & 0xff800000u;
  const int k = (int32_t)top >> 23;
  const double z = (double)__uint_as_float(ix - top);
  const double r = __builtin_fma(z, kPowfLog2Tab[i][0], -1.0);
  const double y0 = kPowfLog2Tab[i][1] + (double)k;
  const double r2 = r * r;
  double yy = __builtin_fma(0x1.27616c9496e0bp-2, r, -0x1.71969a075c67ap-2);
  const double p = __builtin_fma(0x1.ec70a6ca7baddp-2, r, -0x1.7154748bef6c8p-1);
  const double r4 = r2 * r2;
  double q = __builtin_fma(0x1.71547652ab82bp+0, r, y0);
  q = __builtin_fma(p, r2, q);
  yy = __builtin_fma(yy, r4, q);
  const double ylogx = (double)y * yy;
  if (((dbl_bits(ylogx) >> 47) & 0xffff) >= (dbl_bits(126.0) >> 47)) {
    if (ylogx > 0x1.fffffffd1d571p+6) return __uint_as_float(0x7f800000u);
    if (ylogx <= -150.0) return 0.0f;
  }
  const double shift = 0x1.8p+47;                        // exp2_inline
  double kd = ylogx + shift;
  const uint64_t ki = dbl_bits(kd);
  kd -= shift;
  const double rr = ylogx - kd;
  const double s = exp2f_scale(ki);
  const double pz = __builtin_fma(0x1.c6af84b912394p-5, rr, 0x1.ebfce50fac4f3p-3);
  const double rr2 = rr * rr;
  double o = __builtin_fma(0x1.62e42ff0c52d6p-1, rr, 1.0);
  o = __builtin_fma(pz, rr2, o);
  return (float)(o * s);
}
// Spectrum::to_srgb (lib/spectrum.h:61-66) and the byte conversion of HDR_Image::tonemap_to (util/hdr_image.cpp:181):
// (unsigned char)std::round(v * 255.0f), i.e. on x86-64 cvttss2si and the low byte (0x80000000 when out of range / NaN).
SRT_DEV float to_srgb(float f) {
  if (f < 0.0031308f) return 12.92f * f;
  return 1.055f * srt_powf(f, 1.0f / 2.4f) - 0.055f;
}
SRT_DEV uint32_t srgb_byte(float v) {
  const float r = roundf(v * 255.0f);
  const int32_t i = (r >= -2147483648.0f && r < 2147483648.0f) ? (int32_t)r : INT32_MIN;
  return (uint32_t)i & 0xffu;
}

// ---------------------------------------------------------------------------------------------------
// BBox::hit (student/bbox.cpp:5-62): line/slab test; `times` is only narrowed when tmin/tmax fall inside it.
SRT_DEV bool box_hit(const Node& nd, const Ray& ray, float& tx, float& ty) {
  const float ix = 1.0f / ray.d.x, iy = 1.0f / ray.d.y, iz = 1.0f / ray.d.z;
  const bool sx = ix < 0, sy = iy < 0, sz = iz < 0;
  // bounds as values before the selects (an lvalue select would become a load from a selected address)
  const float mn0 = nd.mn[0], mn1 = nd.mn[1], mn2 = nd.mn[2], mx0 = nd.mx[0], mx1 = nd.mx[1], mx2 = nd.mx[2];
  float tmin = ((sx ? mx0 : mn0) - ray.o.x) * ix;
  float tmax = ((sx ? mn0 : mx0) - ray.o.x) * ix;
  const float tymin = ((sy ? mx1 : mn1) - ray.o.y) * iy;
  const float tymax = ((sy ? mn1 : mx1) - ray.o.y) * iy;
  if ((tmin > tymax) || (tymin > tmax)) return false;
  if (tymin > tmin) tmin = tymin;
  if (tymax < tmax) tmax = tymax;
  const float tzmin = ((sz ? mx2 : mn2) - ray.o.z) * iz;
  const float tzmax = ((sz ? mn2 : mx2) - ray.o.z) * iz;
  if ((tmin > tzmax) || (tzmin > tmax)) return false;
  if (tzmin > tmin) tmin = tzmin;
  if (tzmax < tmax) tmax = tzmax;
  if (tmin >= tx && tmin <= ty) tx = tmin;
  if (tmax >= tx && tmax <= ty) ty = tmax;
  return true;
}

// Triangle::hit (student/tri_mesh.cpp:32-111) on the precomputed {p0, e1, e2}.  Returns hit and, when hit,
// distance = |t*d| and the barycentric triple (u, v, t).
struct TriHit { bool hit; float dist, u, v, t; };
// Straight-line form: every quantity is computed for every lane and the verdict is assembled from the same
// comparisons the reference makes (det != 0; u, v, 1-u-v, t not negative; distance inside dist_bounds).  With
// det == 0 the quotients are inf/NaN and simply unused.  No branches: the three rays of a batch and the
// triangles of a leaf become independent instruction streams the scheduler can interleave.
SRT_DEV TriHit tri_hit(const Tri& g, const Ray& ray) {
  TriHit h;
  const V3 e1 = v3p(g.e1), e2 = v3p(g.e2);
  const V3 s = ray.o - v3p(g.p0);
  const V3 e1xd = cross(e1, ray.d);
  const float det = dot(e1xd, e2);
  const V3 sxe2 = cross(s, e2);
  const float nu = -1.0f * dot(sxe2, ray.d);
  const float nv = dot(e1xd, s);
  const float nt = -1.0f * dot(sxe2, e1);
  h.u = nu / det; h.v = nv / det; h.t = nt / det;
  const bool outside = (h.u < 0) || (h.v < 0) || ((1.0f - h.u - h.v) < 0) || (h.t < 0);
  h.dist = fabsf(norm(ray.d * h.t));
  const bool out_of_bounds = (h.dist < ray.b0) || (h.dist > ray.b1);
  h.hit = (det != 0) && !outside && !out_of_bounds;
  return h;
}

// ---- Triangle::hit's inside / outside verdict from the numerators and det alone ----
// The reference tests  outside = u < 0 || v < 0 || (1 - u - v) < 0 || t < 0  on the rounded quotients u = RN(nu / det),
// v = RN(nv / det), t = RN(nt / det).  A caller that reads only {hit, dist, t} needs u and v for nothing else, and for all but a
// vanishing share of (ray, triangle) pairs the first three tests follow exactly from nu, nv and det.  Precondition (div_window):
// every operand is a NaN or has a magnitude in [2^-40, 2^40]; nt may also be exactly zero.  Write x = nu / det, y = nv / det
// for the exact quotients and e = 2^-24 (the unit round-off; nothing here underflows: |x|, |y| >= 2^-80).
//  * u < 0  <=>  nu * det < 0.  A non-zero quotient of magnitude >= 2^-80 never rounds to zero, so u has the sign of x; the
//    product (magnitude in [2^-80, 2^80]) has it too.  A NaN makes both sides false.  The same for v.  (t is computed anyway
//    and tested as it is.)
//  * Given x, y > 0, the third test is  RN(RN(1 - u) - v) < 0  <=>  p < v  with p = RN(1 - u): the difference of two floats
//    is a multiple of the smaller one's ulp, so it is zero or rounds to a non-zero float of its own sign.  Also
//    |p - (1 - u)| <= e / 2 while u <= 1 (1 - u lies in [0, 1]), p <= 0 < v once u >= 1, u and v are within a factor
//    (1 +- e) of x and y.  The test below compares s = |RN(nu + nv)| = |det| (x + y)(1 + d1), |d1| <= e, with
//    RN(|det| (1 +- 2^-20)) = |det| (1 +- 2^-20)(1 + d2), |d2| <= e (the two constants are floats):
//      s > RN(|det| (1 + 2^-20))  =>  x + y > (1 + 2^-20)(1 - e) / (1 + e) > 1 + 2^-21.  Then, for u < 1,
//        p - v <= 1 - (x + y)(1 - e) + e / 2 < 1 - (1 + 2^-22) + 2^-25 < 0: outside, for certain.
//      s < RN(|det| (1 - 2^-20))  =>  x + y < (1 - 2^-20)(1 + e) / (1 - e) < 1 - 2^-21, so u < 1 and
//        p - v >= 1 - (x + y)(1 + e) - e / 2 > 2^-21 - 2^-24 - 2^-25 > 0: not outside, for certain.
//    2^-20 leaves a factor 8 over what the errors need.  Between the two bounds the lane is AMBIGUOUS (about one pair in 10^6 of
//    a rendered scene); a NaN among nu, nv, det fails both comparisons and lands there as well, unless u < 0 or v < 0 has
//    already decided.  The caller then computes u and v and makes the reference's own comparisons.
// Plain C++ (no device builtins): tests/host_emu runs the same function on the CPU.
struct TriVerdict { bool outside, ambiguous; };
SRT_DEV TriVerdict tri_verdict(float nu, float nv, float det) {
  const bool neg = (nu * det < 0) | (nv * det < 0);
  const float s = fabsf(nu + nv), a = fabsf(det);
  const bool beyond = s > a * (1.0f + 0x1p-20f), within = s < a * (1.0f - 0x1p-20f);
  TriVerdict v;
  v.outside = neg | beyond;                // of the first three tests
  v.ambiguous = !(neg | beyond | within);
  return v;
}

// ---- One quotient and one root per ray and leaf: the candidate of the ordered fold ----
// The fold over a leaf's triangles (ret = Trace::min(ret, Triangle::hit), object_testN in pt_wave.h) reads {hit, dist, t} of every
// triangle and keeps those of one.  hit implies "not outside", and by the proof above the first three tests of "outside" follow
// from the numerators for every lane that is in the window and not ambiguous.  So while every (ray, triangle) pair of a leaf is
// decided that way, a ray with at most ONE triangle that is not outside - its candidate - can be hit by no other triangle of the
// leaf, whatever their t and distance would have been: every other Trace::min step has a miss on the right and keeps the left
// side, and the fold returns the candidate's own {hit, dist, t}, or the default Trace (no hit: dist = t = 0) when the candidate
// fails t < 0 or the dist_bounds, or when there is none.  t and the distance are then computed once, for the candidate, by the
// operations tri_hitN performs on the same operands - the same bits.  A lane is BAD, and its wave folds the leaf the long way,
// when any of this does not hold: a pair out of the window (det == 0 is), an ambiguous pair (a NaN among nu, nv, det is, unless
// a sign decided first, as in tri_hitN), or a second candidate (two coplanar triangles of a wall: only a ray through the shared
// edge to within rounding; a closed mesh in one leaf: every ray through it).
// Plain C++ (no device builtins): tests/host_emu runs the same functions on the CPU.
struct LeafCand { float det, nt; uint32_t n; };       // n: the candidate's triangle index + 1, 0 = none (then det = 1, nt = 0: t = 0)
SRT_DEV LeafCand leaf_cand_none() { LeafCand c; c.det = 1.0f; c.nt = 0.0f; c.n = 0u; return c; }
// One (ray, triangle) pair; returns "bad" of this pair apart from the window, which the caller tests per lane (div_in_range).
SRT_DEV bool leaf_cand_add(LeafCand& c, float nu, float nv, float det, float nt, uint32_t n) {
  const TriVerdict v = tri_verdict(nu, nv, det);
  const bool cand = !v.outside;
  const bool bad = v.ambiguous | (cand & (c.n != 0u));
  c.det = cand ? det : c.det;
  c.nt = cand ? nt : c.nt;
  c.n = cand ? n : c.n;
  return bad;
}

// Triangle::hit of one triangle for the N rays of a batch (shared origin), for a caller that folds hits (Trace::min): hit,
// distance and t, no barycentrics.  s, s x e2 and the numerator of t do not depend on the direction.  Inside div_window and
// with no ambiguous lane in the wave (tri_verdict) only t is divided, through the shared-reciprocal refinement; with one, the
// wave computes u and v as well and compares them as the reference does (*fallback, when given, is set: wave-uniform).
// Outside the window, and with SRT_PLAIN_DIV_SQRT, everything is the compiler's own `/`.  The N distances go through sqrtN.
struct TriHitT { bool hit; float dist, t; };
template <int N>
SRT_DEV void tri_hitN(const Tri& g, V3 org, const V3* d, const float* b0, const float* b1, TriHitT* h, bool* fallback = nullptr) {
  const V3 e1 = v3p(g.e1), e2 = v3p(g.e2);
  const V3 s = org - v3p(g.p0);
  const V3 sxe2 = cross(s, e2);
  const float nt = -1.0f * dot(sxe2, e1);
  float num[N][3], det[N], t[N], n2[N], nr[N];
  bool outside[N];
#pragma unroll
  for (int r = 0; r < N; r++) {
    const V3 e1xd = cross(e1, d[r]);
    det[r] = dot(e1xd, e2);
    num[r][0] = -1.0f * dot(sxe2, d[r]);
    num[r][1] = dot(e1xd, s);
    num[r][2] = nt;
  }
  bool decided = false;                         // wave-uniform
#if SRT_EXACT_FAST_PATHS
  // one ballot for both conditions: a lane out of the window or an ambiguous one sends the wave the long way
  bool amb = !div_in_range<N, true>(num, det);
#pragma unroll
  for (int r = 0; r < N; r++) {
    const TriVerdict v = tri_verdict(num[r][0], num[r][1], det[r]);
    outside[r] = v.outside;
    amb = amb | v.ambiguous;
  }
  if (__ballot(amb) == 0ull) {
#pragma unroll
    for (int r = 0; r < N; r++) {
      t[r] = __builtin_amdgcn_div_fixupf(div_refine(nt, det[r], rcp_refined(det[r])), det[r], nt);
      outside[r] = outside[r] | (t[r] < 0);
    }
    decided = true;
  } else if (fallback) {
    *fallback = div_window<N, true>(num, det);   // in the window: an ambiguous lane it was
  }
#endif
  if (!decided) {
    float q[N][3];
    divNx3<N, true>(num, det, q);
#pragma unroll
    for (int r = 0; r < N; r++) {
      t[r] = q[r][2];
      outside[r] = (q[r][0] < 0) || (q[r][1] < 0) || ((1.0f - q[r][0] - q[r][1]) < 0) || (t[r] < 0);
    }
  }
#pragma unroll
  for (int r = 0; r < N; r++) n2[r] = norm2(d[r] * t[r]);
  const bool on_plane = nt == 0.0f;             // t = +-0 for every ray: the distances are exactly +0
  bool zero[N];
#pragma unroll
  for (int r = 0; r < N; r++) zero[r] = on_plane;
  sqrtN<N>(n2, zero, nr);
#pragma unroll
  for (int r = 0; r < N; r++) {
    h[r].t = t[r];
    h[r].dist = fabsf(nr[r]);
    const bool out_of_bounds = (h[r].dist < b0[r]) || (h[r].dist > b1[r]);
    h[r].hit = (det[r] != 0) & !outside[r] & !out_of_bounds;       // (no short-circuit: masks, not branches)
  }
}

// The ordered fold over the triangles of one leaf (<= 4 triangles, or a List<Triangle>) for the NR rays of a batch:
// ret = Trace::min(ret, hit) per triangle, triangles tris[first .. first + ntri).  Out: bd = distance, bt = t, bn = index of the
// winning triangle + 1 (0 = no hit, then bd = bt = 0: the default Trace).
// The long way, one tri_hitN per triangle.  A miss changes nothing: left_wins(l, ., false, .) == l, so either the left side
// is kept or both sides are misses and the fields already hold the default Trace (no hit => bd = bt = 0, true before the
// loop and kept by every step).  Only a hit that is not beaten (ldist < rdist is false on NaN: the right side wins) is
// taken: one mask and one select per field.  "hit so far" is carried as bn != 0, bn = winning triangle's index + 1: a flag
// of its own lives in a register across the loop and costs three more instructions per ray and triangle.
template <int NR>
SRT_DEV void leaf_fold_longN(const Tri* __restrict__ tris, uint32_t first, uint32_t ntri, V3 oorg, const V3* od, const float* ob0,
                             const float* ob1, float* bd, float* bt, uint32_t* bn) {
#pragma unroll
  for (int r = 0; r < NR; r++) { bd[r] = 0.0f; bt[r] = 0.0f; bn[r] = 0u; }
  for (uint32_t t = 0; t < ntri; t++) {
    TriHitT th[NR];
    tri_hitN<NR>(tris[first + t], oorg, od, ob0, ob1, th);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      const bool take = th[r].hit & !((bn[r] != 0u) & (bd[r] < th[r].dist));   // == th.hit && !left_wins(bh, bd, th.hit, th.dist)
      bd[r] = take ? th[r].dist : bd[r];
      bt[r] = take ? th[r].t : bt[r];
      bn[r] = take ? first + t + 1u : bn[r];
    }
  }
}
// The fold as object_testN (pt_wave.h) runs it (ONCE): a candidate pass over the leaf (leaf_cand_add above, where the proof stands) -
// per triangle the numerators and det exactly as tri_hitN forms them, no division, no root, no ballot -, then ONE ballot on "a
// lane is bad".  Without a bad lane every (ray, triangle) pair is decided from its numerators and every ray has at most one
// triangle that is not outside, so no other triangle of the leaf can be hit and the ordered fold returns that candidate's own
// test: one quotient t (the operations of tri_hitN's decided path on the same operands), one norm2(d * t), one sqrtN call, the
// bounds.  Lanes without a candidate compute on det = 1, nt = 0 (t = 0, distance +0) and report the default Trace, as does a
// candidate that fails t < 0 or the bounds.
// A wave with a bad lane (*fellback is set, when given: wave-uniform) folds the leaf with the plain per-ray tri_hit - the
// compiler's own `/` and sqrtf, whose {hit, dist, t} tri_hitN equals bit for bit on every input (tests/test_pt_tri_verdict_gpu.py) -
// one RAY after the other, the triangles in the inner loop: the cold path then needs the registers of one plain test and
// nothing of it is alive across the candidate pass.  How the cold path is attached decides the kernel's scratch (DESIGN.md
// section 6 has the table of forms); ONCE = false keeps the long way for the two kernel forms this form costs scratch.
template <int NR, bool ONCE>
SRT_DEV void leaf_foldN(const Tri* __restrict__ tris, uint32_t first, uint32_t ntri, V3 oorg, const V3* od, const float* ob0,
                        const float* ob1, float* bd, float* bt, uint32_t* bn, bool* fellback = nullptr) {
#if SRT_EXACT_FAST_PATHS
  if (ONCE) {
    LeafCand c[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) c[r] = leaf_cand_none();
    bool bad = false;
    for (uint32_t t = 0; t < ntri; t++) {
      const Tri& g = tris[first + t];
      const V3 e1 = v3p(g.e1), e2 = v3p(g.e2);
      const V3 s = oorg - v3p(g.p0);
      const V3 sxe2 = cross(s, e2);
      const float nt = -1.0f * dot(sxe2, e1);
      float num[NR][3], det[NR];
#pragma unroll
      for (int r = 0; r < NR; r++) {
        const V3 e1xd = cross(e1, od[r]);
        det[r] = dot(e1xd, e2);
        num[r][0] = -1.0f * dot(sxe2, od[r]);
        num[r][1] = dot(e1xd, s);
        num[r][2] = nt;
      }
      bad = bad | !div_in_range<NR, true>(num, det);
#pragma unroll
      for (int r = 0; r < NR; r++) bad = bad | leaf_cand_add(c[r], num[r][0], num[r][1], det[r], nt, first + t + 1u);
    }
    if (__ballot(bad) == 0ull) {
      float tq[NR], n2[NR], nr[NR];
      bool zero[NR];
#pragma unroll
      for (int r = 0; r < NR; r++) {
        tq[r] = __builtin_amdgcn_div_fixupf(div_refine(c[r].nt, c[r].det, rcp_refined(c[r].det)), c[r].det, c[r].nt);
        n2[r] = norm2(od[r] * tq[r]);
        zero[r] = c[r].nt == 0.0f;                // the origin on the candidate's plane, or no candidate: exactly +0
      }
      sqrtN<NR>(n2, zero, nr);
#pragma unroll
      for (int r = 0; r < NR; r++) {
        const float dist = fabsf(nr[r]);
        const bool hit = (c[r].n != 0u) & !(tq[r] < 0) & !((dist < ob0[r]) | (dist > ob1[r]));
        bd[r] = hit ? dist : 0.0f;
        bt[r] = hit ? tq[r] : 0.0f;
        bn[r] = hit ? c[r].n : 0u;
      }
      return;
    }
    if (fellback) *fellback = true;
#pragma unroll
    for (int r = 0; r < NR; r++) {
      Ray ray; ray.o = oorg; ray.d = od[r]; ray.b0 = ob0[r]; ray.b1 = ob1[r];
      float fd = 0.0f, ft = 0.0f;
      uint32_t fn = 0u;
#pragma nounroll
      for (uint32_t t = 0; t < ntri; t++) {
        const TriHit th = tri_hit(tris[first + t], ray);
        const bool take = th.hit & !((fn != 0u) & (fd < th.dist));
        fd = take ? th.dist : fd;
        ft = take ? th.t : ft;
        fn = take ? first + t + 1u : fn;
      }
      bd[r] = fd; bt[r] = ft; bn[r] = fn;
    }
    return;
  }
#endif
  leaf_fold_longN<NR>(tris, first, ntri, oorg, od, ob0, ob1, bd, bt, bn);
}

// Triangle::hit of the (up to) four triangles of a BVH<Triangle> leaf for ONE ray: the twelve quotients and four
// distances go through divNx3 / sqrtN together (one range verdict, independent refinement chains).  Same arithmetic per
// triangle as tri_hit.
template <int N>
SRT_DEV void tri_hit_leafN(const Tri* g, const Ray& ray, TriHit* h) {
  float num[N][3], det[N], q[N][3], n2[N], nr[N];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const V3 e1 = v3p(g[k].e1), e2 = v3p(g[k].e2);
    const V3 s = ray.o - v3p(g[k].p0);
    const V3 e1xd = cross(e1, ray.d);
    det[k] = dot(e1xd, e2);
    const V3 sxe2 = cross(s, e2);
    num[k][0] = -1.0f * dot(sxe2, ray.d);
    num[k][1] = dot(e1xd, s);
    num[k][2] = -1.0f * dot(sxe2, e1);
  }
  divNx3<N, false>(num, det, q);
  bool zero[N];
#pragma unroll
  for (int k = 0; k < N; k++) { n2[k] = norm2(ray.d * q[k][2]); zero[k] = false; }
  sqrtN<N>(n2, zero, nr);
#pragma unroll
  for (int k = 0; k < N; k++) {
    h[k].u = q[k][0]; h[k].v = q[k][1]; h[k].t = q[k][2];
    const bool outside = (h[k].u < 0) || (h[k].v < 0) || ((1.0f - h[k].u - h[k].v) < 0) || (h[k].t < 0);
    h[k].dist = fabsf(nr[k]);
    const bool out_of_bounds = (h[k].dist < ray.b0) || (h[k].dist > ray.b1);
    h[k].hit = (det[k] != 0) && !outside && !out_of_bounds;
  }
}
SRT_DEV void tri_hit_leaf4(const Tri* g, const Ray& ray, TriHit* h) { tri_hit_leafN<4>(g, ray, h); }

// Sphere::hit (student/shapes.cpp:17-80).  The reference's unqualified sqrt(delta) is the double overload,
// so the numerator sum and the quotient are fp64 before narrowing to t1/t2.  Straight-line form as above.
struct SphHit { bool hit; float t; };
// The delta > 0 branch (two roots): delta itself, "a root is valid" and the root the reference returns (0 without one).
SRT_DEV float sphere_two_roots(float radius, const Ray& ray, bool& hit_two, float& t_two) {
  const float a = norm2(ray.d);
  const float b = 2.0f * dot(ray.o, ray.d);
  const float c = norm2(ray.o) - radius * radius;
  const float delta = b * b - 4.0f * a * c;
  const double m2od = (double)((-2.0f) * dot(ray.o, ray.d));
  const double sq = sqrt((double)delta);
  const double den = (double)(2.0f * norm2(ray.d));
  const float t1 = (float)((m2od + sq) / den);
  const float t2 = (float)((m2od - sq) / den);
  bool v1 = !(t1 < 0), v2 = !(t2 < 0);
  const float d1 = fabsf(norm(ray.d * t1));
  const float d2 = fabsf(norm(ray.d * t2));
  v1 = v1 && !(d1 < ray.b0 || d1 > ray.b1);
  v2 = v2 && !(d2 < ray.b0 || d2 > ray.b1);
  hit_two = v1 || v2;
  t_two = hit_two ? ((v1 && v2) ? std_min(t1, t2) : (v1 ? t1 : t2)) : 0.0f;
  return delta;
}
// delta == 0: tangent, no validity checks in the reference
SRT_DEV float sphere_tangent_root(const Ray& ray) { return ((-2.0f) * dot(ray.o, ray.d)) / (2.0f * norm2(ray.d)); }
SRT_DEV SphHit sphere_hit(float radius, const Ray& ray) {
  SphHit h;
  bool hit_two;
  float t_two;
  const float delta = sphere_two_roots(radius, ray, hit_two, t_two);
  const float t_one = sphere_tangent_root(ray);
  const bool two = delta > 0, one = delta == 0;
  h.hit = (two & hit_two) | one;                     // == two ? hit_two : one (delta == 0 excludes delta > 0), without a bool select
  h.t = two ? t_two : (one ? t_one : 0.0f);
  return h;
}
// Sphere::hit for the N rays of a batch (shared origin), wave-uniformly: the tangent root (a full divide that only a lane with
// delta == 0 reads) is computed when some lane of the wave has such a ray, which is next to never (*tangent, when given, is set
// then: wave-uniform).
template <int N>
SRT_DEV void sphere_hitN(float radius, V3 org, const V3* d, const float* b0, const float* b1, SphHit* h, bool* tangent = nullptr) {
  Ray ray[N];
  bool one[N], any_one = false;
#pragma unroll
  for (int r = 0; r < N; r++) {
    ray[r].o = org; ray[r].d = d[r]; ray[r].b0 = b0[r]; ray[r].b1 = b1[r];
    bool hit_two;
    float t_two;
    const float delta = sphere_two_roots(radius, ray[r], hit_two, t_two);
    const bool two = delta > 0;
    one[r] = delta == 0;
    any_one = any_one | one[r];
    h[r].hit = (two & hit_two) | one[r];               // == two ? hit_two : one[r] (delta == 0 excludes delta > 0), without a bool select
    h[r].t = two ? t_two : 0.0f;
  }
  if (__ballot(any_one) != 0ull) {
#pragma unroll
    for (int r = 0; r < N; r++) h[r].t = one[r] ? sphere_tangent_root(ray[r]) : h[r].t;
    if (tangent) *tangent = true;
  }
}

// Mat4::rotate_to (lib/mat4.h:353-367): columns x, dir, z of the shading frame.
struct Frame { V3 x, y, z; };
SRT_DEV Frame rotate_to(V3 dir) {
  const float n = norm(dir);
  dir.x /= n; dir.y /= n; dir.z /= n;
  Frame f;
  if (fabsf(dir.y - 1.0f) < kEps) { f.x = v3(1, 0, 0); f.y = v3(0, 1, 0); f.z = v3(0, 0, 1); return f; }
  if (fabsf(dir.y + 1.0f) < kEps) { f.x = v3(1, 0, 0); f.y = v3(0, -1, 0); f.z = v3(0, 0, 1); return f; }
  f.x = unit(cross(dir, v3(0.0f, 1.0f, 0.0f)));
  f.z = unit(cross(f.x, dir));
  f.y = dir;
  return f;
}
// object_to_world.rotate(v): v.x*col0 + v.y*col1 + v.z*col2 + 0*col3 (col3 = (0,0,0,1))
SRT_DEV V3 frame_to_world(const Frame& f, V3 v) {
  return v3(((f.x.x * v.x + f.y.x * v.y) + f.z.x * v.z) + 0.0f * 0.0f,
            ((f.x.y * v.x + f.y.y * v.y) + f.z.y * v.z) + 0.0f * 0.0f,
            ((f.x.z * v.x + f.y.z * v.y) + f.z.z * v.z) + 0.0f * 0.0f);
}
// world_to_object = object_to_world.T(); its columns are (x.x, y.x, z.x, 0) ...
SRT_DEV V3 frame_to_local(const Frame& f, V3 v) {
  return v3(((f.x.x * v.x + f.x.y * v.y) + f.x.z * v.z) + 0.0f * 0.0f,
            ((f.y.x * v.x + f.y.y * v.y) + f.y.z * v.z) + 0.0f * 0.0f,
            ((f.z.x * v.x + f.z.y * v.y) + f.z.z * v.z) + 0.0f * 0.0f);
}

}  // namespace srt

#endif
