// The test-only math probes of include/srt_pt_debug.h: each runs one piece of the device arithmetic (pt_device.h, pt_trace.h) on
// caller-supplied operands, so that a test can compare it with the host's libm or with the plain per-ray form.  No scene, no render.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "pt_anim.h"
#include "pt_context.h"
#include "pt_device.h"
#include "srt_pt_debug.h"

#include "pt_trace.h"

namespace srt {

__global__ void pt_math_kernel(const float* __restrict__ x, size_t n, float* __restrict__ c, float* __restrict__ s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { c[i] = srt_cosf(x[i]); s[i] = srt_sinf(x[i]); }
}

// srt_sincosf2: no bounds guard around the call, so that every wave runs it with all 64 lanes (the spares repeat the last argument)
__global__ void pt_sincos2_kernel(const float* __restrict__ x, size_t n, float* __restrict__ c, float* __restrict__ s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float cv, sv;
  srt_sincosf2(x[i < n ? i : n - 1], cv, sv);
  if (i < n) { c[i] = cv; s[i] = sv; }
}

__global__ void pt_acos_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = srt_acosf(x[i]);
}

__global__ void pt_sin_unit_kernel(const float* __restrict__ x, size_t n, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = srt_sin_unit(x[i]);
}

// Samplers::Sphere::Image through the render's own device functions (pt_trace.h): lane i < nu bisects u[i] and forms the direction,
// lane nu + j evaluates pdf() of direction j.
__global__ void pt_env_sampler_kernel(DScene S, const float* __restrict__ u, size_t nu, uint32_t* __restrict__ index_out, float* __restrict__ dir_out,
                                      const float* __restrict__ dirs, size_t nd, float* __restrict__ pdf_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nu) {
    const uint32_t index = env_image_upper_bound(S, u[i]);
    const V3 d = env_image_direction(S, index);
    index_out[i] = index;
    dir_out[3 * i] = d.x; dir_out[3 * i + 1] = d.y; dir_out[3 * i + 2] = d.z;
  } else if (i - nu < nd) {
    const size_t j = i - nu;
    pdf_out[j] = env_image_pdf(S, v3(dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]));
  }
}

__global__ void pt_atan2_kernel(const float* __restrict__ y, const float* __restrict__ x, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = srt_atan2f(y[i], x[i]);
}

__global__ void pt_exp_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = srt_expf(x[i]);
}
__global__ void pt_pow_kernel(const float* __restrict__ x, const float* __restrict__ y, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = srt_powf(x[i], y[i]);
}

// Diagnostic for divNx3 / sqrtN (pt_device.h): lane i takes the operands of "rays" 3i, 3i+1, 3i+2 — exactly how the
// wave kernel's batch tests call them.  io layout: planes of n3 = 3 * lanes floats: num0, num1, num2, den, x in; q0, q1, q2,
// root out.  shared_c2: column 2's numerator of a lane is num2[3i] for its three rays (the triangle test's shared t numerator).
__global__ void pt_div_sqrt_kernel(const float* __restrict__ in, size_t lanes, int shared_c2, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n3 = lanes * 3;
  const size_t k = (i < lanes ? i : lanes - 1) * 3;     // every lane of the last wave computes; the spares repeat the last lane
  float num[3][3], den[3], q[3][3], x[3], root[3];
  bool zero[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    num[r][0] = in[k + r]; num[r][1] = in[n3 + k + r];
    num[r][2] = in[2 * n3 + (shared_c2 ? k : k + r)];
    den[r] = in[3 * n3 + k + r];
    x[r] = in[4 * n3 + k + r];
    zero[r] = __float_as_uint(x[r]) == 0u;
  }
  if (shared_c2) divNx3<3, true>(num, den, q); else divNx3<3, false>(num, den, q);
  sqrtN<3>(x, zero, root);
  if (i < lanes) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      out[k + r] = q[r][0]; out[n3 + k + r] = q[r][1]; out[2 * n3 + k + r] = q[r][2];
      out[3 * n3 + k + r] = root[r];
    }
  }
}

// Triangle::hit of the wave kernel's fold (tri_hitN<3>: verdict from the numerators, only t divided) next to the plain per-ray
// form (tri_hit), lane i on its own triangle, origin and three rays.  in: 27 planes of `lanes` floats (p0, e1, e2, origin, three
// directions, then b0 and b1 of the three rays); out: 19 planes - {hit, t, dist} x 3 rays of the batch form, the same of
// tri_hit, and "this lane's wave computed u and v after all" (an ambiguous lane in it).
__global__ void pt_tri_verdict_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t k = i < lanes ? i : lanes - 1;           // every lane of the last wave computes; the spares repeat the last lane
  float v[27];
#pragma unroll
  for (int j = 0; j < 27; j++) v[j] = in[(size_t)j * lanes + k];
  Tri g;
#pragma unroll
  for (int j = 0; j < 3; j++) { g.p0[j] = v[j]; g.e1[j] = v[3 + j]; g.e2[j] = v[6 + j]; }
  const V3 org = v3(v[9], v[10], v[11]);
  V3 d[3];
  float b0[3], b1[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { d[r] = v3(v[12 + 3 * r], v[13 + 3 * r], v[14 + 3 * r]); b0[r] = v[21 + r]; b1[r] = v[24 + r]; }
  TriHitT hb[3];
  bool fallback = false;
  tri_hitN<3>(g, org, d, b0, b1, hb, &fallback);
  if (i < lanes) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      Ray ray; ray.o = org; ray.d = d[r]; ray.b0 = b0[r]; ray.b1 = b1[r];
      const TriHit hp = tri_hit(g, ray);
      out[(size_t)(3 * r) * lanes + i] = hb[r].hit ? 1.0f : 0.0f;
      out[(size_t)(3 * r + 1) * lanes + i] = hb[r].t;
      out[(size_t)(3 * r + 2) * lanes + i] = hb[r].dist;
      out[(size_t)(9 + 3 * r) * lanes + i] = hp.hit ? 1.0f : 0.0f;
      out[(size_t)(10 + 3 * r) * lanes + i] = hp.t;
      out[(size_t)(11 + 3 * r) * lanes + i] = hp.dist;
    }
    out[(size_t)18 * lanes + i] = fallback ? 1.0f : 0.0f;
  }
}

// The leaf fold of the wave kernel's mesh branch (leaf_foldN<3, true>, pt_device.h: one candidate, one quotient and one root per ray)
// next to the plain ordered fold over tri_hit, one leaf per wave (64 consecutive lanes), lane i on its own origin and three rays.
// in: per wave 148 floats - the triangle count as a 32-bit integer, three unused words, twelve Tri records (p0, e1, e2 as xyz + pad) -
// then 18 planes of `lanes` floats (origin, three directions, then b0 and b1 of the three rays); out: 25 planes - per ray
// {hit as 0 / 1, winning triangle as a 32-bit integer, t, dist} of the leaf code, the same four of the plain fold, and "this lane's
// wave met a bad lane and folded the leaf the long way".  lanes is a multiple of 64 and every count in 1..12 (checked by the caller).
constexpr size_t kLeafFoldWave = 4 + 12 * sizeof(Tri) / sizeof(float);
__global__ void pt_leaf_fold_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;                               // whole waves
  const float* leaf = in + (i / 64) * kLeafFoldWave;
  const uint32_t ntri = (uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(leaf[0]));
  const Tri* tris = reinterpret_cast<const Tri*>(leaf + 4);
  const float* planes = in + (lanes / 64) * kLeafFoldWave;
  float v[18];
#pragma unroll
  for (int j = 0; j < 18; j++) v[j] = planes[(size_t)j * lanes + i];
  const V3 org = v3(v[0], v[1], v[2]);
  V3 d[3];
  float b0[3], b1[3], bd[3], bt[3];
  uint32_t bn[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { d[r] = v3(v[3 + 3 * r], v[4 + 3 * r], v[5 + 3 * r]); b0[r] = v[12 + r]; b1[r] = v[15 + r]; }
  bool fellback = false;
  leaf_foldN<3, true>(tris, 0u, ntri, org, d, b0, b1, bd, bt, bn, &fellback);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    Ray ray; ray.o = org; ray.d = d[r]; ray.b0 = b0[r]; ray.b1 = b1[r];
    bool ph = false;                                    // ret = Trace::min(ret, Triangle::hit), as Trace::min is written
    float pd = 0.0f, ptt = 0.0f;
    uint32_t pn = 0u;
    for (uint32_t t = 0; t < ntri; t++) {
      const TriHit h = tri_hit(tris[t], ray);
      const bool left = ph && (!h.hit || pd < h.dist);
      if (!left && h.hit) { ph = true; pd = h.dist; ptt = h.t; pn = t; }
    }
    const bool hit = bn[r] != 0u;
    out[(size_t)(8 * r) * lanes + i] = hit ? 1.0f : 0.0f;
    out[(size_t)(8 * r + 1) * lanes + i] = __uint_as_float(hit ? bn[r] - 1u : 0u);
    out[(size_t)(8 * r + 2) * lanes + i] = bt[r];
    out[(size_t)(8 * r + 3) * lanes + i] = bd[r];
    out[(size_t)(8 * r + 4) * lanes + i] = ph ? 1.0f : 0.0f;
    out[(size_t)(8 * r + 5) * lanes + i] = __uint_as_float(pn);
    out[(size_t)(8 * r + 6) * lanes + i] = ptt;
    out[(size_t)(8 * r + 7) * lanes + i] = pd;
  }
  out[(size_t)24 * lanes + i] = fellback ? 1.0f : 0.0f;
}

// Sphere::hit of the wave kernel's batch (sphere_hitN<3> and the distance step through sqrtN, as object_testN's sphere branch in
// pt_wave.h performs them - restated below, since moving the branch into a function of its own changed a wave kernel's scratch)
// next to the plain per-ray form (sphere_hit, then the distance as object_hit has it, pt_trace.h), lane i on its own radius,
// origin and three rays.  in: 19 planes of `lanes` floats (radius, origin, three directions, then b0 and b1 of the three
// rays); out: 22 planes - {hit, t, dist} x 3 rays of the batch form, the same of the plain form, delta of the three rays
// (sphere_two_roots), and "this lane's wave computed the tangent root" (a lane with delta == 0 in it).
__global__ void pt_sphere_batch_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t k = i < lanes ? i : lanes - 1;           // every lane of the last wave computes; the spares repeat the last lane
  float v[19];
#pragma unroll
  for (int j = 0; j < 19; j++) v[j] = in[(size_t)j * lanes + k];
  const float radius = v[0];
  const V3 org = v3(v[1], v[2], v[3]);
  V3 d[3], pos[3];
  float b0[3], b1[3], tb[3], db[3];
  bool hb[3];
#pragma unroll
  for (int r = 0; r < 3; r++) { d[r] = v3(v[4 + 3 * r], v[5 + 3 * r], v[6 + 3 * r]); b0[r] = v[13 + r]; b1[r] = v[16 + r]; }
  bool tangent = false;
  {                                                     // the sphere branch of object_testN (pt_wave.h), line for line: change both
    constexpr int NR = 3;
    SphHit sh[NR];
    sphere_hitN<NR>(radius, org, d, b0, b1, sh, &tangent);
#pragma unroll
    for (int r = 0; r < NR; r++) {
      hb[r] = sh[r].hit; tb[r] = sh[r].t;
      pos[r] = org + d[r] * sh[r].t;                    // Ray::at
    }
    float n2[NR], nr[NR];
    bool miss[NR];                                      // no hit: t = 0, pos == origin
#pragma unroll
    for (int r = 0; r < NR; r++) { n2[r] = norm2(pos[r] - org); miss[r] = !hb[r]; }
    sqrtN<NR>(n2, miss, nr);
#pragma unroll
    for (int r = 0; r < NR; r++) db[r] = fabsf(nr[r]);
  }
  if (i < lanes) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
      Ray ray; ray.o = org; ray.d = d[r]; ray.b0 = b0[r]; ray.b1 = b1[r];
      const SphHit hp = sphere_hit(radius, ray);
      bool hit_two;
      float t_two;
      const float delta = sphere_two_roots(radius, ray, hit_two, t_two);
      out[(size_t)(3 * r) * lanes + i] = hb[r] ? 1.0f : 0.0f;
      out[(size_t)(3 * r + 1) * lanes + i] = tb[r];
      out[(size_t)(3 * r + 2) * lanes + i] = db[r];
      out[(size_t)(9 + 3 * r) * lanes + i] = hp.hit ? 1.0f : 0.0f;
      out[(size_t)(10 + 3 * r) * lanes + i] = hp.t;
      out[(size_t)(11 + 3 * r) * lanes + i] = fabsf(norm(ray_at(ray, hp.t) - ray.o));
      out[(size_t)(18 + r) * lanes + i] = delta;
    }
    out[(size_t)21 * lanes + i] = tangent ? 1.0f : 0.0f;
  }
}

// BBox::hit of the sweeps (box_hit_inv: both products per axis, the select on the results) next to the form of the per-lane
// traversals (box_hit_rec: the bound selected first; both in pt_trace.h), lane i on its own box, origin, reciprocal direction
// and incoming `times`.  in: 14 planes of `lanes` floats (box min xyz, box max xyz, origin xyz, 1 / direction xyz, times x, y);
// out: 6 planes - {hit as 0 / 1, times.x, times.y} of box_hit_inv, then the same of box_hit_rec.
__global__ void pt_box_sweep_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;
  float v[14];
#pragma unroll
  for (int j = 0; j < 14; j++) v[j] = in[(size_t)j * lanes + i];
  const float bx[6] = {v[0], v[1], v[2], v[3], v[4], v[5]};
  const V3 org = v3(v[6], v[7], v[8]), inv = v3(v[9], v[10], v[11]);
  float ax = v[12], ay = v[13], bxx = v[12], bxy = v[13];
  const bool ha = box_hit_inv(bx, org, inv, ax, ay);
  const bool hb = box_hit_rec(bx, org, inv, bxx, bxy);
  out[i] = ha ? 1.0f : 0.0f; out[lanes + i] = ax; out[2 * lanes + i] = ay;
  out[3 * lanes + i] = hb ? 1.0f : 0.0f; out[4 * lanes + i] = bxx; out[5 * lanes + i] = bxy;
}

// Mat4 * Vec3 of the leaf section's point transforms (mat_point_affine, pt_device.h: w not computed for an affine wave-uniform matrix
// and finite points) next to mat_point, one matrix per wave of 64 lanes, lane i on its own point.  Layout: srt_pt_math_point_affine.
__global__ void pt_point_affine_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;                               // (whole waves: lanes % 64 == 0)
  Mat4 m;
#pragma unroll
  for (int j = 0; j < 16; j++) m.c[j / 4][j % 4] = in[(i / 64) * 16 + j];
  const float* pl = in + (lanes / 64) * 16;
  const V3 v = v3(pl[i], pl[lanes + i], pl[2 * lanes + i]);
  bool skipped = false;
  const V3 a = mat_point_affine(m, mat_affine_row(m), v, &skipped);
  const V3 b = mat_point(m, v);
  out[i] = a.x; out[lanes + i] = a.y; out[2 * lanes + i] = a.z;
  out[3 * lanes + i] = b.x; out[4 * lanes + i] = b.y; out[5 * lanes + i] = b.z;
  out[6 * lanes + i] = skipped ? 1.0f : 0.0f;
}

// The top-down sweep of pt_wave.h with the min / max step behind its guard (box_hit_minmax, the minmax_*_ok predicates, pt_trace.h)
// next to the same sweep through the old step alone, one seven-node tree per wave of 64 lanes, lane i on its own ray.  The loop and
// the guard are those of pt_wave_kernel, restated (change both): the boxes once per wave, origin and reciprocals in one ballot, the
// old loop behind one scalar branch, `times` and flags through LDS slots.  Layout: srt_pt_math_topdown_minmax.
constexpr int kProbeQ = 7;
__global__ void pt_topdown_minmax_kernel(const float* __restrict__ in, size_t lanes, float* __restrict__ out) {
  __shared__ float s_slot[4][kProbeQ][2][64];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;                               // (whole waves: lanes % 64 == 0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t w = (size_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(i / 64));
  const WaveInterior* __restrict__ recs = reinterpret_cast<const WaveInterior*>(in) + w * kProbeQ;
  const float* pl = in + (lanes / 64) * kProbeQ * 16;
  float v[10];
#pragma unroll
  for (int j = 0; j < 10; j++) v[j] = pl[(size_t)j * lanes + i];
  const V3 org = v3(v[0], v[1], v[2]), inv = v3(v[3], v[4], v[5]);
  const float tx0 = v[6], ty0 = v[7], rb0 = v[8], rb1 = v[9];
#define PSLOT(q, f) s_slot[wave][q][f][lane]
  bool bok = true;
  if (lane < kProbeQ) {
    const bool l = minmax_box_ok(recs[lane].boxl), r = minmax_box_ok(recs[lane].boxr);
    bok = l & r;
  }
  const bool boxes_ok = __ballot(!bok) == 0ull;
  const bool org_ok = minmax_origin_ok(org), inv_ok = minmax_inv_ok(inv);
  const bool ok = org_ok & inv_ok;
  const bool fast = boxes_ok && __ballot(!ok) == 0ull;
  auto sweep = [&](auto minmax, float* __restrict__ o) {
    for (int q = 0; q < kProbeQ; q++) {
      const WaveInterior& W = recs[q];
      float tx = tx0, ty = ty0;
      if (q != 0) { tx = PSLOT(q, 0); ty = PSLOT(q, 1); }
      float fx, lx, ly, rx, ry;
      const uint32_t f = topdown_step<decltype(minmax)::value>(W, org, inv, tx, ty, rb0, rb1, fx, lx, ly, rx, ry);
      if (q != 0) { PSLOT(q, 0) = fx; PSLOT(q, 1) = __uint_as_float(f); }
      if (W.l_ref >= 0) { PSLOT(W.l_ref, 0) = lx; PSLOT(W.l_ref, 1) = ly; }
      if (W.r_ref >= 0) { PSLOT(W.r_ref, 0) = rx; PSLOT(W.r_ref, 1) = ry; }
      float* p = o + (size_t)(6 * q) * lanes + i;
      p[0] = __uint_as_float(f); p[lanes] = fx; p[2 * lanes] = lx; p[3 * lanes] = ly; p[4 * lanes] = rx; p[5 * lanes] = ry;
    }
  };
  if (fast) sweep(std::true_type{}, out); else sweep(std::false_type{}, out);
  sweep(std::false_type{}, out + (size_t)(6 * kProbeQ) * lanes);
  out[(size_t)(12 * kProbeQ) * lanes + i] = fast ? 1.0f : 0.0f;
#undef PSLOT
}

}  // namespace srt

using namespace srt;

namespace {

// The round trip every probe but srt_pt_math_hypot makes: `what`'s argument checks, upload the input planes of in_floats floats
// each, launch(device inputs, device outputs), download the output planes of out_floats floats each, synchronise.
template <size_t K, size_t M, class Launch>
int math_round_trip(srt_pt* pt, const char* what, const float* const (&in)[K], size_t in_floats, float* const (&out)[M], size_t out_floats, Launch&& launch) {
  int st = need_device(pt, what);
  if (st != SRT_OK) return st;
  for (const float* p : in) if (!p) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  for (const float* p : out) if (!p) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (!in_floats) return SRT_OK;
  DeviceBuffer<float> din_own[K], dout_own[M];            // (this call's own: freed on every return)
  float *din[K], *dout[M];
  for (size_t k = 0; k < K; k++) { if ((st = din_own[k].ensure(in_floats))) return st; din[k] = din_own[k]; }
  for (size_t m = 0; m < M; m++) { if ((st = dout_own[m].ensure(out_floats))) return st; dout[m] = dout_own[m]; }
  for (size_t k = 0; k < K; k++) SRT_HIP(hipMemcpyAsync(din[k], in[k], in_floats * 4, hipMemcpyHostToDevice, pt->stream));
  launch(din, dout);
  SRT_HIP(hipGetLastError());
  for (size_t m = 0; m < M; m++) SRT_HIP(hipMemcpyAsync(out[m], dout[m], out_floats * 4, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}
dim3 math_grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

extern "C" {

int srt_pt_math_cos_sin(srt_pt* pt, const float* x, size_t n, float* cos_out, float* sin_out) {
  return math_round_trip(pt, "srt_pt_math_cos_sin", {x}, n, {cos_out, sin_out}, n, [&](float* const* d, float* const* o) {
    pt_math_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], n, o[0], o[1]); });
}

int srt_pt_math_sincos2(srt_pt* pt, const float* x, size_t n, float* cos_out, float* sin_out) {
  return math_round_trip(pt, "srt_pt_math_sincos2", {x}, n, {cos_out, sin_out}, n, [&](float* const* d, float* const* o) {
    pt_sincos2_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], n, o[0], o[1]); });
}

int srt_pt_math_acos(srt_pt* pt, const float* x, size_t n, float* out) {
  return math_round_trip(pt, "srt_pt_math_acos", {x}, n, {out}, n, [&](float* const* d, float* const* o) {
    pt_acos_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], n, o[0]); });
}

int srt_pt_math_sin_unit(srt_pt* pt, const float* x, size_t n, double* out) {
  int st = need_device(pt, "srt_pt_math_sin_unit");
  if (st != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!x || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_sin_unit: NULL argument");
  DeviceBuffer<float> dx;
  DeviceBuffer<double> dout;
  if ((st = dx.ensure(n)) || (st = dout.ensure(n))) return st;
  SRT_HIP(hipMemcpyAsync(dx, x, n * sizeof(float), hipMemcpyHostToDevice, pt->stream));
  pt_sin_unit_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(dx, n, dout);
  SRT_HIP(hipGetLastError());
  SRT_HIP(hipMemcpyAsync(out, dout, n * sizeof(double), hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}

int srt_pt_dump_env_sampler(srt_pt* pt, int from_device, uint32_t dims[2], float* total, float* cdf, float* pdf, size_t cap_texels,
                            double* trig, size_t cap_trig) {
  if (!pt || !dims) return srt::fail(SRT_ERR_INVALID, "srt_pt_dump_env_sampler: NULL argument");
  int st;
  if (from_device) {
    if (pt->device < 0) return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_dump_env_sampler: a host-only context has no device tables");
    if ((st = need_device(pt, "srt_pt_dump_env_sampler")) || (st = env_image_upload(pt, "srt_pt_dump_env_sampler"))) return st;
  } else if ((st = env_image_host_tables(pt, "srt_pt_dump_env_sampler"))) {
    return st;
  }
  const size_t texels = (size_t)pt->env_w * pt->env_h, ntrig = pt->env_image.trig.size();
  dims[0] = pt->env_w; dims[1] = pt->env_h;
  if (total) *total = pt->env_image.total;                // (the host's: the device holds the normalised tables only)
  if ((cdf || pdf) && cap_texels < texels) return srt::fail(SRT_ERR_INVALID, "srt_pt_dump_env_sampler: room for %zu texels, the map has %zu", cap_texels, texels);
  if (trig && cap_trig < ntrig) return srt::fail(SRT_ERR_INVALID, "srt_pt_dump_env_sampler: room for %zu doubles, the tables have %zu", cap_trig, ntrig);
  if (from_device) {
    SRT_HIP(hipDeviceSynchronize());
    if (cdf) SRT_HIP(hipMemcpy(cdf, pt->env_image.d_tables, texels * sizeof(float), hipMemcpyDeviceToHost));
    if (pdf) SRT_HIP(hipMemcpy(pdf, pt->env_image.d_tables + texels, texels * sizeof(float), hipMemcpyDeviceToHost));
    if (trig) SRT_HIP(hipMemcpy(trig, pt->env_image.d_trig, ntrig * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    if (cdf) memcpy(cdf, pt->env_image.cdf_pdf.data(), texels * sizeof(float));
    if (pdf) memcpy(pdf, pt->env_image.cdf_pdf.data() + texels, texels * sizeof(float));
    if (trig) memcpy(trig, pt->env_image.trig.data(), ntrig * sizeof(double));
  }
  return SRT_OK;
}

int srt_pt_env_sampler_probe(srt_pt* pt, const float* u, size_t nu, uint32_t* index_out, float* dir_out, const float* dirs, size_t nd, float* pdf_out) {
  int st = need_device(pt, "srt_pt_env_sampler_probe");
  if (st != SRT_OK) return st;
  if ((nu && (!u || !index_out || !dir_out)) || (nd && (!dirs || !pdf_out))) return srt::fail(SRT_ERR_INVALID, "srt_pt_env_sampler_probe: NULL argument");
  if ((st = env_image_upload(pt, "srt_pt_env_sampler_probe"))) return st;
  if (nu + nd == 0) return SRT_OK;
  DeviceBuffer<float> du, ddir, ddirs, dpdf;
  DeviceBuffer<uint32_t> dindex;
  if ((st = du.ensure(nu + 1)) || (st = dindex.ensure(nu + 1)) || (st = ddir.ensure(3 * nu + 1)) || (st = ddirs.ensure(3 * nd + 1)) || (st = dpdf.ensure(nd + 1))) return st;
  if (nu) SRT_HIP(hipMemcpyAsync(du, u, nu * sizeof(float), hipMemcpyHostToDevice, pt->stream));
  if (nd) SRT_HIP(hipMemcpyAsync(ddirs, dirs, 3 * nd * sizeof(float), hipMemcpyHostToDevice, pt->stream));
  DScene S{};
  const size_t texels = (size_t)pt->env_w * pt->env_h;
  S.env_type = SRT_ENV_MAP; S.env_w = pt->env_w; S.env_h = pt->env_h; S.env_sampling = 1u;
  S.env_cdf = pt->env_image.d_tables; S.env_pdf = pt->env_image.d_tables + texels; S.env_trig = pt->env_image.d_trig;
  pt_env_sampler_kernel<<<math_grid(nu + nd), dim3(256), 0, pt->stream>>>(S, du, nu, dindex, ddir, ddirs, nd, dpdf);
  SRT_HIP(hipGetLastError());
  if (nu) {
    SRT_HIP(hipMemcpyAsync(index_out, dindex, nu * sizeof(uint32_t), hipMemcpyDeviceToHost, pt->stream));
    SRT_HIP(hipMemcpyAsync(dir_out, ddir, 3 * nu * sizeof(float), hipMemcpyDeviceToHost, pt->stream));
  }
  if (nd) SRT_HIP(hipMemcpyAsync(pdf_out, dpdf, nd * sizeof(float), hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}

int srt_pt_math_atan2(srt_pt* pt, const float* y, const float* x, size_t n, float* out) {
  return math_round_trip(pt, "srt_pt_math_atan2", {y, x}, n, {out}, n, [&](float* const* d, float* const* o) {
    pt_atan2_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], d[1], n, o[0]); });
}

// (srt_hypotf lives with the animation kernels: pt_anim.hip.  n == 0 returns before the NULL check, unlike the round trips above.)
int srt_pt_math_hypot(srt_pt* pt, const float* x, const float* y, size_t n, float* out) {
  int st = need_device(pt, "srt_pt_math_hypot");
  if (st != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!x || !y || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_hypot: NULL argument");
  DeviceBuffer<float> d;
  if ((st = d.ensure(3 * n))) return st;
  hipError_t e = hipMemcpy(d, x, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, y, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_anim_hypot(pt->stream, d, d + n, n, d + 2 * n);
    e = hipMemcpyAsync(out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost, pt->stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(pt->stream);
  SRT_HIP(e);
  return SRT_OK;
}

int srt_pt_math_exp(srt_pt* pt, const float* x, size_t n, float* out) {
  return math_round_trip(pt, "srt_pt_math_exp", {x}, n, {out}, n, [&](float* const* d, float* const* o) {
    pt_exp_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], n, o[0]); });
}

int srt_pt_math_pow(srt_pt* pt, const float* x, const float* y, size_t n, float* out) {
  return math_round_trip(pt, "srt_pt_math_pow", {x, y}, n, {out}, n, [&](float* const* d, float* const* o) {
    pt_pow_kernel<<<math_grid(n), dim3(256), 0, pt->stream>>>(d[0], d[1], n, o[0]); });
}

int srt_pt_math_div_sqrt(srt_pt* pt, const float* in, size_t lanes, int shared_c2, float* out) {
  return math_round_trip(pt, "srt_pt_math_div_sqrt", {in}, 5 * 3 * lanes, {out}, 4 * 3 * lanes, [&](float* const* d, float* const* o) {
    pt_div_sqrt_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, shared_c2, o[0]); });
}

int srt_pt_math_tri_verdict(srt_pt* pt, const float* in, size_t lanes, float* out) {
  return math_round_trip(pt, "srt_pt_math_tri_verdict", {in}, 27 * lanes, {out}, 19 * lanes, [&](float* const* d, float* const* o) {
    pt_tri_verdict_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

int srt_pt_math_leaf_fold(srt_pt* pt, const float* in, size_t lanes, float* out) {
  if (lanes % 64) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_leaf_fold: %zu lanes are not whole waves of 64", lanes);
  if (in)
    for (size_t w = 0; w < lanes / 64; w++) {
      uint32_t ntri;
      __builtin_memcpy(&ntri, in + w * kLeafFoldWave, 4);
      if (ntri < 1 || ntri > 12) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_leaf_fold: wave %zu has %u triangles (1..12)", w, ntri);
    }
  const size_t in_floats = (lanes / 64) * kLeafFoldWave + 18 * lanes;
  return math_round_trip(pt, "srt_pt_math_leaf_fold", {in}, in_floats, {out}, 25 * lanes, [&](float* const* d, float* const* o) {
    pt_leaf_fold_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

int srt_pt_math_sphere_batch(srt_pt* pt, const float* in, size_t lanes, float* out) {
  return math_round_trip(pt, "srt_pt_math_sphere_batch", {in}, 19 * lanes, {out}, 22 * lanes, [&](float* const* d, float* const* o) {
    pt_sphere_batch_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

int srt_pt_math_box_sweep(srt_pt* pt, const float* in, size_t lanes, float* out) {
  return math_round_trip(pt, "srt_pt_math_box_sweep", {in}, 14 * lanes, {out}, 6 * lanes, [&](float* const* d, float* const* o) {
    pt_box_sweep_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

int srt_pt_math_point_affine(srt_pt* pt, const float* in, size_t lanes, float* out) {
  if (lanes % 64) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_point_affine: %zu lanes are not whole waves of 64", lanes);
  return math_round_trip(pt, "srt_pt_math_point_affine", {in}, (lanes / 64) * 16 + 3 * lanes, {out}, 7 * lanes, [&](float* const* d, float* const* o) {
    pt_point_affine_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

int srt_pt_math_topdown_minmax(srt_pt* pt, const float* in, size_t lanes, float* out) {
  if (lanes % 64) return srt::fail(SRT_ERR_INVALID, "srt_pt_math_topdown_minmax: %zu lanes are not whole waves of 64", lanes);
  if (in)                                               // a child is a leaf (< 0) or a later node of the wave's seven: the slots it indexes
    for (size_t w = 0; w < lanes / 64; w++)
      for (int q = 0; q < kProbeQ; q++) {
        WaveInterior W;
        __builtin_memcpy(&W, in + (w * kProbeQ + (size_t)q) * 16, sizeof(W));
        for (int32_t ref : {W.l_ref, W.r_ref})
          if (ref >= 0 && (ref <= q || ref >= kProbeQ))
            return srt::fail(SRT_ERR_INVALID, "srt_pt_math_topdown_minmax: wave %zu, node %d has child %d (a leaf, or %d..%d)", w, q, ref, q + 1, kProbeQ - 1);
      }
  const size_t in_floats = (lanes / 64) * kProbeQ * 16 + 10 * lanes;
  return math_round_trip(pt, "srt_pt_math_topdown_minmax", {in}, in_floats, {out}, (12 * kProbeQ + 1) * lanes, [&](float* const* d, float* const* o) {
    pt_topdown_minmax_kernel<<<math_grid(lanes), dim3(256), 0, pt->stream>>>(d[0], lanes, o[0]); });
}

}  // extern "C"
