// TEST-ONLY: Triangle::hit's inside / outside verdict from the numerators (tri_verdict, pt_device.h) compiled for the host,
// next to the reference's comparisons on the correctly rounded quotients and to the plain tri_hit.  Built by
// tests/test_pt_tri_verdict_host.py with g++ -ffp-contract=off.
#include "pt_device.h"

using namespace srt;

// per (lane, ray): out[0] in the window (div_in_range of this ray alone), out[1] verdict.outside, out[2] verdict.ambiguous,
// out[3] the reference's u < 0 || v < 0 || (1 - u - v) < 0, out[4] hit, out[5] bits of t, out[6] bits of dist (tri_hit).
// tri: 9 floats per lane (p0, e1, e2); org 3; dirs 9 (three rays); bounds 6 ({b0, b1} per ray).
extern "C" int tri_verdict_host(const float* tri, const float* org, const float* dirs, const float* bounds, size_t lanes, uint32_t* out) {
  for (size_t i = 0; i < lanes; i++) {
    Tri g;
    for (int j = 0; j < 3; j++) { g.p0[j] = tri[9 * i + j]; g.e1[j] = tri[9 * i + 3 + j]; g.e2[j] = tri[9 * i + 6 + j]; }
    for (int r = 0; r < 3; r++) {
      Ray ray;
      ray.o = v3p(org + 3 * i); ray.d = v3p(dirs + 9 * i + 3 * r);
      ray.b0 = bounds[6 * i + 2 * r]; ray.b1 = bounds[6 * i + 2 * r + 1];
      // the numerators exactly as tri_hit / tri_hitN form them
      const V3 e1 = v3p(g.e1), e2 = v3p(g.e2);
      const V3 s = ray.o - v3p(g.p0);
      const V3 e1xd = cross(e1, ray.d);
      const float det = dot(e1xd, e2);
      const V3 sxe2 = cross(s, e2);
      float num[1][3] = {{-1.0f * dot(sxe2, ray.d), dot(e1xd, s), -1.0f * dot(sxe2, e1)}};
      const TriVerdict v = tri_verdict(num[0][0], num[0][1], det);
      const float u = num[0][0] / det, w = num[0][1] / det;
      const TriHit h = tri_hit(g, ray);
      uint32_t* o = out + 7 * (3 * i + r);
      o[0] = div_in_range<1, true>(num, &det);
      o[1] = v.outside; o[2] = v.ambiguous;
      o[3] = (u < 0) || (w < 0) || ((1.0f - u - w) < 0);
      o[4] = h.hit; o[5] = __float_as_uint(h.t); o[6] = __float_as_uint(h.dist);
    }
  }
  return 0;
}

// Ray::transform's divide (object_testN, pt_wave.h: the rotated direction over its norm, divNx3<NR, false>): out[i] = the window
// verdict div_in_range of lane i alone.  num: 3 floats per lane, den: 1.
extern "C" int div_window_host(const float* num, const float* den, size_t lanes, uint32_t* out) {
  for (size_t i = 0; i < lanes; i++) {
    const float n[1][3] = {{num[3 * i], num[3 * i + 1], num[3 * i + 2]}};
    out[i] = div_in_range<1, false>(n, den + i);
  }
  return 0;
}
