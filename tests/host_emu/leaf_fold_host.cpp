// TEST-ONLY: the candidate bookkeeping of the wave kernel's leaf fold (leaf_cand_add, pt_device.h) compiled for the host, next to
// the plain ordered fold over tri_hit.  Built by tests/test_pt_leaf_fold_host.py with g++ -ffp-contract=off.
#include "pt_device.h"

using namespace srt;

// Waves of 64 lanes, one leaf per wave.  tris: 12 x 9 floats per wave (p0, e1, e2); ntri per wave (1..12); org 3 floats per lane;
// dirs 9 (three rays); bounds 6 ({b0, b1} per ray).
// bad: per lane, 1 where the device flags the lane (a pair of its three rays out of the window or ambiguous, or a second candidate).
// out: per (lane, ray) 9 words - number of candidates (triangles that are not outside by tri_verdict), then {hit, triangle, bits of t,
// bits of dist} of the plain tri_hit on the LAST candidate (zeros without one or when it misses: the default Trace), then the same
// four of the ordered fold ret = Trace::min(ret, tri_hit) over the whole leaf.
extern "C" int leaf_fold_host(const float* tris, const uint32_t* ntri, const float* org, const float* dirs, const float* bounds, size_t waves,
                              uint32_t* bad, uint32_t* out) {
  for (size_t w = 0; w < waves; w++) {
    if (ntri[w] < 1 || ntri[w] > 12) return 1;
    Tri g[12];
    for (uint32_t t = 0; t < ntri[w]; t++)
      for (int j = 0; j < 3; j++) {
        g[t].p0[j] = tris[(w * 12 + t) * 9 + j]; g[t].e1[j] = tris[(w * 12 + t) * 9 + 3 + j]; g[t].e2[j] = tris[(w * 12 + t) * 9 + 6 + j];
      }
    for (size_t l = 0; l < 64; l++) {
      const size_t i = w * 64 + l;
      const V3 o = v3p(org + 3 * i);
      LeafCand c[3];
      uint32_t count[3] = {0, 0, 0};
      for (int r = 0; r < 3; r++) c[r] = leaf_cand_none();
      bool lane_bad = false;
      for (uint32_t t = 0; t < ntri[w]; t++) {
        // the numerators exactly as tri_hit / tri_hitN / leaf_foldN form them
        const V3 e1 = v3p(g[t].e1), e2 = v3p(g[t].e2);
        const V3 s = o - v3p(g[t].p0);
        const V3 sxe2 = cross(s, e2);
        const float nt = -1.0f * dot(sxe2, e1);
        float num[3][3], det[3];
        for (int r = 0; r < 3; r++) {
          const V3 d = v3p(dirs + 9 * i + 3 * r);
          const V3 e1xd = cross(e1, d);
          det[r] = dot(e1xd, e2);
          num[r][0] = -1.0f * dot(sxe2, d);
          num[r][1] = dot(e1xd, s);
          num[r][2] = nt;
        }
        lane_bad = lane_bad | !div_in_range<3, true>(num, det);
        for (int r = 0; r < 3; r++) {
          count[r] += !tri_verdict(num[r][0], num[r][1], det[r]).outside;
          lane_bad = lane_bad | leaf_cand_add(c[r], num[r][0], num[r][1], det[r], nt, t + 1u);
        }
      }
      bad[i] = lane_bad;
      for (int r = 0; r < 3; r++) {
        Ray ray;
        ray.o = o; ray.d = v3p(dirs + 9 * i + 3 * r);
        ray.b0 = bounds[6 * i + 2 * r]; ray.b1 = bounds[6 * i + 2 * r + 1];
        uint32_t* q = out + 9 * (3 * i + r);
        q[0] = count[r];
        q[1] = q[2] = q[3] = q[4] = 0;
        if (c[r].n != 0u) {
          const TriHit h = tri_hit(g[c[r].n - 1u], ray);
          if (h.hit) { q[1] = 1; q[2] = c[r].n - 1u; q[3] = __float_as_uint(h.t); q[4] = __float_as_uint(h.dist); }
        }
        bool fh = false;                                  // Trace::min as the reference writes it
        float fd = 0.0f, ft = 0.0f;
        uint32_t fn = 0;
        for (uint32_t t = 0; t < ntri[w]; t++) {
          const TriHit h = tri_hit(g[t], ray);
          const bool left = fh && (!h.hit || fd < h.dist);
          if (!left && h.hit) { fh = true; fd = h.dist; ft = h.t; fn = t; }
        }
        q[5] = fh; q[6] = fn; q[7] = __float_as_uint(ft); q[8] = __float_as_uint(fd);
      }
    }
  }
  return 0;
}
