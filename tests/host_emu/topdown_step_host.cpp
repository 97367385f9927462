// TEST-ONLY: one (node, ray) step of the top-down sweep (topdown_step, pt_trace.h: one select per field of the children's `times`)
// compiled for the host next to the long form it replaces - closer / second chosen as student/bvh.inl:186-209 chooses them, then
// handed to the children.  Built by tests/test_pt_topdown_step_host.py with g++ -ffp-contract=off.
#include "pt_trace.h"

using namespace srt;

// in: 22 floats per case (left box min xyz max xyz, right box min xyz max xyz, origin xyz, reciprocal direction xyz, times x, y,
// dist_bounds x, y); out: 12 words per case {flags, cur_far_t.x, left times x, y, right times x, y} of topdown_step, then the same
// six of the long form.
extern "C" int topdown_step_host(const float* in, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    const float* c = in + 22 * i;
    WaveInterior W;
    for (int j = 0; j < 6; j++) { W.boxl[j] = c[j]; W.boxr[j] = c[6 + j]; }
    W.l_ref = 1; W.r_ref = 2; W.l_cnt = W.r_cnt = 0u;
    const V3 org = v3(c[12], c[13], c[14]), inv = v3(c[15], c[16], c[17]);
    const float tx = c[18], ty = c[19], rb0 = c[20], rb1 = c[21];
    float fx, lx, ly, rx, ry;
    const uint32_t f = topdown_step(W, org, inv, tx, ty, rb0, rb1, fx, lx, ly, rx, ry);
    uint32_t* o = out + 12 * i;
    o[0] = f; o[1] = __float_as_uint(fx); o[2] = __float_as_uint(lx); o[3] = __float_as_uint(ly); o[4] = __float_as_uint(rx); o[5] = __float_as_uint(ry);
    // the long form
    float t1x = tx, t1y = ty, t2x = tx, t2y = ty;
    const bool hl = box_hit_inv(W.boxl, org, inv, t1x, t1y);
    const bool hr = box_hit_inv(W.boxr, org, inv, t2x, t2y);
    bool hitboth = false, left_first;
    float cx, cy, sx = rb0, sy = rb1;                   // `second` gets ray.dist_bounds unless both were hit
    if (hl && hr) {
      hitboth = true;
      if (t1x < t2x) { left_first = true; cx = t1x; cy = t1y; sx = t2x; sy = t2y; }
      else { left_first = false; cx = t2x; cy = t2y; sx = t1x; sy = t1y; }
    } else if (hl) { left_first = true; cx = t1x; cy = t1y; }
    else { left_first = false; cx = t2x; cy = t2y; }
    o[6] = (hl ? 1u : 0u) | (hr ? 2u : 0u) | (left_first ? 4u : 0u) | (hitboth ? 8u : 0u);
    o[7] = __float_as_uint(sx);
    o[8] = __float_as_uint(left_first ? cx : sx); o[9] = __float_as_uint(left_first ? cy : sy);
    o[10] = __float_as_uint(left_first ? sx : cx); o[11] = __float_as_uint(left_first ? sy : cy);
  }
  return 0;
}
