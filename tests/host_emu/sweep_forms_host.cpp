// TEST-ONLY: the bottom-up sweep's fold and combine on the two-word hit (packed_fold, packed_combine, pt_trace.h) compiled for
// the host next to the four-field form they replace (Hit {hit, dist, obj, tri}: fold, left_wins, the visit rule of
// student/bvh.inl:216 and Trace::min written out).  Built by tests/test_pt_sweep_forms_host.py with g++ -ffp-contract=off.
#include "pt_trace.h"

using namespace srt;

namespace {
constexpr uint32_t kShift = 27u;
Hit none() { Hit h; h.hit = false; h.dist = 0.0f; h.obj = 0; h.tri = 0; return h; }
Hit unpack(PHit p) {
  Hit h = none();
  if (p.id != kRetMiss) { h.hit = true; h.dist = p.dist; h.obj = p.id >> kShift; h.tri = p.id & ((1u << kShift) - 1u); }
  return h;
}
PHit pack(const Hit& h) { PHit p; p.dist = h.dist; p.id = h.hit ? ((h.obj << kShift) | h.tri) : kRetMiss; return p; }
}  // namespace

// One node per case.  in: {l.dist bits, l.id, r.dist bits, r.id, flags (1 either box hit, 2 left child nearer, 4 hitboth), farx bits};
// out: {packed dist bits, packed id, four-field dist bits, four-field id (packed for comparison), four-field hit}.
extern "C" int sweep_combine_host(const uint32_t* in, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    const uint32_t* c = in + 6 * i;
    PHit l, r;
    l.dist = __uint_as_float(c[0]); l.id = c[1]; r.dist = __uint_as_float(c[2]); r.id = c[3];
    const bool hit_any = (c[4] & 1u) != 0, cl = (c[4] & 2u) != 0, hitboth = (c[4] & 4u) != 0;
    const float farx = __uint_as_float(c[5]);
    const PHit p = packed_combine(l, r, hit_any, cl, hitboth, farx);
    // the four-field form
    const Hit L = unpack(l), R = unpack(r);
    const Hit rc = cl ? L : R;
    const Hit rs = cl ? R : L;
    Hit ret = none();
    if (hit_any) {
      ret = rc;
      if (farx < rc.dist || (!rc.hit && hitboth)) {
        if (!left_wins(rc.hit, rc.dist, rs.hit, rs.dist)) ret = rs.hit ? rs : none();
      }
    }
    const PHit q = pack(ret);
    uint32_t* o = out + 5 * i;
    o[0] = __float_as_uint(p.dist); o[1] = p.id; o[2] = __float_as_uint(q.dist); o[3] = q.id; o[4] = ret.hit ? 1u : 0u;
  }
  return 0;
}

// A leaf of `m` candidates per case, folded in order.  in per candidate: {hit, dist bits, obj, tri}; out as above.
extern "C" int sweep_fold_host(const uint32_t* in, size_t n, size_t m, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    PHit p = packed_miss();
    Hit h = none();
    for (size_t j = 0; j < m; j++) {
      const uint32_t* c = in + 4 * (i * m + j);
      const bool hit = c[0] != 0;
      const float dist = __uint_as_float(c[1]);
      packed_fold(p, hit, dist, (c[2] << kShift) | c[3]);
      fold(h, hit, dist, c[2], c[3]);
    }
    const PHit q = pack(h);
    uint32_t* o = out + 5 * i;
    o[0] = __float_as_uint(p.dist); o[1] = p.id; o[2] = __float_as_uint(q.dist); o[3] = q.id; o[4] = h.hit ? 1u : 0u;
  }
  return 0;
}
