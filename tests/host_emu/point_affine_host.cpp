// TEST-ONLY: the leaf section's point transform (mat_point_affine / mat_affine_row, pt_device.h) compiled for the host next to the
// plain projective product (mat_point), one lane at a time.  Built by tests/test_pt_point_affine_host.py with g++ -ffp-contract=off.
#include "pt_device.h"

using namespace srt;

// in: per set 16 floats (Mat4::data, column-major) and the point (3); out: 8 words per set {x, y, z bits of mat_point_affine, x, y, z
// bits of mat_point, 1 where w was not computed, 1 where the bottom row counts as affine}.
extern "C" int point_affine_host(const float* in, size_t n, uint32_t* out) {
  for (size_t i = 0; i < n; i++) {
    const float* c = in + 19 * i;
    Mat4 m;
    for (int j = 0; j < 16; j++) m.c[j / 4][j % 4] = c[j];
    const V3 v = v3(c[16], c[17], c[18]);
    bool skipped = false;
    const bool affine = mat_affine_row(m);
    const V3 a = mat_point_affine(m, affine, v, &skipped);
    const V3 b = mat_point(m, v);
    uint32_t* o = out + 8 * i;
    o[0] = __float_as_uint(a.x); o[1] = __float_as_uint(a.y); o[2] = __float_as_uint(a.z);
    o[3] = __float_as_uint(b.x); o[4] = __float_as_uint(b.y); o[5] = __float_as_uint(b.z);
    o[6] = skipped ? 1u : 0u; o[7] = affine ? 1u : 0u;
  }
  return 0;
}
