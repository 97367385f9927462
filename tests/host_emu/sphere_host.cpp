// TEST-ONLY: Sphere::hit of the device headers (sphere_hit and the batch form sphere_hitN<3>, pt_device.h) compiled for the host and
// run one set at a time: a "wave" is one lane here (hip/hip_runtime.h), so the batch form computes the tangent root exactly when one
// of the set's own three rays has delta == 0.  Built by tests/test_pt_sphere_host.py with g++ -ffp-contract=off; the stand-alone
// main below it (-DSPHERE_HOST_MAIN) is for a sanitizer build.
#include "pt_device.h"

using namespace srt;

// radius: 1 float per set; org 3; dirs 9 (three rays); bounds 6 ({b0, b1} per ray).  Per (set, ray), nine words: out[0] hit,
// out[1] bits of t, out[2] bits of delta (sphere_hit / sphere_two_roots); out[3] hit, out[4] bits of t (sphere_hitN<3>); out[5] bits of
// the distance |Ray::at(t) - origin| as object_hit forms it, out[6..8] bits of the position Ray::at(t) as surface_of forms it.
extern "C" int sphere_host(const float* radius, const float* org, const float* dirs, const float* bounds, size_t sets, uint32_t* out) {
  for (size_t i = 0; i < sets; i++) {
    const V3 o = v3p(org + 3 * i);
    V3 d[3];
    float b0[3], b1[3];
    for (int r = 0; r < 3; r++) { d[r] = v3p(dirs + 9 * i + 3 * r); b0[r] = bounds[6 * i + 2 * r]; b1[r] = bounds[6 * i + 2 * r + 1]; }
    SphHit hn[3];
    sphere_hitN<3>(radius[i], o, d, b0, b1, hn);
    for (int r = 0; r < 3; r++) {
      Ray ray;
      ray.o = o; ray.d = d[r]; ray.b0 = b0[r]; ray.b1 = b1[r];
      const SphHit h = sphere_hit(radius[i], ray);
      bool hit_two;
      float t_two;
      const float delta = sphere_two_roots(radius[i], ray, hit_two, t_two);
      const V3 pos = ray_at(ray, h.t);
      uint32_t* w = out + 9 * (3 * i + r);
      w[0] = h.hit; w[1] = __float_as_uint(h.t); w[2] = __float_as_uint(delta);
      w[3] = hn[r].hit; w[4] = __float_as_uint(hn[r].t);
      w[5] = __float_as_uint(fabsf(norm(pos - ray.o)));
      w[6] = __float_as_uint(pos.x); w[7] = __float_as_uint(pos.y); w[8] = __float_as_uint(pos.z);
    }
  }
  return 0;
}

#ifdef SPHERE_HOST_MAIN
#include <cstdio>
#include <vector>
// sets from a file of floats (19 per set: radius, origin, three directions, three {b0, b1}); prints a checksum of the results.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<float> v;
  float buf[19];
  while (std::fread(buf, sizeof(float), 19, f) == 19) v.insert(v.end(), buf, buf + 19);
  std::fclose(f);
  const size_t n = v.size() / 19;
  std::vector<float> radius(n), org(3 * n), dirs(9 * n), bounds(6 * n);
  for (size_t i = 0; i < n; i++) {
    const float* s = v.data() + 19 * i;
    radius[i] = s[0];
    for (int j = 0; j < 3; j++) org[3 * i + j] = s[1 + j];
    for (int j = 0; j < 9; j++) dirs[9 * i + j] = s[4 + j];
    for (int j = 0; j < 6; j++) bounds[6 * i + j] = s[13 + j];
  }
  std::vector<uint32_t> out(27 * n);
  sphere_host(radius.data(), org.data(), dirs.data(), bounds.data(), n, out.data());
  uint64_t sum = 0;
  for (uint32_t w : out) sum = sum * 1099511628211ull + w;
  std::printf("%zu sets, checksum %016llx\n", n, (unsigned long long)sum);
  return 0;
}
#endif
