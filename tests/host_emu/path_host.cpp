// TEST-ONLY: path_sample() of csrc/pt_trace.h - Pathtracer::trace_pixel as the lane-per-sample kernels run it, shading included -
// compiled for the host and run one lane at a time, on top of flat_host.cpp's scene feeder.  tests/test_pt_shade_edges_host.py
// compares it with the oracle on the CPU; the HIP build of the same source is what the GPU tests check.  With -DPATH_HOST_MAIN the
// same file is a stand-alone program (built with -fsanitize=address,undefined and run as its own process) that reads scenes, a
// sample list and the expected values from a flat file and evaluates every scene in it.
#include "flat_host.cpp"

#include <cstdio>
#include <cstring>
#include <string>

extern "C" {

// rgb: 3 floats per sample; draws = rng.draws, rays = cnt.v[C_RAYS] per sample.  max_depth <= kMaxPathDepth.
int emu_path_samples(void* h, const float* iview, float vfov, float ar, uint32_t w, uint32_t hh, uint32_t max_depth, uint64_t seed,
                     const uint32_t* xs, const uint32_t* ys, const uint32_t* ss, size_t n, float* rgb, uint32_t* draws, uint32_t* rays) {
  Emu* e = (Emu*)h;
  if (max_depth > (uint32_t)kMaxPathDepth || !w || !hh) return -1;
  DScene S = e->S;
  S.cam = make_camera(iview, vfov, ar);
  S.w = w; S.h = hh; S.max_depth = max_depth;
  S.delta_lights = e->delta_lights.data(); S.ndelta = (uint32_t)e->delta_lights.size();
  S.env_type = e->env_type;
  for (int i = 0; i < 3; i++) S.env_radiance[i] = e->env_radiance[i];
  S.env_map = e->env_map.empty() ? nullptr : e->env_map.data(); S.env_w = e->env_w; S.env_h = e->env_h;
  S.ray_log = nullptr; S.ray_log_cap = 0; S.elide = 0;
  for (size_t i = 0; i < n; i++) {
    if (xs[i] >= w || ys[i] >= hh) return -1;
    Counters cnt;
    for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
    Rng rng;
    rng.key(seed, ys[i] * w + xs[i], ss[i]);
    const Spec p = path_sample<true>(S, xs[i], ys[i], rng, cnt);
    rgb[3 * i] = p.r; rgb[3 * i + 1] = p.g; rgb[3 * i + 2] = p.b;
    draws[i] = rng.draws; rays[i] = cnt.v[C_RAYS];
  }
  return 0;
}

}  // extern "C"

#ifdef PATH_HOST_MAIN
namespace {

// The file as 32-bit words; every read is checked against its end.
struct Words {
  std::vector<uint32_t> w;
  size_t at = 0;
  bool ok = true;
  const uint32_t* take(size_t n) {
    if (!ok || n > w.size() - at) { ok = false; return nullptr; }
    const uint32_t* p = w.data() + at;
    at += n;
    return p;
  }
  uint32_t u32() { const uint32_t* p = take(1); return p ? *p : 0u; }
  float f32() { const uint32_t v = u32(); float f; std::memcpy(&f, &v, 4); return f; }
  const float* floats(size_t n) { return (const float*)take(n); }
};

bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }

enum : uint32_t { OP_END = 0, OP_MATERIAL, OP_MESH, OP_SPHERE, OP_SPHERE_LIGHT, OP_LIGHT, OP_ENV, OP_ENV_MAP, OP_COMMIT, OP_CAMERA };

}  // namespace

// File (32-bit words): {magic, cases, w, h, max_depth, n, seed low, seed high}; xs[n], ys[n], ss[n]; per case a name {bytes, the
// characters padded to words}, the feeder's calls in order, each as {op, arguments} (tests/test_pt_shade_edges_host.py writes
// them), OP_END, and the expected rgb[3 n], draws[n], rays[n].
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  Words in;
  uint32_t buf[4096];
  size_t got;
  while ((got = fread(buf, 4, 4096, f)) > 0) in.w.insert(in.w.end(), buf, buf + got);
  fclose(f);
  const uint32_t magic = in.u32(), ncases = in.u32(), w = in.u32(), h = in.u32(), depth = in.u32(), n = in.u32();
  const uint64_t seed = (uint64_t)in.u32() | ((uint64_t)in.u32() << 32);
  if (!in.ok || magic != 0x54534850u || n > (1u << 20)) return 2;
  const uint32_t *xs = in.take(n), *ys = in.take(n), *ss = in.take(n);
  if (!in.ok) return 2;
  std::vector<float> rgb(3 * (size_t)n);
  std::vector<uint32_t> draws(n), rays(n);
  size_t bad_cases = 0;
  for (uint32_t c = 0; c < ncases; c++) {
    const uint32_t name_bytes = in.u32();
    if (!in.ok || name_bytes > 256) return 2;
    const uint32_t* nw = in.take((name_bytes + 3) / 4);
    if (!in.ok) return 2;
    const std::string name((const char*)nw, name_bytes);
    void* e = emu_create();
    float iview[16] = {0}, vfov = 0, ar = 0;
    bool committed = false, camera = false;
    for (;;) {
      const uint32_t op = in.u32();
      if (!in.ok) return 2;
      if (op == OP_END) break;
      if (op == OP_MATERIAL) {
        const uint32_t type = in.u32();
        const float *a = in.floats(3), *b = in.floats(3);
        const float ior = in.f32();
        if (in.ok) emu_add_material(e, type, a, b, ior);
      } else if (op == OP_MESH || op == OP_SPHERE_LIGHT) {
        const float radius = in.f32();
        const uint32_t material = in.u32(), is_light = in.u32();
        const float* T = in.floats(16);
        const uint32_t nv = in.u32(), ni = in.u32();
        if (!in.ok || nv > (1u << 24) || ni > (1u << 24) || ni % 3) return 2;
        const float *pos = in.floats(3 * (size_t)nv), *nrm = in.floats(3 * (size_t)nv);
        const uint32_t* idx = in.take(ni);
        if (!in.ok) return 2;
        for (uint32_t i = 0; i < ni; i++)
          if (idx[i] >= nv) return 2;
        if (op == OP_MESH) emu_add_mesh(e, pos, nrm, nv, idx, ni, T, material, (int)is_light);
        else emu_feed_sphere_light(e, radius, T, material, pos, nrm, nv, idx, ni);
      } else if (op == OP_SPHERE) {
        const float radius = in.f32();
        const uint32_t material = in.u32();
        const float* T = in.floats(16);
        if (in.ok) emu_add_sphere(e, radius, T, material);
      } else if (op == OP_LIGHT) {
        const uint32_t type = in.u32();
        const float *radiance = in.floats(3), *bounds = in.floats(2), *T = in.floats(16);
        if (in.ok) emu_feed_light(e, type, radiance, bounds, T);
      } else if (op == OP_ENV) {
        const uint32_t type = in.u32();
        const float* radiance = in.floats(3);
        if (in.ok) emu_feed_env_light(e, type, radiance);
      } else if (op == OP_ENV_MAP) {
        const uint32_t ew = in.u32(), eh = in.u32();
        if (!in.ok || !ew || !eh || (uint64_t)ew * eh > (1u << 24)) return 2;
        const float* px = in.floats(3 * (size_t)ew * eh);
        if (in.ok) emu_feed_env_map(e, ew, eh, px);
      } else if (op == OP_COMMIT) {
        const uint32_t use_bvh = in.u32();
        if (!in.ok) return 2;
        const Emu* E = (const Emu*)e;
        for (const ObjectInput& o : E->inputs)
          if (o.material >= E->materials.size()) return 2;
        if (emu_commit(e, (int)use_bvh) != 0) { printf("%s: the scene is refused\n", name.c_str()); return 1; }
        committed = true;
      } else if (op == OP_CAMERA) {
        const float* m = in.floats(16);
        vfov = in.f32(); ar = in.f32();
        if (in.ok) { std::memcpy(iview, m, sizeof iview); camera = true; }
      } else {
        return 2;
      }
      if (!in.ok) return 2;
    }
    const float* want_rgb = in.floats(3 * (size_t)n);
    const uint32_t *want_draws = in.take(n), *want_rays = in.take(n);
    if (!in.ok || !committed || !camera) return 2;
    if (emu_path_samples(e, iview, vfov, ar, w, h, depth, seed, xs, ys, ss, n, rgb.data(), draws.data(), rays.data()) != 0) return 2;
    size_t bad = 0;
    for (uint32_t i = 0; i < n; i++)
      bad += !(same(rgb[3 * i], want_rgb[3 * i]) && same(rgb[3 * i + 1], want_rgb[3 * i + 1]) && same(rgb[3 * i + 2], want_rgb[3 * i + 2]) &&
               draws[i] == want_draws[i] && rays[i] == want_rays[i]);
    if (bad) { printf("%s: %zu of %u samples differ from the expected ones\n", name.c_str(), bad, n); bad_cases++; }
    emu_destroy(e);
  }
  if (in.at != in.w.size()) return 2;
  if (bad_cases) return 1;
  printf("path_sanitized: ok (%u scenes, %u samples each)\n", ncases, n);
  return 0;
}
#endif
