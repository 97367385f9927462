// TEST-ONLY: Env_Map's importance sampler as the kernels run it - the host-built tables of csrc/pt_env_image.h, env_image_upper_bound /
// env_image_direction / env_image_pdf and path_sample's image-sampler build of csrc/pt_trace.h, and srt_sin_unit of csrc/pt_sin_unit.h -
// compiled for the host on top of path_host.cpp's scene feeder.  tests/test_pt_env_image_host.py compares them with the fixtures
// recorded from the reference; the HIP build of the same source is what the GPU tests check.  With -DENV_IMAGE_HOST_MAIN the same file
// is a stand-alone program (built with -fsanitize=address,undefined, run as its own process) that evaluates every component case of
// a flat file.
#include "path_host.cpp"

#include <cmath>

#include "pt_env_image.h"

namespace {
struct Sampler {
  EnvImageTables T;
  DScene S;
  Sampler(uint32_t w, uint32_t h, const float* rgb) {
    build_env_image_tables(rgb, w, h, &T);
    S = DScene();
    S.env_type = 3u; S.env_w = w; S.env_h = h; S.env_sampling = 1u;
    S.env_cdf = T.cdf_pdf.data(); S.env_pdf = T.cdf_pdf.data() + (size_t)w * h; S.env_trig = T.trig.data();
  }
};
}  // namespace

extern "C" {

// cdf, pdf: w * h floats; trig: 2 (h + 1) + 2 w doubles
int emu_env_image_tables(uint32_t w, uint32_t h, const float* rgb, float* cdf, float* pdf, float* total, double* trig) {
  const Sampler s(w, h, rgb);
  const size_t n = (size_t)w * h;
  std::memcpy(cdf, s.T.cdf_pdf.data(), n * 4);
  std::memcpy(pdf, s.T.cdf_pdf.data() + n, n * 4);
  std::memcpy(trig, s.T.trig.data(), s.T.trig.size() * 8);
  *total = s.T.total;
  return 0;
}

int emu_env_image_probe(uint32_t w, uint32_t h, const float* rgb, const float* u, size_t nu, uint32_t* index, float* dir_out,
                        const float* dirs, size_t nd, float* pdf_out) {
  const Sampler s(w, h, rgb);
  for (size_t i = 0; i < nu; i++) {
    index[i] = env_image_upper_bound(s.S, u[i]);
    const V3 d = env_image_direction(s.S, index[i]);
    dir_out[3 * i] = d.x; dir_out[3 * i + 1] = d.y; dir_out[3 * i + 2] = d.z;
  }
  for (size_t j = 0; j < nd; j++) pdf_out[j] = env_image_pdf(s.S, v3(dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]));
  return 0;
}

// emu_path_samples (path_host.cpp) with the image sampler on: the scene must have an environment map
int emu_env_image_path_samples(void* h, const float* iview, float vfov, float ar, uint32_t w, uint32_t hh, uint32_t max_depth, uint64_t seed,
                               const uint32_t* xs, const uint32_t* ys, const uint32_t* ss, size_t n, float* rgb, uint32_t* draws, uint32_t* rays) {
  Emu* e = (Emu*)h;
  if (max_depth > (uint32_t)kMaxPathDepth || !w || !hh || e->env_type != 3u || e->env_map.empty()) return -1;
  const Sampler s(e->env_w, e->env_h, e->env_map.data());
  DScene S = e->S;
  S.cam = make_camera(iview, vfov, ar);
  S.w = w; S.h = hh; S.max_depth = max_depth;
  S.delta_lights = e->delta_lights.data(); S.ndelta = (uint32_t)e->delta_lights.size();
  S.env_type = e->env_type;
  for (int i = 0; i < 3; i++) S.env_radiance[i] = e->env_radiance[i];
  S.env_map = e->env_map.data(); S.env_w = e->env_w; S.env_h = e->env_h;
  S.ray_log = nullptr; S.ray_log_cap = 0; S.elide = 0;
  S.env_cdf = s.S.env_cdf; S.env_pdf = s.S.env_pdf; S.env_trig = s.S.env_trig; S.env_sampling = 1u;
  for (size_t i = 0; i < n; i++) {
    if (xs[i] >= w || ys[i] >= hh) return -1;
    Counters cnt;
    for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
    Rng rng;
    rng.key(seed, ys[i] * w + xs[i], ss[i]);
    const Spec p = path_sample<true, true>(S, xs[i], ys[i], rng, cnt);
    rgb[3 * i] = p.r; rgb[3 * i + 1] = p.g; rgb[3 * i + 2] = p.b;
    draws[i] = rng.draws; rays[i] = cnt.v[C_RAYS];
  }
  return 0;
}

// the restated double sin next to the C library's, for floats x (the caller keeps them in [0, 1])
int emu_sin_unit(const float* x, size_t n, double* restated, double* libm) {
  for (size_t i = 0; i < n; i++) { restated[i] = srt_sin_unit(x[i]); libm[i] = std::sin((double)x[i]); }
  return 0;
}
// every float of [first, last] (bit patterns, both non-negative): how many differ from the C library's, and the first that does
uint64_t emu_sin_unit_sweep(uint32_t first, uint32_t last, uint32_t* first_bad) {
  uint64_t bad = 0;
  for (uint64_t b = first; b <= last; b++) {
    float x;
    const uint32_t bb = (uint32_t)b;
    std::memcpy(&x, &bb, 4);
    const double a = srt_sin_unit(x), r = std::sin((double)x);
    if (std::memcmp(&a, &r, 8) != 0) { if (!bad && first_bad) *first_bad = bb; bad++; }
  }
  return bad;
}

}  // extern "C"

#ifdef ENV_IMAGE_HOST_MAIN
// File (32-bit words): {magic, cases}; per case {w, h, nu, nd}, rgb[3 w h], u[nu], dirs[3 nd], then the expected cdf[w h], pdf[w h],
// total, index[nu], sample[3 nu], pdf_of[nd].  Every read is checked against the file's end (Words, path_host.cpp's... own copy here).
namespace {
struct In {
  std::vector<uint32_t> w;
  size_t at = 0;
  bool ok = true;
  const uint32_t* take(size_t n) {
    if (!ok || n > w.size() - at) { ok = false; return nullptr; }
    const uint32_t* p = w.data() + at;
    at += n;
    return p;
  }
};
bool same_f(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  In in;
  uint32_t buf[4096];
  size_t got;
  while ((got = fread(buf, 4, 4096, f)) > 0) in.w.insert(in.w.end(), buf, buf + got);
  fclose(f);
  const uint32_t* head = in.take(2);
  if (!head || head[0] != 0x47494e45u) return 2;
  const uint32_t ncases = head[1];
  size_t bad_cases = 0, draws = 0, dirs_n = 0;
  for (uint32_t c = 0; c < ncases; c++) {
    const uint32_t* d = in.take(4);
    if (!d) return 2;
    const uint32_t w = d[0], h = d[1], nu = d[2], nd = d[3];
    if (!w || !h || (uint64_t)w * h > (1u << 20) || nu > (1u << 20) || nd > (1u << 20)) return 2;
    const size_t n = (size_t)w * h;
    const float* rgb = (const float*)in.take(3 * n);
    const float* u = (const float*)in.take(nu);
    const float* dirs = (const float*)in.take(3 * (size_t)nd);
    const float* want_cdf = (const float*)in.take(n);
    const float* want_pdf = (const float*)in.take(n);
    const float* want_total = (const float*)in.take(1);
    const uint32_t* want_index = in.take(nu);
    const float* want_sample = (const float*)in.take(3 * (size_t)nu);
    const float* want_pdf_of = (const float*)in.take(nd);
    if (!in.ok) return 2;
    std::vector<float> cdf(n), pdf(n), dir_out(3 * (size_t)nu + 1), pdf_out(nd + 1);
    std::vector<double> trig(2 * ((size_t)h + 1) + 2 * (size_t)w);
    std::vector<uint32_t> index(nu + 1);
    float total = 0;
    emu_env_image_tables(w, h, rgb, cdf.data(), pdf.data(), &total, trig.data());
    emu_env_image_probe(w, h, rgb, u, nu, index.data(), dir_out.data(), dirs, nd, pdf_out.data());
    size_t bad = !same_f(total, *want_total);
    for (size_t i = 0; i < n; i++) bad += !same_f(cdf[i], want_cdf[i]) + !same_f(pdf[i], want_pdf[i]);
    for (size_t i = 0; i < nu; i++) {
      bad += index[i] != want_index[i];
      for (int k = 0; k < 3; k++) bad += !same_f(dir_out[3 * i + k], want_sample[3 * i + k]);
    }
    for (size_t j = 0; j < nd; j++) bad += !same_f(pdf_out[j], want_pdf_of[j]);
    if (bad) { printf("case %u (%ux%u): %zu values differ from the expected ones\n", c, w, h, bad); bad_cases++; }
    draws += nu; dirs_n += nd;
  }
  if (in.at != in.w.size()) return 2;
  if (bad_cases) return 1;
  printf("env_image_sanitized: ok (%u maps, %zu draws, %zu directions)\n", ncases, draws, dirs_n);
  return 0;
}
#endif
