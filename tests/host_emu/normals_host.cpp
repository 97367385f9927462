// TEST-ONLY: normal_sample() of csrc/pt_trace.h - the per-sample function of the normal-colors view's kernels - compiled for the
// host and run one lane at a time, on top of flat_host.cpp's scene feeder.  tests/test_pt_normals_host.py compares it with
// tests/_normals_expected.py on the CPU; the HIP build of the same source is what the GPU tests check.
#include "flat_host.cpp"

extern "C" {

// env_type 0 / 1 / 2 with a uniform radiance (image maps are left to the GPU tests).  rgb: 3 floats per sample.
int emu_normal_samples(void* h, const float* iview, float vfov, float ar, uint32_t w, uint32_t hh, uint32_t env_type, const float* env_radiance,
                       uint64_t seed, const uint32_t* xs, const uint32_t* ys, const uint32_t* ss, size_t n, float* rgb, uint32_t* draws, uint32_t* rays) {
  Emu* e = (Emu*)h;
  DScene S = e->S;
  S.cam = make_camera(iview, vfov, ar);
  S.w = w; S.h = hh;
  S.env_type = env_type;
  for (int i = 0; i < 3; i++) S.env_radiance[i] = env_radiance ? env_radiance[i] : 0.0f;
  S.ray_log = nullptr; S.ray_log_cap = 0; S.elide = 0;
  for (size_t i = 0; i < n; i++) {
    Counters cnt;
    for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
    Rng rng;
    rng.key(seed, ys[i] * w + xs[i], ss[i]);
    const Spec p = normal_sample<true>(S, xs[i], ys[i], rng, cnt);
    rgb[3 * i] = p.r; rgb[3 * i + 1] = p.g; rgb[3 * i + 2] = p.b;
    draws[i] = rng.draws; rays[i] = cnt.v[C_RAYS];
  }
  return 0;
}

}  // extern "C"
