// env_sampler_ref.cpp - the REFERENCE's Samplers::Sphere::Image (student/samplers.cpp:27-137) on its own, with a settable RNG::unit:
// the tables its constructor builds, sample() for a chosen draw and pdf() for a chosen direction.  Calls only; nothing of the
// reference is copied.  Linked with student/samplers.cpp and util/hdr_image.cpp where they lie (integration/Makefile).
//
// TEST INFRASTRUCTURE ONLY.  Output: integration/_build/libref_env_sampler.so (git-ignored), used by
// tests/golden/make_env_image_golden.py for the component fixture.  Compiled with -fno-access-control (this translation unit only).
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "rays/samplers.h"
#include "util/hdr_image.h"
#include "util/rand.h"

namespace {
thread_local float g_unit = 0.0f;   // what the next RNG::unit() returns
}

namespace RNG {   // the seam (util/rand.cpp is not linked)
float unit() { return g_unit; }
int integer(int min, int) { return min; }
bool coin_flip(float p) { return g_unit < p; }
void seed() {}
}  // namespace RNG

#pragma GCC visibility push(default)
extern "C" {

void* ref_env_sampler_create(uint32_t w, uint32_t h, const float* rgb) {
  HDR_Image img(w, h);
  for (size_t i = 0; i < (size_t)w * h; i++) img.at(i) = Spectrum(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
  return new Samplers::Sphere::Image(img);
}
void ref_env_sampler_destroy(void* s) { delete (Samplers::Sphere::Image*)s; }

// _pdf, _cdf (w * h floats each) and total
void ref_env_sampler_tables(void* s, float* pdf, float* cdf, float* total) {
  const Samplers::Sphere::Image* im = (const Samplers::Sphere::Image*)s;
  std::copy(im->_pdf.begin(), im->_pdf.end(), pdf);
  std::copy(im->_cdf.begin(), im->_cdf.end(), cdf);
  *total = im->total;
}

// sample() with RNG::unit() == u[i]; index_out: what the library's std::upper_bound returns for the same table and draw
void ref_env_sampler_sample(void* s, const float* u, size_t n, float* dir_out, uint32_t* index_out) {
  const Samplers::Sphere::Image* im = (const Samplers::Sphere::Image*)s;
  for (size_t i = 0; i < n; i++) {
    g_unit = u[i];
    const Vec3 d = im->sample();
    dir_out[3 * i] = d.x; dir_out[3 * i + 1] = d.y; dir_out[3 * i + 2] = d.z;
    index_out[i] = (uint32_t)(std::upper_bound(im->_cdf.begin(), im->_cdf.end(), u[i]) - im->_cdf.begin());
  }
}

void ref_env_sampler_pdf(void* s, const float* dirs, size_t n, float* pdf_out) {
  const Samplers::Sphere::Image* im = (const Samplers::Sphere::Image*)s;
  for (size_t i = 0; i < n; i++) pdf_out[i] = im->pdf(Vec3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]));
}

}  // extern "C"
#pragma GCC visibility pop
