// Samplers::Sphere::Image's constructor (student/samplers.cpp:37-79) and the trigonometry of its sample() (:103-112) on the host,
// once per environment map: what srt_pt_set_env_sampling(SRT_ENV_SAMPLING_IMAGE) uploads and env_image_sample / env_image_pdf
// (pt_trace.h) read.  Host code only, no HIP call: tests/host_emu builds the same tables with g++.
//
// The constructor accumulates `total` in float, serially, in row-major order, and _cdf[i] is the running total at texel i - that
// order IS the result (a scan on the device would add in another one), so the loop below is the reference's loop.  The quirks
// it keeps: a black map divides by total == 0 (NaN tables), a map with negative texels gives a _cdf that is not sorted.
#ifndef SRT_PT_ENV_IMAGE_H
#define SRT_PT_ENV_IMAGE_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "pt_device.h"

namespace srt {

struct EnvImageTables {
  std::vector<float> cdf_pdf;   // _cdf (w * h), then _pdf (w * h): 8 B per texel
  std::vector<double> trig;     // sin theta, cos theta of rows 0 .. h (h + 1 each), then cos phi, sin phi of columns 0 .. w - 1
  float total = 0.0f;
};

inline void build_env_image_tables(const float* rgb, uint32_t w, uint32_t h, EnvImageTables* out) {
  const size_t n = (size_t)w * h;
  out->cdf_pdf.assign(2 * n, 0.0f);
  float* cdf = out->cdf_pdf.data();
  float* pdf = cdf + n;
  float total = 0.0f;
  for (uint32_t row = 0; row < h; row++) {
    // std::sin(theta) of a float is sinf: the library's own restatement (SRT-MATH v2), not the installed libm
    const float theta = kPi - kPi * (float)row / (float)h;
    const float abs_sin = std::fabs(srt_sincosf(theta, 0));
    for (uint32_t col = 0; col < w; col++) {
      const float* p = rgb + 3 * ((size_t)row * w + col);
      const float luma = 0.2126f * p[0] + 0.7152f * p[1] + 0.0722f * p[2];   // Spectrum::luma(), lib/spectrum.h:111
      const float l_sin = luma * abs_sin;
      const size_t index = (size_t)row * w + col;
      pdf[index] = l_sin;
      total += l_sin;
      cdf[index] = total;
    }
  }
  for (size_t i = 0; i < n; i++) pdf[i] /= total;
  for (size_t i = 0; i < n; i++) cdf[i] /= total;
  out->total = total;
  // sample(): theta = clamp(PI_F - PI_F * row / h, 0, PI_F), phi = clamp(2 PI_F * col / w, 0, 2 PI_F) in float, then the DOUBLE
  // sin / cos of them (the unqualified calls of :110-112) - the C library's, evaluated here on the host.
  out->trig.resize(2 * ((size_t)h + 1) + 2 * (size_t)w);
  double* st = out->trig.data();
  double* ct = st + (h + 1);
  double* cp = ct + (h + 1);
  double* sp = cp + w;
  for (uint32_t row = 0; row <= h; row++) {
    float theta = kPi - kPi * (float)(int)row / (float)h;
    theta = (theta < 0.f) ? 0.f : ((kPi < theta) ? kPi : theta);           // std::clamp
    st[row] = std::sin((double)theta);
    ct[row] = std::cos((double)theta);
  }
  for (uint32_t col = 0; col < w; col++) {
    float phi = (2.0f * kPi) * (float)(int)col / (float)w;
    phi = (phi < 0.f) ? 0.f : (((2.0f * kPi) < phi) ? (2.0f * kPi) : phi);
    cp[col] = std::cos((double)phi);
    sp[col] = std::sin((double)phi);
  }
}

}  // namespace srt

#endif
