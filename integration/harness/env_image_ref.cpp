// env_image_ref.cpp - the REFERENCE's path tracer with "step two" of its Task 7 switched on: Env_Map::sample / Env_Map::pdf
// (student/env_light.cpp:8-32 render with uniform_sampler) answered by the map's own image_sampler, the Samplers::Sphere::Image the
// constructor builds and the fork never uses (rays/env_light.h:43-52).  Nothing of the reference is edited or copied: the linker
// redirects the two member functions here (-Wl,--wrap=..., integration/Makefile) and the wrappers below only CALL the reference.
// Linked with oracle/ref_harness/pt_ref.cpp as it is, whose RNG seam and ref_pt_* exports come along unchanged.
//
// TEST INFRASTRUCTURE ONLY.  Output: integration/_build/libref_pt_envimage.so (git-ignored), used by
// tests/golden/make_env_image_golden.py.  Compiled with -fno-access-control (this translation unit only).
#include <atomic>
#include <cstdint>

#include "rays/env_light.h"

namespace {
std::atomic<uint64_t> g_sample_calls{0}, g_pdf_calls{0};
}

// PT::Env_Map::sample() const / PT::Env_Map::pdf(Vec3) const, by their mangled names
extern "C" Vec3 __wrap__ZNK2PT7Env_Map6sampleEv(const PT::Env_Map* m) {
  g_sample_calls.fetch_add(1, std::memory_order_relaxed);
  return m->image_sampler.sample();
}
extern "C" float __wrap__ZNK2PT7Env_Map3pdfE4Vec3(const PT::Env_Map* m, Vec3 dir) {
  g_pdf_calls.fetch_add(1, std::memory_order_relaxed);
  return m->image_sampler.pdf(dir);
}

#pragma GCC visibility push(default)
extern "C" {
// calls of the two wrappers since the last reset: {sample, pdf}
void ref_env_image_calls(uint64_t out[2], int reset) {
  out[0] = g_sample_calls.load(); out[1] = g_pdf_calls.load();
  if (reset) { g_sample_calls = 0; g_pdf_calls = 0; }
}
}
#pragma GCC visibility pop
