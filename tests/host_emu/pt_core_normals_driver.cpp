// TEST-ONLY: srt_host::RenderCore (soft-rendering-toolsets_amd/host/pathtracer_core.{h,cpp}) against a STAND-IN of the group ABI
// that records the order of the calls it receives - no device, no product library.  tests/test_pt_normals_host.py uses it to
// show that RenderCore::begin forwards the normal-colors switch (srt_pt_group_set_normal_colors) before the first launch of a
// render, and again - with the new value - after the switch was flipped between two renders.
// Every entry point RenderCore calls is defined here; the launches "complete" at once and the accumulator image is never asked for.
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "pathtracer_core.h"

namespace {
std::mutex g_mut;
std::string g_log;            // one line per recorded call
int g_normal_colors = -1;     // what the stand-in group holds (-1: never set)
void note(const char* what, long a = -1, long b = -1) {
  std::lock_guard<std::mutex> lock(g_mut);
  char line[96];
  if (a < 0) std::snprintf(line, sizeof line, "%s\n", what);
  else if (b < 0) std::snprintf(line, sizeof line, "%s %ld\n", what, a);
  else std::snprintf(line, sizeof line, "%s %ld %ld\n", what, a, b);
  g_log += line;
}
void fatal(const char* what, int status, const char* message) {
  std::fprintf(stderr, "[pt_core_normals_driver] %s failed (%d): %s\n", what, status, message);
  note("fatal");
}
int g_group_tag = 0, g_ctx_tag = 0;
}  // namespace

extern "C" {

// ---- the stand-in ABI (only what pathtracer_core.cpp references) ----
const char* srt_last_error(void) { return ""; }
int srt_pt_create_multi(const int*, int, srt_pt_group** out) { *out = reinterpret_cast<srt_pt_group*>(&g_group_tag); return SRT_OK; }
int srt_pt_group_destroy(srt_pt_group*) { return SRT_OK; }
int srt_pt_group_size(srt_pt_group*) { return 1; }
srt_pt* srt_pt_group_context(srt_pt_group*, int) { return reinterpret_cast<srt_pt*>(&g_ctx_tag); }
int srt_pt_set_elision(srt_pt*, int) { return SRT_OK; }
int srt_pt_group_set_ray_log(srt_pt_group*, uint32_t) { return SRT_OK; }
int srt_pt_group_set_params(srt_pt_group*, uint32_t, uint32_t, uint32_t) { note("set_params"); return SRT_OK; }
int srt_pt_group_reset_accumulator(srt_pt_group*) { return SRT_OK; }
int srt_pt_group_max_samples_per_launch(srt_pt_group*, uint32_t* samples) { *samples = 64; return SRT_OK; }
int srt_pt_group_set_normal_colors(srt_pt_group*, int on) { g_normal_colors = on; note("set_normal_colors", on); return SRT_OK; }
int srt_pt_set_camera(srt_pt*, const float*, float, float) { note("set_camera"); return SRT_OK; }
int srt_pt_group_render_samples(srt_pt_group*, int, uint64_t, uint32_t base, uint32_t n) {
  note("render_samples", (long)base, (long)n);
  note("launch_sees_normal_colors", g_normal_colors);
  return SRT_OK;
}
int srt_pt_group_wait_lane(srt_pt_group*, int) { return SRT_OK; }
int srt_pt_group_cancel_requested(srt_pt_group*) { return 0; }
int srt_pt_group_fold(srt_pt_group*, int, uint32_t, uint32_t, uint32_t, uint32_t) { note("fold"); return SRT_OK; }
int srt_pt_group_read_ray_log(srt_pt_group*, int, srt_pt_logged_ray*, size_t, size_t* n_out, uint64_t* dropped) {
  if (n_out) *n_out = 0;
  if (dropped) *dropped = 0;
  return SRT_OK;
}
int srt_pt_group_cancel(srt_pt_group*) { return SRT_OK; }
int srt_pt_group_clear_cancel(srt_pt_group*) { return SRT_OK; }
int srt_pt_group_accumulator_image(srt_pt_group*, float**, void**) { return SRT_ERR_STATE; }
int srt_pt_tonemap_device(srt_pt*, void*, const float*, uint32_t, uint32_t, float, uint8_t*) { return SRT_ERR_STATE; }

// ---- the driver ----
// Two renders of `samples` samples at 8 x 8 on one core: the first with the switch as `first`, the second with it as `second`
// (set between the renders, as the GUI's checkbox would).  Writes the recorded calls to `out` (NUL-terminated); returns their length.
size_t normals_driver_run(int first, int second, unsigned samples, char* out, size_t cap) {
  { std::lock_guard<std::mutex> lock(g_mut); g_log.clear(); g_normal_colors = -1; }
  const int device = 0;
  const float iview[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  {
    srt_host::RenderCore core(&device, 1, fatal);
    core.set_threads(1);
    core.set_params(8, 8, samples, 4);
    for (int on : {first, second}) {
      core.set_normal_colors(on != 0);
      note("begin");
      core.begin(iview, 60.0f, 1.0f, false);
      core.wait();
    }
  }
  std::lock_guard<std::mutex> lock(g_mut);
  const size_t n = g_log.size() < cap - 1 ? g_log.size() : cap - 1;
  std::memcpy(out, g_log.data(), n);
  out[n] = 0;
  return g_log.size();
}

}  // extern "C"
