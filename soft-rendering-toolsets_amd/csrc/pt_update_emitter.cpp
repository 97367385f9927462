// srt_pt_emitter: Scene_Particles::step for a pool of fixed capacity whose slots are objects of a committed scene.  The schedule runs
// here, on the host (pt_emitter.h: emitter_plan_step); per substep two launches of pt_emitter.hip go onto the caller's stream; present is
// srt_pt_particle_transforms_device, srt_pt_set_active_device and srt_pt_repose_refit_device on the render context.  Host code only.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_emitter.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

struct srt_pt_emitter : SceneHandle {
  srt_pt* collide = nullptr;
  std::vector<uint32_t> objects;
  float radius = 0.0f;
  EmitterOptions opt;
  float pos[3] = {0.0f, 0.0f, 0.0f}, euler[3] = {0.0f, 0.0f, 0.0f};   // Pose::id()
  EmitterSchedule schedule;
  uint64_t seed = 0;
  const float* d_uniforms = nullptr; size_t nuniforms = 0;
  uint64_t born = 0;                                      // birth ordinals consumed so far
  EmitterPlan plan;                                       // scratch of one step
  DeviceBuffer<float> d_pos, d_vel, d_age, d_trans;
  DeviceBuffer<uint8_t> d_alive;
  DeviceBuffer<uint32_t> d_birth, d_wave_dead, d_counters;

  uint32_t capacity() const { return (uint32_t)objects.size(); }
  EmitterPool pool() const { return {d_pos, d_vel, d_age, d_alive, d_birth, d_wave_dead, d_counters, capacity()}; }
};

namespace {

int emitter_usable(const srt_pt_emitter* em, const char* what) {
  if (!em) return srt::fail(SRT_ERR_INVALID, "%s: NULL emitter", what);
  if (em->stale()) return srt::fail(SRT_ERR_STATE, "%s: the emitter is stale - its render context's scene was begun or committed again after srt_pt_emitter_create", what);
  return SRT_OK;
}

// Usable and on a device context, the device current.
int emitter_on_device(const srt_pt_emitter* em, const char* what) {
  const int st = emitter_usable(em, what);
  if (st != SRT_OK) return st;
  if (em->pt->device < 0) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the pool lives on the device only; this context is host-only", what);
  SRT_HIP(hipSetDevice(em->pt->device));
  return SRT_OK;
}

// The schedule of one step into em->plan, the uniform buffer checked against the call's last ordinal; on a refusal nothing changed.
int emitter_plan(srt_pt_emitter* em, const char* what, float dt) {
  const EmitterSchedule before = em->schedule;
  const int over = emitter_plan_step(&em->schedule, em->opt, dt, &em->plan);
  if (over == 1) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: dt %g with Options::dt %g needs more than %u substeps in one call", what, dt, em->opt.dt, kEmitterMaxSubsteps);
  if (over == 2) return srt::fail(SRT_ERR_UNSUPPORTED, "%s: pps %g with Options::dt %g needs more than %u spawns in one substep", what, em->opt.pps, em->opt.dt, kEmitterMaxSpawns);
  uint64_t spawns = 0;
  for (uint32_t i = 0; i < em->plan.nsubsteps; i++) spawns += em->plan.spawns[i];
  const uint64_t last = em->born + spawns;
  const char* refused = nullptr;
  if (last > 0xffffffffull) refused = "the birth ordinals would pass 2^32";
  else if (em->d_uniforms && 2 * last > em->nuniforms) refused = "the uniform buffer is too short for this call's spawns (two floats per birth ordinal)";
  if (refused) {
    em->schedule = before;
    return srt::fail(last > 0xffffffffull ? SRT_ERR_UNSUPPORTED : SRT_ERR_INVALID, "%s: %s: %llu ordinals, %zu floats", what, refused, (unsigned long long)last, em->nuniforms);
  }
  return SRT_OK;
}

// The planned step's launches on s.
int emitter_enqueue(srt_pt_emitter* em, const char* what, hipStream_t s) {
  const EmitterPool P = em->pool();
  if (em->plan.clear) {
    launch_emitter_clear(s, P);
  } else if (em->plan.nsubsteps) {
    const EmitterLaunch L = emitter_launch(em->opt, em->pos, em->euler);
    const float radius = em->radius * em->opt.scale;
    for (uint32_t i = 0; i < em->plan.nsubsteps; i++) {
      launch_emitter_step(s, em->collide, P, em->opt.dt, radius);
      launch_emitter_spawn(s, P, L, em->plan.spawns[i], (uint32_t)em->born, em->d_uniforms, em->seed, em->objects[0]);
      em->born += em->plan.spawns[i];
    }
  }
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

// What a step needs of the collide context: a committed scene (no settle(): the device forms only enqueue).
int collide_ready(const srt_pt_emitter* em, const char* what) {
  if (!em->collide->committed) return srt::fail(SRT_ERR_STATE, "%s: the collide context holds no committed scene", what);
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_pt_emitter_create(srt_pt* render, srt_pt* collide, const uint32_t* objects, uint32_t capacity, float radius, srt_pt_emitter** out) {
  const char* what = "srt_pt_emitter_create";
  if (out) *out = nullptr;
  if (!render || !collide || !objects || !out) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if (!capacity) return srt::fail(SRT_ERR_INVALID, "%s: a pool of no slots", what);
  int st;
  if ((st = need_committed(render, what))) return st;
  if (collide != render && (st = need_committed(collide, what))) return st;
  if (collide->device != render->device) return srt::fail(SRT_ERR_INVALID, "%s: the collide context is on device %d, the render context on %d", what, collide->device, render->device);
  bool unsupported = false;
  const std::string refused = check_active_list(render->built, objects, capacity, &unsupported);
  if (!refused.empty()) return srt::fail(unsupported ? SRT_ERR_UNSUPPORTED : SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt_emitter* em = new (std::nothrow) srt_pt_emitter;
  if (!em) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  em->pt = render; em->generation = render->scene_generation;
  em->collide = collide;
  em->objects.assign(objects, objects + capacity);
  em->radius = radius;
  return handle_publish(em, out, [&]() -> int {
    SRT_HIP(hipSetDevice(render->device));
    const size_t n = capacity, nwaves = (n + 63) / 64;
    int w;
    if ((w = em->d_pos.ensure(3 * n)) || (w = em->d_vel.ensure(3 * n)) || (w = em->d_age.ensure(n)) || (w = em->d_trans.ensure(16 * n)) || (w = em->d_alive.ensure(n)) ||
        (w = em->d_birth.ensure(n)) || (w = em->d_wave_dead.ensure(nwaves)) || (w = em->d_counters.ensure(2)))
      return w;
    SRT_HIP(hipMemset(em->d_pos, 0, 12 * n)); SRT_HIP(hipMemset(em->d_vel, 0, 12 * n)); SRT_HIP(hipMemset(em->d_age, 0, 4 * n));
    SRT_HIP(hipMemset(em->d_trans, 0, 64 * n)); SRT_HIP(hipMemset(em->d_alive, 0, n)); SRT_HIP(hipMemset(em->d_birth, 0, 4 * n));
    SRT_HIP(hipMemset(em->d_wave_dead, 0, 4 * nwaves)); SRT_HIP(hipMemset(em->d_counters, 0, 8));
    SRT_HIP(hipDeviceSynchronize());
    return SRT_OK;
  });
}

int srt_pt_emitter_destroy(srt_pt_emitter* em) {
  if (em && em->collide != em->pt && em->collide->device >= 0) (void)quiesce(em->collide);
  return handle_destroy(em);
}

int srt_pt_emitter_set_options(srt_pt_emitter* em, float velocity, float angle, float scale, float lifetime, float pps, float dt, int enabled) {
  const int st = emitter_usable(em, "srt_pt_emitter_set_options");
  if (st != SRT_OK) return st;
  em->opt.velocity = velocity; em->opt.angle = angle; em->opt.scale = scale; em->opt.lifetime = lifetime; em->opt.pps = pps; em->opt.dt = dt;
  em->opt.enabled = enabled != 0;
  return SRT_OK;
}

int srt_pt_emitter_set_pose(srt_pt_emitter* em, const float* pos3, const float* euler3) {
  const int st = emitter_usable(em, "srt_pt_emitter_set_pose");
  if (st != SRT_OK) return st;
  if (!pos3 || !euler3) return srt::fail(SRT_ERR_INVALID, "srt_pt_emitter_set_pose: NULL argument");
  std::memcpy(em->pos, pos3, sizeof em->pos);
  std::memcpy(em->euler, euler3, sizeof em->euler);
  return SRT_OK;
}

int srt_pt_emitter_seed(srt_pt_emitter* em, uint64_t seed) {
  const int st = emitter_usable(em, "srt_pt_emitter_seed");
  if (st != SRT_OK) return st;
  em->seed = seed;
  return SRT_OK;
}

int srt_pt_emitter_set_uniforms_device(srt_pt_emitter* em, const float* d_uniforms, size_t n) {
  const int st = emitter_usable(em, "srt_pt_emitter_set_uniforms_device");   // (a pointer and a length: kept, not read)
  if (st != SRT_OK) return st;
  em->d_uniforms = n ? d_uniforms : nullptr;
  em->nuniforms = d_uniforms ? n : 0;
  return SRT_OK;
}

int srt_pt_emitter_step_device(srt_pt_emitter* em, void* stream, float dt) {
  const char* what = "srt_pt_emitter_step_device";
  int st;
  if ((st = emitter_on_device(em, what)) || (st = collide_ready(em, what)) || (st = emitter_plan(em, what, dt))) return st;
  return emitter_enqueue(em, what, (hipStream_t)stream);
}

int srt_pt_emitter_step(srt_pt_emitter* em, float dt) {
  const char* what = "srt_pt_emitter_step";
  int st;
  if ((st = emitter_on_device(em, what))) return st;
  if ((st = need_committed(em->collide, what))) return st;   // (settles: the host form sees what the enqueue-only calls left)
  if ((st = emitter_plan(em, what, dt)) || (st = emitter_enqueue(em, what, em->pt->stream))) return st;
  SRT_HIP(hipStreamSynchronize(em->pt->stream));
  return SRT_OK;
}

int srt_pt_emitter_present_device(srt_pt_emitter* em, void* stream) {
  const char* what = "srt_pt_emitter_present_device";
  int st;
  if ((st = emitter_on_device(em, what))) return st;
  const uint32_t n = em->capacity();
  if ((st = srt_pt_particle_transforms_device(em->pt, stream, em->d_pos, n, em->opt.scale, em->d_trans))) return st;
  if ((st = srt_pt_set_active_device(em->pt, stream, em->objects.data(), em->d_alive, n))) return st;
  return srt_pt_repose_refit_device(em->pt, stream, em->objects.data(), em->d_trans, n);
}

int srt_pt_emitter_frame_device(srt_pt_emitter* em, void* stream, float dt) {
  const int st = srt_pt_emitter_step_device(em, stream, dt);
  return st != SRT_OK ? st : srt_pt_emitter_present_device(em, stream);
}

int srt_pt_emitter_clear_device(srt_pt_emitter* em, void* stream) {
  const int st = emitter_on_device(em, "srt_pt_emitter_clear_device");
  if (st != SRT_OK) return st;
  launch_emitter_clear(stream, em->pool());
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_emitter_clear(srt_pt_emitter* em) {
  int st = emitter_on_device(em, "srt_pt_emitter_clear");
  if (st != SRT_OK) return st;
  if ((st = srt_pt_emitter_clear_device(em, (void*)em->pt->stream))) return st;
  SRT_HIP(hipStreamSynchronize(em->pt->stream));
  return SRT_OK;
}

int srt_pt_emitter_read(srt_pt_emitter* em, float* pos, float* vel, float* age, uint8_t* alive, uint32_t* birth) {
  const int st = emitter_on_device(em, "srt_pt_emitter_read");
  if (st != SRT_OK) return st;
  const size_t n = em->capacity();
  SRT_HIP(hipDeviceSynchronize());
  if (pos) SRT_HIP(hipMemcpy(pos, em->d_pos, 12 * n, hipMemcpyDeviceToHost));
  if (vel) SRT_HIP(hipMemcpy(vel, em->d_vel, 12 * n, hipMemcpyDeviceToHost));
  if (age) SRT_HIP(hipMemcpy(age, em->d_age, 4 * n, hipMemcpyDeviceToHost));
  if (alive) SRT_HIP(hipMemcpy(alive, em->d_alive, n, hipMemcpyDeviceToHost));
  if (birth) SRT_HIP(hipMemcpy(birth, em->d_birth, 4 * n, hipMemcpyDeviceToHost));
  return SRT_OK;
}

int srt_pt_emitter_write(srt_pt_emitter* em, const float* pos, const float* vel, const float* age, const uint8_t* alive, const uint32_t* birth) {
  const int st = emitter_on_device(em, "srt_pt_emitter_write");
  if (st != SRT_OK) return st;
  const size_t n = em->capacity();
  SRT_HIP(hipDeviceSynchronize());
  if (pos) SRT_HIP(hipMemcpy(em->d_pos, pos, 12 * n, hipMemcpyHostToDevice));
  if (vel) SRT_HIP(hipMemcpy(em->d_vel, vel, 12 * n, hipMemcpyHostToDevice));
  if (age) SRT_HIP(hipMemcpy(em->d_age, age, 4 * n, hipMemcpyHostToDevice));
  if (alive) SRT_HIP(hipMemcpy(em->d_alive, alive, n, hipMemcpyHostToDevice));
  if (birth) SRT_HIP(hipMemcpy(em->d_birth, birth, 4 * n, hipMemcpyHostToDevice));
  SRT_HIP(hipDeviceSynchronize());
  return SRT_OK;
}

int srt_pt_emitter_counts(srt_pt_emitter* em, uint64_t out[3]) {
  const int st = emitter_usable(em, "srt_pt_emitter_counts");
  if (st != SRT_OK) return st;
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_emitter_counts: NULL argument");
  out[0] = 0; out[1] = em->born; out[2] = 0;
  if (em->pt->device < 0) return SRT_OK;
  std::vector<uint8_t> alive(em->capacity());
  uint32_t counters[2] = {0, 0};
  SRT_HIP(hipSetDevice(em->pt->device));
  SRT_HIP(hipDeviceSynchronize());
  SRT_HIP(hipMemcpy(alive.data(), em->d_alive, alive.size(), hipMemcpyDeviceToHost));
  SRT_HIP(hipMemcpy(counters, em->d_counters, sizeof counters, hipMemcpyDeviceToHost));
  for (uint8_t a : alive) out[0] += a ? 1 : 0;
  out[2] = counters[0];
  return SRT_OK;
}

int srt_pt_emitter_arrays_device(srt_pt_emitter* em, void* out[5]) {
  const int st = emitter_on_device(em, "srt_pt_emitter_arrays_device");
  if (st != SRT_OK) return st;
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_emitter_arrays_device: NULL argument");
  out[0] = em->d_pos; out[1] = em->d_vel; out[2] = em->d_age; out[3] = em->d_alive; out[4] = em->d_birth;
  return SRT_OK;
}

int srt_pt_emitter_advance_host(srt_pt_emitter* em, float dt, uint32_t* substeps, uint32_t* spawns_out, uint32_t cap, int* cleared, double schedule_out[2]) {
  const char* what = "srt_pt_emitter_advance_host";
  int st = emitter_usable(em, what);
  if (st != SRT_OK) return st;
  if (!substeps || !cleared || (cap && !spawns_out)) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if ((st = emitter_plan(em, what, dt))) return st;
  *substeps = em->plan.nsubsteps;
  *cleared = em->plan.clear ? 1 : 0;
  for (uint32_t i = 0; i < em->plan.nsubsteps; i++) {
    if (i < cap) spawns_out[i] = em->plan.spawns[i];
    em->born += em->plan.spawns[i];
  }
  if (schedule_out) { schedule_out[0] = em->schedule.last_update; schedule_out[1] = em->schedule.particle_cooldown; }
  return SRT_OK;
}

}  // extern "C"
