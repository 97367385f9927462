// Scene_Particles::step (scene/particles.cpp:101-162) for a pool of fixed capacity, as functions for the device and the host: the
// schedule - `last_update`, `particle_cooldown`, the substep loop and step2's cooldown loop, which depend on the dts and the options
// only and therefore run on the host, with the reference's types and expressions - and the spawn arithmetic (:141-156), which
// pt_emitter.hip runs one lane per spawned slot.  The host emulation (tests/host_emu/emitter_host.cpp) compiles this header with
// g++ -ffp-contract=off.  Every function restates the reference operation for operation, in fp32 unless the reference widens, and
// nothing is built with contraction.
//
// Transcendentals are SRT-MATH v2 (pt_device.h): std::cos / std::sin of a float are cosf / sinf, restated by srt_sincosf, which is
// exact for |x| < 120 radians - the spawn's t = 2 PI_F u lies in [0, 2 pi] and Radians(angle) / 2 is below 120 for angles below
// 13750 degrees.
#ifndef SRT_PT_EMITTER_H
#define SRT_PT_EMITTER_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_anim.h"
#include "pt_device.h"

struct srt_pt;

namespace srt {

// Bounds of one srt_pt_emitter_step[_device] call.  The reference's loops have none: `while(last_update > opt.dt)` runs dt / opt.dt
// times and never ends once last_update is so large that subtracting opt.dt no longer changes it, and `while(particle_cooldown <=
// 0.0f)` never ends when adding 1.0 / pps no longer changes the cooldown.  A call that would need more is refused before
// anything is enqueued, and the schedule stays as it was.
constexpr uint32_t kEmitterMaxSubsteps = 4096;             // substeps of one call
constexpr uint32_t kEmitterMaxSpawns = 1u << 20;           // spawns of one substep

// Scene_Particles::Options without name and colour (scene/particles.h:56-66), with its defaults.
struct EmitterOptions {
  float velocity = 25.0f, angle = 0.0f, scale = 0.1f, lifetime = 15.0f, pps = 5.0f, dt = 0.01f;
  bool enabled = false;
};

// Scene_Particles::last_update and ::particle_cooldown (scene/particles.h:87-88): a float and a double.
struct EmitterSchedule {
  float last_update = 0.0f;
  double particle_cooldown = 0.0f;
};

// What one step(dt) enqueues: `clear` (the emitter is disabled), or spawns[i] spawns behind the update of substep i.
struct EmitterPlan {
  bool clear = false;
  uint32_t nsubsteps = 0;
  uint32_t spawns[kEmitterMaxSubsteps];
};

// step2's schedule half for one substep of length dt (:140-160): the spawn count.  false: more than kEmitterMaxSpawns.
inline bool emitter_substep_spawns(EmitterSchedule* s, const EmitterOptions& opt, float dt, uint32_t* spawns) {
  uint32_t k = 0;
  s->particle_cooldown -= dt;                                  // a double minus a float
  if (opt.pps > 0.0f) {
    const double cooldown = 1.0 / opt.pps;                     // in double
    while (s->particle_cooldown <= 0.0f) {
      if (k == kEmitterMaxSpawns) return false;
      k++;
      s->particle_cooldown += cooldown;
    }
  }
  *spawns = k;
  return true;
}

// Scene_Particles::step (:101-117) on the schedule alone.  0, or 1: more than kEmitterMaxSubsteps substeps, 2: more than
// kEmitterMaxSpawns spawns in one substep - then *s is unchanged.
inline int emitter_plan_step(EmitterSchedule* s, const EmitterOptions& opt, float dt, EmitterPlan* plan) {
  plan->clear = false;
  plan->nsubsteps = 0;
  if (!opt.enabled) { plan->clear = true; return 0; }
  if (opt.dt < kEps) return 0;
  EmitterSchedule next = *s;
  next.last_update += dt;
  while (next.last_update > opt.dt) {
    if (plan->nsubsteps == kEmitterMaxSubsteps) return 1;
    if (!emitter_substep_spawns(&next, opt, opt.dt, &plan->spawns[plan->nsubsteps])) return 2;
    plan->nsubsteps++;
    next.last_update -= opt.dt;
  }
  *s = next;
  return 0;
}

// What every spawn of a substep shares, computed once on the host and passed to the kernel by value: pose.pos, Mat4::euler(pose.euler)
// (pose.rotation_mat(), scene/pose.cpp:8-10), cos = std::cos(Radians(opt.angle) / 2.0f), opt.velocity and opt.lifetime.
struct EmitterLaunch {
  float pos[3];
  float rot[16];
  float cos_half, velocity, lifetime;
};

SRT_ANIM_FN EmitterLaunch emitter_launch(const EmitterOptions& opt, const float* pos3, const float* euler3) {
  EmitterLaunch L;
  for (int a = 0; a < 3; a++) L.pos[a] = pos3[a];
  anim_mat4_euler(anim_v3(euler3), L.rot);
  L.cos_half = srt_sincosf((opt.angle * (kPi / 180.0f)) / 2.0f, 1);   // Radians(v) = v * (PI_F / 180.0f)
  L.velocity = opt.velocity;
  L.lifetime = opt.lifetime;
  return L;
}

// The velocity of one spawn from its two uniforms (:147-154).  lerp is lib/mathlib.h:35, start + (end - start) * t; Mat4::rotate(v)
// is operator*(Vec4(v, 0.0f)).xyz() (lib/mat4.h:149-160): ((v0 * c0 + v1 * c1) + v2 * c2) + 0 * c3 per component, the last term kept.
SRT_ANIM_FN void emitter_spawn_velocity(const EmitterLaunch& L, float u0, float u1, float* vel3) {
  const float z = L.cos_half + (1.0f - L.cos_half) * u0;
  const float t = (2 * kPi) * u1;
  const float r = sqrtf(1 - z * z);
  float ct, st;
  srt_sincosf2(t, ct, st);
  const float dir[3] = {L.velocity * (r * ct), L.velocity * z, L.velocity * (r * st)};
  for (int a = 0; a < 3; a++)
    vel3[a] = ((dir[0] * L.rot[a] + dir[1] * L.rot[4 + a]) + dir[2] * L.rot[8 + a]) + 0.0f * L.rot[12 + a];
}

// The two uniforms of the spawn with birth ordinal b when no buffer is set: the first two draws of SRT-RNG v1 (pt_device.h: Rng,
// restated here for both sides) keyed (seed, emitter key, b) - the z one first, then the angle one.
SRT_ANIM_FN void emitter_uniforms(uint64_t seed, uint32_t key, uint32_t b, float* u0, float* u1) {
  const uint64_t k = ((uint64_t)key << 32) | b;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (k + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  const uint64_t inc = (k << 1) | 1;
  uint64_t state = z * 6364136223846793005ull + inc;
  float u[2];
  for (int i = 0; i < 2; i++) {
    const uint64_t old = state;
    state = old * 6364136223846793005ull + inc;
    const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27);
    const uint32_t rot = (uint32_t)(old >> 59);
    const uint32_t v = (xs >> rot) | (xs << ((32 - rot) & 31));
    u[i] = (float)(v >> 8) * (1.0f / 16777216.0f);
  }
  *u0 = u[0]; *u1 = u[1];
}

// The pool on the device: 3 floats per slot of pos and vel, one of age, a byte of alive, a word of birth; wave_dead holds one count
// per 64 slots, written by every masked step and read by the spawn behind it; counters[0] = spawns dropped so far.
struct EmitterPool {
  float *pos, *vel, *age;
  uint8_t* alive;
  uint32_t* birth;
  uint32_t* wave_dead;
  uint32_t* counters;
  uint32_t capacity;
};

// The launches of pt_emitter.hip.  `stream` is a hipStream_t; every call only enqueues.
// Particle::update for the alive slots against collide's committed scene (a dead slot is neither traced nor written), and every
// wave's dead count.
void launch_emitter_step(void* stream, const srt_pt* collide, const EmitterPool& P, float dt, float radius);
// The spawns with ordinals born .. born + k - 1 into the first k dead slots in ascending order; what finds no slot is counted in
// counters[0].  d_uniforms: the caller's buffer (2 floats per ordinal, checked by the caller) or NULL for emitter_uniforms(seed, key, b).
void launch_emitter_spawn(void* stream, const EmitterPool& P, const EmitterLaunch& L, uint32_t k, uint32_t born, const float* d_uniforms, uint64_t seed,
                          uint32_t key);
// alive = 0 for every slot
void launch_emitter_clear(void* stream, const EmitterPool& P);

}  // namespace srt

#endif
