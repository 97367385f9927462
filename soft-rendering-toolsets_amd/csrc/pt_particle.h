// Scene_Particles::Particle::update (student/particles.cpp:5-59) for one lane's particle: the second caller of Object::hit
// (SURVEY.md 8(f)-4).  What pt_particles_kernel (pt_query.hip) runs for every particle and the emitter's masked step
// (pt_emitter.hip) for the alive slots of its pool.  Device code only.
#ifndef SRT_PT_PARTICLE_H
#define SRT_PT_PARTICLE_H

#include "pt_trace.h"

namespace srt {

// The reference's loop does not return when hit_time stays <= 0; a lane gives up after kParticleMaxLegs legs.
constexpr uint32_t kParticleMaxLegs = 4096;

// The particle flies at constant velocity for what is left of dt, bounces off what scene.hit(Ray(pos, velocity)) reports - default
// bounds [0, inf], the direction is the velocity, NOT normalised - and gravity acts on the velocity after every leg.  p and
// velocity are updated in place; the age is the caller's.
SRT_DEV void particle_update(const DScene& S, V3& p, V3& velocity, float dt, float radius) {
  const V3 acceleration = v3(0.0f, -9.8f, 0.0f);
  float remain = dt;
  Counters cnt;
  for (uint32_t leg = 0; remain > 0 && leg < kParticleMaxLegs; leg++) {
    Ray r;
    r.o = p; r.d = velocity; r.b0 = 0.0f; r.b1 = __uint_as_float(0x7f800000u);
    const Hit h = scene_hit<false>(S, r, cnt);
    V3 t_normal = v3(0, 0, 0), t_position = v3(0, 0, 0);       // a Trace without a hit is all zeros (rays/trace.h)
    if (h.hit) { const Surface sf = surface_of(S, h, r); t_normal = sf.normal; t_position = sf.position; }
    float cos_t = dot(t_normal, velocity * -1.0f) / (norm(velocity) * norm(t_normal));
    V3 surface_normal = t_normal / norm(t_normal);
    if (cos_t < 0) {
      cos_t = (float)sqrt((double)(1 - cos_t * cos_t));          // unqualified sqrt: the double overload
      surface_normal = surface_normal * -1.0f;
    }
    const float interval = fabsf(radius / cos_t);
    const float hit_time = (h.dist - interval) / norm(r.d);
    if (!h.hit || hit_time > remain || cos_t == 0) {
      p = p + velocity * remain;
      velocity = velocity + acceleration * remain;
      break;
    }
    p = t_position - (velocity * interval) / norm(velocity);
    velocity = velocity - surface_normal * (2.0f * dot(velocity, surface_normal));
    velocity = velocity + acceleration * hit_time;
    remain -= hit_time;
  }
}

}  // namespace srt

#endif
