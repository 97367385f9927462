// emitter_ref.cpp - the reference's own Scene_Particles::step (scene/particles.cpp:101-162: the enabled / opt.dt exits, the substep loop,
// step2 with Particle::update, the cooldown loop and the spawn arithmetic, gen_instances) run frame by frame against a collide scene
// built the way Simulate::build_scene builds it (gui/simulate.cpp:69-99), for tests/golden/make_emitter_golden.py to record
// (tests/golden/emitter_*.npz: data only).
//
// INTEGRATION HARNESS, part of integration/_build/libdropin_pt_full.so, where scene/particles.cpp, student/particles.cpp, util/rand.cpp
// and the PT:: scene classes are compiled where they lie.  Nothing of the product runs here.  The library is built with
// -fno-access-control, so Scene_Particles::radius is set as given and last_update / particle_cooldown / particle_instances are read.
//
// util/rand.cpp's generator is a thread_local default-constructed std::mt19937: every run happens in a fresh std::thread, so it starts
// from the default seed, and a second default-constructed generator with the same uniform_real_distribution<float>(0, 1) mirrors the
// draws.  After the run one more RNG::unit() is compared with the mirror's next value: equal proves that the recorded uniforms are
// the ones the run consumed.
#include <cmath>
#include <cstdint>
#include <random>
#include <thread>
#include <vector>

#include "rays/object.h"
#include "scene/particles.h"
#include "util/rand.h"

namespace {

struct EmitterRun {
  // the collide scene: kind 0 a mesh (its slice of pos / nrm / idx), 1 a sphere (radius); T: Pose::transform(), 16 floats
  const uint32_t* kind; const uint32_t *vert_off, *idx_off; const float *pos, *nrm; const uint32_t* idx; const float *sphere_radius, *T; uint32_t nobj;
  float radius;                          // Scene_Particles::radius
  const float* options;                  // per frame: velocity, angle, scale, lifetime, pps, dt, enabled
  const float* pose;                     // per frame: pos3, euler3
  const float* frame_dt; uint32_t nframes;
  uint32_t cap;                          // particles recorded per frame
  uint32_t* count; float* particles;     // per frame: the vector's size; pos3, velocity3, age of the first min(size, cap)
  uint32_t *substeps, *spawns;           // per frame, from last_update / particle_cooldown before and after
  double* schedule;                      // per frame: last_update, particle_cooldown afterwards
  float* uniforms; uint32_t uniform_cap; uint32_t* nuniforms;
  int status;
};

void run(EmitterRun* R) {
  std::vector<PT::Object> obj_list;
  for (uint32_t i = 0; i < R->nobj; i++) {
    Mat4 M;
    for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++) M.cols[c][r] = R->T[16 * (size_t)i + 4 * c + r];
    if (R->kind[i] == 1) {
      PT::Shape shape{PT::Sphere(R->sphere_radius[i])};
      obj_list.push_back(PT::Object(std::move(shape), i + 1, 0, M));
    } else {
      const uint32_t v0 = R->vert_off[i], nv = R->vert_off[i + 1] - v0, i0 = R->idx_off[i], ni = R->idx_off[i + 1] - i0;
      std::vector<GL::Mesh::Vert> verts(nv);
      for (uint32_t v = 0; v < nv; v++) {
        const float *p = R->pos + 3 * (size_t)(v0 + v), *n = R->nrm + 3 * (size_t)(v0 + v);
        verts[v] = {Vec3(p[0], p[1], p[2]), Vec3(n[0], n[1], n[2]), 0};
      }
      std::vector<GL::Mesh::Index> indices(R->idx + i0, R->idx + i0 + ni);
      GL::Mesh gl_mesh(std::move(verts), std::move(indices));
      PT::Tri_Mesh mesh(gl_mesh, true);
      obj_list.push_back(PT::Object(std::move(mesh), i + 1, 0, M));
    }
  }
  PT::Object scene(PT::BVH<PT::Object>(std::move(obj_list)));

  Scene_Particles sp(1);
  sp.radius = R->radius;
  uint64_t total_spawns = 0;
  for (uint32_t f = 0; f < R->nframes; f++) {
    const float* o = R->options + 7 * (size_t)f;
    sp.opt.velocity = o[0]; sp.opt.angle = o[1]; sp.opt.scale = o[2]; sp.opt.lifetime = o[3]; sp.opt.pps = o[4]; sp.opt.dt = o[5];
    sp.opt.enabled = o[6] != 0.0f;
    const float* p = R->pose + 6 * (size_t)f;
    sp.pose.pos = Vec3(p[0], p[1], p[2]);
    sp.pose.euler = Vec3(p[3], p[4], p[5]);
    const double last0 = sp.last_update, cool0 = sp.particle_cooldown;
    sp.step(scene, R->frame_dt[f]);
    const double last1 = sp.last_update, cool1 = sp.particle_cooldown;
    // the counts, measured on the schedule's own variables: every substep took opt.dt off both, every spawn put 1 / pps onto the cooldown
    uint32_t substeps = 0, spawns = 0;
    if (sp.opt.enabled && !(sp.opt.dt < EPS_F)) {
      substeps = (uint32_t)std::llround((last0 + (double)R->frame_dt[f] - last1) / (double)sp.opt.dt);
      if (sp.opt.pps > 0.0f) spawns = (uint32_t)std::llround((cool1 - cool0 + (double)substeps * (double)sp.opt.dt) * (double)sp.opt.pps);
    }
    R->substeps[f] = substeps; R->spawns[f] = spawns;
    total_spawns += spawns;
    R->schedule[2 * (size_t)f] = last1; R->schedule[2 * (size_t)f + 1] = cool1;
    const std::vector<Scene_Particles::Particle>& ps = sp.get_particles();
    R->count[f] = (uint32_t)ps.size();
    if (sp.opt.enabled && !(sp.opt.dt < EPS_F) && sp.particle_instances.data.size() != ps.size()) { R->status = -3; return; }   // gen_instances
    for (uint32_t k = 0; k < ps.size() && k < R->cap; k++) {
      float* out = R->particles + 7 * ((size_t)f * R->cap + k);
      out[0] = ps[k].pos.x; out[1] = ps[k].pos.y; out[2] = ps[k].pos.z;
      out[3] = ps[k].velocity.x; out[4] = ps[k].velocity.y; out[5] = ps[k].velocity.z;
      out[6] = ps[k].age;
    }
  }
  // the mirror of util/rand.cpp
  std::mt19937 mirror;
  auto unit = [&mirror]() { std::uniform_real_distribution<float> d(0.0f, 1.0f); return d(mirror); };
  if (2 * total_spawns > R->uniform_cap) { R->status = -2; return; }
  for (uint64_t k = 0; k < 2 * total_spawns; k++) R->uniforms[k] = unit();
  *R->nuniforms = (uint32_t)(2 * total_spawns);
  const float next_ref = RNG::unit(), next_mirror = unit();
  R->status = next_ref == next_mirror ? 0 : -1;
}

}  // namespace

extern "C" {

// Returns 0; -1: the mirror generator is not aligned with the run's (the spawn counts are wrong); -2: uniform_cap too small; -3:
// gen_instances left another number of instances than particles.
__attribute__((visibility("default")))
int dropin_emitter_reference(const uint32_t* kind, const uint32_t* vert_off, const uint32_t* idx_off, const float* pos, const float* nrm, const uint32_t* idx,
                             const float* sphere_radius, const float* T, uint32_t nobj, float radius, const float* options, const float* pose,
                             const float* frame_dt, uint32_t nframes, uint32_t cap, uint32_t* count, float* particles, uint32_t* substeps, uint32_t* spawns,
                             double* schedule, float* uniforms, uint32_t uniform_cap, uint32_t* nuniforms) {
  EmitterRun R{kind, vert_off, idx_off, pos, nrm, idx, sphere_radius, T, nobj, radius, options, pose, frame_dt, nframes, cap, count, particles,
               substeps, spawns, schedule, uniforms, uniform_cap, nuniforms, -4};
  std::thread t(run, &R);
  t.join();
  return R.status;
}

}  // extern "C"
