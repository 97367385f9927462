// The emitter's kernels (pt_emitter.h): Scene_Particles::step2 for a pool of fixed capacity, two launches per substep.
//
//   emitter_step_kernel   one wave per 64 slots, as pt_particles_kernel: Particle::update (pt_particle.h) for the alive slots only -
//                         a dead slot is neither traced nor written - and, after the verdicts, the wave's dead count
//                         (__popcll(__ballot(...)), one vector store by lane 0).
//   emitter_spawn_kernel  the k spawns of the substep into the first k dead slots in ascending slot index.  A wave owns the 64 slots
//                         the step's wave owned.  It sums the dead counts of the waves in front of it, 64 counts per pass with a
//                         butterfly reduction, and stops as soon as the sum reaches k: then it owns none of the first k dead
//                         slots and touches nothing.  Otherwise a dead lane's rank is that sum plus the dead lanes below it in
//                         the wave (ballot / mbcnt), and the lanes of rank < k spawn: ordinal born + rank, two uniforms, the
//                         velocity, pos, age, alive and birth.  The last wave sums every count and adds what found no slot
//                         to counters[0].
//   emitter_clear_kernel  alive = 0.
//
// Every index is inside its array: a lane touches slot s < capacity only, the count loops read wave_dead[i] for i < the wave's
// own index <= (capacity - 1) / 64, and the uniform buffer's length was checked against the last ordinal on the host.
#include <hip/hip_runtime.h>

#include "pt_context.h"
#include "pt_emitter.h"
#include "pt_particle.h"

namespace srt {
namespace {

__global__ __launch_bounds__(64) void emitter_step_kernel(DScene S, EmitterPool P, float dt, float radius) {
  const uint32_t k = blockIdx.x * 64u + threadIdx.x;
  const bool live = k < P.capacity && P.alive[k] != 0;
  bool dead = k < P.capacity;
  if (live) {
    V3 p = v3(P.pos[3 * k], P.pos[3 * k + 1], P.pos[3 * k + 2]);
    V3 velocity = v3(P.vel[3 * k], P.vel[3 * k + 1], P.vel[3 * k + 2]);
    particle_update(S, p, velocity, dt, radius);
    const float a = P.age[k] - dt;
    P.age[k] = a;
    dead = !(a > 0);
    P.alive[k] = dead ? 0 : 1;
    P.pos[3 * k] = p.x; P.pos[3 * k + 1] = p.y; P.pos[3 * k + 2] = p.z;
    P.vel[3 * k] = velocity.x; P.vel[3 * k + 1] = velocity.y; P.vel[3 * k + 2] = velocity.z;
  }
  const uint32_t ndead = (uint32_t)__popcll(__ballot(dead));
  if (threadIdx.x == 0) P.wave_dead[blockIdx.x] = ndead;
}

constexpr uint32_t kSpawnBlock = 256;                      // four waves: four runs of 64 slots

__global__ __launch_bounds__(kSpawnBlock) void emitter_spawn_kernel(EmitterPool P, EmitterLaunch L, uint32_t nspawn, uint32_t born,
                                                                    const float* __restrict__ uniforms, uint64_t seed, uint32_t key) {
  const uint32_t slot = blockIdx.x * kSpawnBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = slot >> 6;                          // the same for the 64 lanes of a wave
  const uint32_t nwaves = (P.capacity + 63u) >> 6;
  if (wave >= nwaves) return;                               // (whole waves beyond the pool)
  const bool last = wave == nwaves - 1u;
  // the dead slots in front of this wave's
  uint32_t before = 0;
  for (uint32_t base = 0; base < wave; base += 64u) {
    uint32_t v = base + lane < wave ? P.wave_dead[base + lane] : 0u;
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    before += v;
    if (before >= nspawn && !last) return;                  // wave-uniform: the first nspawn dead slots lie in front
  }
  const bool dead = slot < P.capacity && P.alive[slot] == 0;
  const unsigned long long mask = __ballot(dead);
  const uint32_t rank = before + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  if (last && lane == 0) {
    const uint32_t total = before + (uint32_t)__popcll(mask);
    if (nspawn > total) P.counters[0] += nspawn - total;    // one lane of one wave of a stream-ordered launch: no other writer
  }
  if (!dead || rank >= nspawn) return;
  const uint32_t b = born + rank;
  float u0, u1;
  if (uniforms) { u0 = uniforms[2 * (size_t)b]; u1 = uniforms[2 * (size_t)b + 1]; }
  else emitter_uniforms(seed, key, b, &u0, &u1);
  float v[3];
  emitter_spawn_velocity(L, u0, u1, v);
  for (int a = 0; a < 3; a++) { P.pos[3 * (size_t)slot + a] = L.pos[a]; P.vel[3 * (size_t)slot + a] = v[a]; }
  P.age[slot] = L.lifetime;
  P.alive[slot] = 1;
  P.birth[slot] = b;
}

__global__ __launch_bounds__(256) void emitter_clear_kernel(EmitterPool P) {
  const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
  if (slot < P.capacity) P.alive[slot] = 0;
}

}  // namespace

void launch_emitter_step(void* stream, const srt_pt* collide, const EmitterPool& P, float dt, float radius) {
  if (!P.capacity) return;
  emitter_step_kernel<<<dim3((P.capacity + 63u) / 64u), dim3(64), 0, (hipStream_t)stream>>>(device_scene(collide), P, dt, radius);
}

void launch_emitter_spawn(void* stream, const EmitterPool& P, const EmitterLaunch& L, uint32_t k, uint32_t born, const float* d_uniforms, uint64_t seed,
                          uint32_t key) {
  if (!P.capacity || !k) return;
  emitter_spawn_kernel<<<dim3((P.capacity + kSpawnBlock - 1u) / kSpawnBlock), dim3(kSpawnBlock), 0, (hipStream_t)stream>>>(P, L, k, born, d_uniforms, seed, key);
}

void launch_emitter_clear(void* stream, const EmitterPool& P) {
  if (!P.capacity) return;
  emitter_clear_kernel<<<dim3((P.capacity + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(P);
}

}  // namespace srt
