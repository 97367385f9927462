// Per-lane work on the committed scene outside a render - explicit samples (srt_pt_trace_samples), closest hits (srt_pt_hit), the
// particle step - and the dumps of what a commit built (BVHs, area lights, the counters of the last srt_pt_trace_samples).  The
// kernels are the per-lane forms of pt_trace.h / pt_flat.h; the scene they read is pt.hip's device_scene().
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "pt_context.h"
#include "pt_device.h"
#include "srt_pt_debug.h"

#include "pt_trace.h"
#include "pt_flat.h"
#include "pt_particle.h"

namespace srt {

// Explicit (x, y, sample) triples; instrumented when COUNT.  NORMALS: the normal-colors view (normal_sample) instead of a path.
// ENVIMG: path_sample's build with Env_Map's image sampler (srt_pt_set_env_sampling).
template <bool COUNT, bool NORMALS = false, bool ENVIMG = false>
__global__ __launch_bounds__(64) void pt_samples_kernel(DScene S, uint64_t seed, const uint32_t* __restrict__ xs,
                                                        const uint32_t* __restrict__ ys, const uint32_t* __restrict__ ss,
                                                        uint32_t n, float* __restrict__ rgb, uint32_t* __restrict__ draws,
                                                        uint32_t* __restrict__ rays, unsigned long long* __restrict__ totals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Counters cnt;
  for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
  Rng rng;
  rng.key(seed, ys[i] * S.w + xs[i], ss[i]);
  const Spec p = NORMALS ? normal_sample<COUNT>(S, xs[i], ys[i], rng, cnt) : path_sample<COUNT, ENVIMG>(S, xs[i], ys[i], rng, cnt);
  rgb[3 * i] = p.r; rgb[3 * i + 1] = p.g; rgb[3 * i + 2] = p.b;
  if (draws) draws[i] = rng.draws;
  if (COUNT) {
    if (rays) rays[i] = cnt.v[C_RAYS];
    for (int k = 0; k < C_COUNT; k++) atomicAdd(&totals[k], (unsigned long long)cnt.v[k]);
  }
}

// FLAT: the query goes through flat_trace3 (pt_flat.h) in batch slot i % 3 instead of the nested scene_hit.
template <bool FLAT>
__global__ void pt_hit_kernel(DScene S, const float* __restrict__ org, const float* __restrict__ dir,
                              const float* __restrict__ bounds, uint32_t n, float* __restrict__ out9) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;                     // every lane stays in the kernel: flat_trace3 is a wave-wide loop
  const uint32_t j = live ? i : 0;
  Ray r;
  r.o = v3(org[3 * j], org[3 * j + 1], org[3 * j + 2]);
  r.d = v3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  r.b0 = bounds[2 * j]; r.b1 = bounds[2 * j + 1];
  Counters cnt;
  Hit h;
  if (FLAT) {
    const uint32_t slot = i % 3u;
    Hit res[3];
    flat_trace3(S, r.o, r.d, r.d, r.d, r.b0, r.b1, live && slot == 0, live && slot == 1, live && slot == 2, res[0], res[1], res[2]);
    h = slot == 0 ? res[0] : (slot == 1 ? res[1] : res[2]);
  } else {
    h = scene_hit<false>(S, r, cnt);
  }
  if (!live) return;
  float* o = out9 + 9 * i;
  for (int k = 0; k < 9; k++) o[k] = 0.0f;
  if (h.hit) {
    const Surface sf = surface_of(S, h, r);
    o[0] = 1.0f; o[1] = h.dist;
    o[2] = sf.position.x; o[3] = sf.position.y; o[4] = sf.position.z;
    o[5] = sf.normal.x; o[6] = sf.normal.y; o[7] = sf.normal.z;
    o[8] = (float)S.objects[h.obj].material;
  }
}

// Scene_Particles::Particle::update (pt_particle.h: particle_update), one lane per particle.
__global__ __launch_bounds__(64) void pt_particles_kernel(DScene S, float* __restrict__ pos, float* __restrict__ vel, float* __restrict__ age,
                                                          uint32_t n, float dt, float radius, uint8_t* __restrict__ alive) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  V3 p = v3(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
  V3 velocity = v3(vel[3 * k], vel[3 * k + 1], vel[3 * k + 2]);
  particle_update(S, p, velocity, dt, radius);
  const float a = age[k] - dt;
  age[k] = a;
  alive[k] = a > 0 ? 1 : 0;
  pos[3 * k] = p.x; pos[3 * k + 1] = p.y; pos[3 * k + 2] = p.z;
  vel[3 * k] = velocity.x; vel[3 * k + 1] = velocity.y; vel[3 * k + 2] = velocity.z;
}

}  // namespace srt

using namespace srt;

extern "C" {

int srt_pt_trace_samples(srt_pt* pt, uint64_t seed, const uint32_t* xs, const uint32_t* ys, const uint32_t* ss, size_t n,
                         float* rgb_out, uint32_t* draws_out, uint32_t* rays_out) {
  int st = need_ready(pt, "srt_pt_trace_samples");
  if (st != SRT_OK) return st;
  if ((st = settle(pt)) != SRT_OK) return st;
  if ((st = env_image_ready(pt, "srt_pt_trace_samples")) != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!xs || !ys || !ss || !rgb_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_trace_samples: NULL argument");
  if (n > 0x7fffffffull) return srt::fail(SRT_ERR_UNSUPPORTED, "too many samples in one call");
  for (size_t i = 0; i < n; i++)
    if (xs[i] >= pt->w || ys[i] >= pt->h) return srt::fail(SRT_ERR_INVALID, "sample %zu: pixel (%u,%u) outside %ux%u", i, xs[i], ys[i], pt->w, pt->h);
  DeviceBuffer<uint32_t> dx, dy, ds, dd, dr;
  DeviceBuffer<float> drgb;
  if ((st = dx.ensure(n)) || (st = dy.ensure(n)) || (st = ds.ensure(n)) || (st = dd.ensure(n)) || (st = dr.ensure(n)) || (st = drgb.ensure(3 * n))) return st;
  SRT_HIP(hipMemcpyAsync(dx, xs, n * 4, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(dy, ys, n * 4, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(ds, ss, n * 4, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemsetAsync(pt->d_totals, 0, C_COUNT * sizeof(unsigned long long), pt->stream));
  const auto kern = pt->normal_colors ? pt_samples_kernel<true, true>
                  : image_sampling_launch(pt) ? pt_samples_kernel<true, false, true> : pt_samples_kernel<true, false>;
  kern<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pt->stream>>>(device_scene(pt), seed, dx, dy, ds, (uint32_t)n, drgb, dd, dr, pt->d_totals);
  SRT_HIP(hipGetLastError());
  SRT_HIP(hipMemcpyAsync(rgb_out, drgb, n * 12, hipMemcpyDeviceToHost, pt->stream));
  if (draws_out) SRT_HIP(hipMemcpyAsync(draws_out, dd, n * 4, hipMemcpyDeviceToHost, pt->stream));
  if (rays_out) SRT_HIP(hipMemcpyAsync(rays_out, dr, n * 4, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipMemcpyAsync(pt->last_counters, pt->d_totals, sizeof pt->last_counters, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}

int srt_pt_hit(srt_pt* pt, const float* origins, const float* dirs, const float* bounds, size_t n, float* out9) {
  int st = need_device(pt, "srt_pt_hit");
  if (st != SRT_OK) return st;
  if ((st = need_committed(pt, "srt_pt_hit")) != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!origins || !dirs || !bounds || !out9) return srt::fail(SRT_ERR_INVALID, "srt_pt_hit: NULL argument");
  DeviceBuffer<float> dorg, ddir, db, dout;
  if ((st = dorg.ensure(3 * n)) || (st = ddir.ensure(3 * n)) || (st = db.ensure(2 * n)) || (st = dout.ensure(9 * n))) return st;
  SRT_HIP(hipMemcpyAsync(dorg, origins, n * 12, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(ddir, dirs, n * 12, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(db, bounds, n * 8, hipMemcpyHostToDevice, pt->stream));
  DScene S = device_scene(pt);
  if (pt->kernel_mode == 5) {
    if (!flat_walk_fits(pt->built.flat)) return srt::fail(SRT_ERR_UNSUPPORTED, "the flattened walk needs 1..31 objects");
    pt_hit_kernel<true><<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pt->stream>>>(S, dorg, ddir, db, (uint32_t)n, dout);
  } else {
    pt_hit_kernel<false><<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pt->stream>>>(S, dorg, ddir, db, (uint32_t)n, dout);
  }
  SRT_HIP(hipGetLastError());
  SRT_HIP(hipMemcpyAsync(out9, dout, n * 36, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}

int srt_pt_particles_step_device(srt_pt* pt, void* stream, float* d_pos, float* d_vel, float* d_age, size_t n, float dt, float radius,
                                 uint8_t* d_alive) {
  int st = need_device(pt, "srt_pt_particles_step_device");
  if (st != SRT_OK) return st;
  if (!pt->committed) return not_committed("srt_pt_particles_step");
  if (n == 0) return SRT_OK;
  if (!d_pos || !d_vel || !d_age || !d_alive) return srt::fail(SRT_ERR_INVALID, "srt_pt_particles_step: NULL argument");
  if (n > 0x7fffffffull) return srt::fail(SRT_ERR_UNSUPPORTED, "too many particles in one call");
  pt_particles_kernel<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream>>>(device_scene(pt), d_pos, d_vel, d_age, (uint32_t)n, dt,
                                                                                           radius, d_alive);
  SRT_HIP(hipGetLastError());
  return SRT_OK;
}

int srt_pt_particles_step(srt_pt* pt, float* pos, float* vel, float* age, size_t n, float dt, float radius, uint8_t* alive) {
  int st = need_device(pt, "srt_pt_particles_step");
  if (st != SRT_OK) return st;
  if ((st = settle(pt)) != SRT_OK) return st;
  if (n == 0) return SRT_OK;
  if (!pos || !vel || !age || !alive) return srt::fail(SRT_ERR_INVALID, "srt_pt_particles_step: NULL argument");
  DeviceBuffer<float> dp, dv, da;
  DeviceBuffer<uint8_t> dl;
  if ((st = dp.ensure(3 * n)) || (st = dv.ensure(3 * n)) || (st = da.ensure(n)) || (st = dl.ensure(n))) return st;
  SRT_HIP(hipMemcpyAsync(dp, pos, n * 12, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(dv, vel, n * 12, hipMemcpyHostToDevice, pt->stream));
  SRT_HIP(hipMemcpyAsync(da, age, n * 4, hipMemcpyHostToDevice, pt->stream));
  st = srt_pt_particles_step_device(pt, (void*)pt->stream, dp, dv, da, n, dt, radius, dl);
  if (st != SRT_OK) return st;
  SRT_HIP(hipMemcpyAsync(pos, dp, n * 12, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipMemcpyAsync(vel, dv, n * 12, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipMemcpyAsync(age, da, n * 4, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipMemcpyAsync(alive, dl, n, hipMemcpyDeviceToHost, pt->stream));
  SRT_HIP(hipStreamSynchronize(pt->stream));
  return SRT_OK;
}

long srt_pt_dump_bvh(srt_pt* pt, int which, float* boxes, uint32_t* links, size_t cap, uint32_t* order) {
  if (!pt || !boxes || !links) return srt::fail(SRT_ERR_INVALID, "srt_pt_dump_bvh: NULL argument");
  { const int ready = need_committed(pt, "srt_pt_dump_bvh"); if (ready != SRT_OK) return ready; }
  if (!pt->built.flat.use_bvh) return srt::fail(SRT_ERR_STATE, "scene was committed without BVHs");
  const HostBVH* b = &pt->built.tlas;
  const ObjectInput* in = nullptr;
  if (which >= 0) {
    if ((size_t)which >= pt->built.tlas.prim.size()) return srt::fail(SRT_ERR_INVALID, "object slot %d out of range", which);
    uint32_t obj = pt->built.tlas.prim[which];
    in = &pt->built.inputs[obj];
    if (in->kind != OBJ_MESH) return srt::fail(SRT_ERR_INVALID, "object slot %d is not a mesh", which);
    if (in->source >= 0) { obj = (uint32_t)in->source; in = &pt->built.inputs[obj]; }   // an instance: the shared arrays
    b = &pt->built.blas[obj];
  }
  for (size_t i = 0; i < b->nodes.size() && i < cap; i++) {
    const HostNode& nd = b->nodes[i];
    for (int a = 0; a < 3; a++) { boxes[6 * i + a] = nd.mn[a]; boxes[6 * i + 3 + a] = nd.mx[a]; }
    links[4 * i] = nd.start; links[4 * i + 1] = nd.size; links[4 * i + 2] = nd.l; links[4 * i + 3] = nd.r;
  }
  if (order)
    for (size_t i = 0; i < b->prim.size(); i++) order[i] = in ? in->mesh.idx[3 * b->prim[i]] : b->prim[i] + 1;
  return (long)b->nodes.size();
}

long srt_pt_dump_lights(srt_pt* pt, int from_device, uint32_t* heads, float* mats, size_t cap_lights, float* tris, size_t cap_tris) {
  if (!pt || (cap_lights && (!heads || !mats)) || (cap_tris && !tris)) return srt::fail(SRT_ERR_INVALID, "srt_pt_dump_lights: NULL argument");
  { const int ready = need_committed(pt, "srt_pt_dump_lights"); if (ready != SRT_OK) return ready; }
  if (from_device && pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "srt_pt_dump_lights: this context is host-only, there are no device arrays to read (from_device = 0 reads the host's)");
  const FlatScene& F = pt->built.flat;
  const size_t nl = F.lights.size(), nt = F.light_tris.size();
  std::vector<Light> lights(F.lights);
  std::vector<LightTri> ltris(F.light_tris);
  std::vector<Tri> tr(F.tris.begin() + F.light_tri_first, F.tris.end());
  std::vector<TriNrm> tn(F.tri_nrm.begin() + F.light_tri_first, F.tri_nrm.end());
  if (tr.size() != nt || tn.size() != nt) return srt::fail(SRT_ERR_STATE, "srt_pt_dump_lights: the light tables disagree about their triangle count");
  if (from_device) {
    SRT_HIP(hipSetDevice(pt->device));
    SRT_HIP(hipDeviceSynchronize());
    if (nl) SRT_HIP(hipMemcpy(lights.data(), pt->d_lights, nl * sizeof(Light), hipMemcpyDeviceToHost));
    if (nt) {
      SRT_HIP(hipMemcpy(ltris.data(), pt->d_ltris, nt * sizeof(LightTri), hipMemcpyDeviceToHost));
      SRT_HIP(hipMemcpy(tr.data(), pt->d_tris + F.light_tri_first, nt * sizeof(Tri), hipMemcpyDeviceToHost));
      SRT_HIP(hipMemcpy(tn.data(), pt->d_nrm + F.light_tri_first, nt * sizeof(TriNrm), hipMemcpyDeviceToHost));
    }
  }
  size_t li = 0;
  for (size_t i = 0; i < pt->built.inputs.size() && li < nl; i++) {
    if (light_of(pt->built, (uint32_t)i) < 0) continue;
    if (li < cap_lights) {
      const Light& L = lights[li];
      heads[4 * li] = L.has_trans; heads[4 * li + 1] = L.tri_base - F.light_tri_first; heads[4 * li + 2] = L.ntri; heads[4 * li + 3] = (uint32_t)i;
      std::memcpy(mats + 64 * li, &L.trans, 64 * sizeof(float));   // trans, itrans, pdfT, pdfiT
    }
    li++;
  }
  for (size_t t = 0; t < nt && t < cap_tris; t++) {
    float* o = tris + 31 * t;
    std::memcpy(o, &ltris[t], 13 * sizeof(float));                 // v0 v1 v2 (four floats each, padding included), area_term
    for (int a = 0; a < 3; a++) {
      o[13 + a] = tr[t].p0[a]; o[16 + a] = tr[t].e1[a]; o[19 + a] = tr[t].e2[a];
      o[22 + a] = tn[t].n0[a]; o[25 + a] = tn[t].n1[a]; o[28 + a] = tn[t].n2[a];
    }
  }
  return (long)nl;
}

int srt_pt_counters(srt_pt* pt, uint64_t out[8]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_counters: NULL argument");
  for (int k = 0; k < C_COUNT; k++) out[k] = pt->last_counters[k];
  return SRT_OK;
}

}  // extern "C"
