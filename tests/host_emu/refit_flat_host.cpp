// The host emulation of the traversal headers (instances_flat_host.cpp) with a host refit in between: prepare_mesh_refit /
// apply_mesh_refit on the built scene, then the device headers' nested walk, flattened walk and per-sample path over the
// refitted arrays, one lane at a time.  tests/test_pt_refit_emu_host.py compares the result with the oracle on the description
// with the new vertices (whose build yields another tree); tests/test_pt_refit_gpu.py takes it as the expectation for the GPU.
#include "instances_flat_host.cpp"

#include <cstring>

// The emulated context with what path_sample reads beyond the flattened scene: the delta lights (srt_pt_add_light).
struct RefitEmu : Emu {
  std::vector<DeltaLight> delta;
};

static void bind_scene(Emu* e) {
  const FlatScene& F = e->built.flat;
  DScene& S = e->S;
  S.nodes = F.nodes.data(); S.tris = F.tris.data(); S.tri_nrm = F.tri_nrm.data(); S.objects = F.objects.data();
  S.wave_tlas = F.wave_tlas.data(); S.blas_recs = F.blas_recs.data(); S.wave_lazy = F.wave_lazy.data();
  S.wave_q = (uint32_t)F.wave_tlas.size();
  S.nobjects = (uint32_t)F.objects.size(); S.tlas_nodes = F.tlas_nodes;
}

extern "C" {

void* emu_refit_create() { return static_cast<Emu*>(new RefitEmu()); }
void emu_refit_destroy(void* h) { delete static_cast<RefitEmu*>((Emu*)h); }

// srt_pt_add_light / srt_pt_set_env_light, after emu_commit
void emu_add_light(void* h, uint32_t type, const float* radiance, const float* angle_bounds, const float* T) {
  RefitEmu* e = static_cast<RefitEmu*>((Emu*)h);
  Mat4 m;
  std::memcpy(&m, T, sizeof m);
  e->delta.push_back(make_delta_light(type, radiance, angle_bounds, m));
  e->S.delta_lights = e->delta.data(); e->S.ndelta = (uint32_t)e->delta.size();
}
void emu_set_env(void* h, uint32_t type, const float* radiance) {
  Emu* e = (Emu*)h;
  e->S.env_type = type;
  for (int i = 0; i < 3; i++) e->S.env_radiance[i] = radiance[i];
}

// 0 applied, 1 refused argument, 2 unsupported
int emu_refit(void* h, uint32_t object, const float* pos, const float* nrm, uint32_t nverts) {
  Emu* e = (Emu*)h;
  MeshRefit R;
  bool bad = false;
  const std::string err = prepare_mesh_refit(e->built, object, pos, nrm, nverts, nullptr, &R, &bad);
  if (!err.empty()) return bad ? 1 : 2;
  apply_mesh_refit(&e->built, &R);
  bind_scene(e);
  return 0;
}

void emu_set_camera(void* h, const float* iview, float vfov, float ar, uint32_t w, uint32_t ht, uint32_t max_depth) {
  Emu* e = (Emu*)h;
  e->S.cam = make_camera(iview, vfov, ar);
  e->S.w = w; e->S.h = ht; e->S.max_depth = max_depth;
}

// pt_samples_kernel (pt_query.hip) for n (x, y, sample) triples: radiance, RNG draws and rays of each; normals != 0: the
// normal-colors view's first-hit sample instead.
void emu_trace_samples(void* h, uint64_t seed, const uint32_t* xs, const uint32_t* ys, const uint32_t* ss, size_t n, int normals, float* rgb,
                       uint32_t* draws, uint32_t* rays) {
  Emu* e = (Emu*)h;
  const DScene& S = e->S;
  for (size_t i = 0; i < n; i++) {
    Counters cnt;
    for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
    Rng rng;
    rng.key(seed, ys[i] * S.w + xs[i], ss[i]);
    const Spec p = normals ? normal_sample<true>(S, xs[i], ys[i], rng, cnt) : path_sample<true>(S, xs[i], ys[i], rng, cnt);
    rgb[3 * i] = p.r; rgb[3 * i + 1] = p.g; rgb[3 * i + 2] = p.b;
    draws[i] = rng.draws;
    rays[i] = cnt.v[C_RAYS];
  }
}

// pt_hit_kernel (pt_query.hip) for n rays: the nine floats of srt_pt_hit {hit, dist, position, normal, material}, from the nested walk
// and from the flattened walk (ray i in batch slot i % 3, as the kernel places it).
void emu_hit9(void* h, const float* org, const float* dir, const float* bounds, size_t n, float* nested9, float* flat9) {
  Emu* e = (Emu*)h;
  const DScene& S = e->S;
  for (size_t i = 0; i < n; i++) {
    Ray r; r.o = v3p(org + 3 * i); r.d = v3p(dir + 3 * i); r.b0 = bounds[2 * i]; r.b1 = bounds[2 * i + 1];
    Counters cnt;
    for (int k = 0; k < C_COUNT; k++) cnt.v[k] = 0;
    const uint32_t slot = (uint32_t)(i % 3u);
    Hit res[3];
    flat_trace3(S, r.o, r.d, r.d, r.d, r.b0, r.b1, slot == 0, slot == 1, slot == 2, res[0], res[1], res[2]);
    const Hit both[2] = {scene_hit<false>(S, r, cnt), res[slot]};
    for (int f = 0; f < 2; f++) {
      float* o = (f ? flat9 : nested9) + 9 * i;
      for (int k = 0; k < 9; k++) o[k] = 0.0f;
      if (!both[f].hit) continue;
      const Surface sf = surface_of(S, both[f], r);
      o[0] = 1.0f; o[1] = both[f].dist;
      o[2] = sf.position.x; o[3] = sf.position.y; o[4] = sf.position.z;
      o[5] = sf.normal.x; o[6] = sf.normal.y; o[7] = sf.normal.z;
      o[8] = (float)S.objects[both[f].obj].material;
    }
  }
}

}  // extern "C"
