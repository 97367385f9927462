// TEST-ONLY stand-alone program for a sanitizer run of the traversal stacks at full depth: it reads scenes and rays written by
// tests/host_emu/stack_depth_sanitized.py (the deep_* fixtures of tests/_cases.py), builds each scene with the product's host
// builder and traces every ray through the nested walk (scene_hit: private arrays traverse<24> / traverse_records<48>), the
// flattened walk (flat_trace3: FlatFrame stack[kFlatStack]) and the counting walk of flat_host.cpp.  Built with
// -fsanitize=address,undefined a frame written past any of those arrays ends the run.  Links flat_host.cpp and csrc/pt_scene.cpp.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
void* emu_create();
void emu_destroy(void* h);
int emu_add_material(void* h, uint32_t type, const float* a, const float* b, float ior);
int emu_add_mesh(void* h, const float* pos, const float* nrm, uint32_t nv, const uint32_t* idx, uint32_t ni, const float* T, uint32_t material,
                 int is_light);
int emu_add_sphere(void* h, float radius, const float* T, uint32_t material);
int emu_commit(void* h, int use_bvh);
int emu_hit(void* h, const float* org, const float* dir, const float* bounds, size_t n, int slot, uint32_t* nested, uint32_t* flat);
int emu_hit_depth(void* h, const float* org, const float* dir, const float* bounds, size_t n, int32_t* deepest, uint32_t* flat,
                  uint32_t tree_depth[2]);
}

static bool take(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

// File: u32 nscenes; per scene: u32 nobjects, per object {u32 kind (0 mesh, 1 sphere), f32 T[16], sphere: f32 radius; mesh: u32 nv,
// f32 pos[3 nv], f32 nrm[3 nv], u32 ni, u32 idx[ni]}; u32 nrays, f32 org[3 n], f32 dir[3 n], f32 bounds[2 n]; u32 want[2] = the
// tree depths the fixture promises.
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s scenes.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  uint32_t nscenes = 0;
  if (!take(f, &nscenes, 4)) return 2;
  for (uint32_t s = 0; s < nscenes; s++) {
    void* h = emu_create();
    const float white[3] = {1, 1, 1}, black[3] = {0, 0, 0};
    emu_add_material(h, 0, white, black, 1.0f);
    uint32_t nobj = 0;
    if (!take(f, &nobj, 4)) return 2;
    for (uint32_t o = 0; o < nobj; o++) {
      uint32_t kind = 0; float T[16];
      if (!take(f, &kind, 4) || !take(f, T, sizeof T)) return 2;
      if (kind == 1) {
        float radius = 0;
        if (!take(f, &radius, 4)) return 2;
        emu_add_sphere(h, radius, T, 0);
      } else {
        uint32_t nv = 0, ni = 0;
        if (!take(f, &nv, 4)) return 2;
        std::vector<float> pos(3 * (size_t)nv), nrm(3 * (size_t)nv);
        if (!take(f, pos.data(), pos.size() * 4) || !take(f, nrm.data(), nrm.size() * 4) || !take(f, &ni, 4)) return 2;
        std::vector<uint32_t> idx(ni);
        if (!take(f, idx.data(), idx.size() * 4)) return 2;
        emu_add_mesh(h, pos.data(), nrm.data(), nv, idx.data(), ni, T, 0, 0);
      }
    }
    uint32_t n = 0, want[2];
    if (!take(f, &n, 4)) return 2;
    std::vector<float> org(3 * (size_t)n), dir(3 * (size_t)n), bounds(2 * (size_t)n);
    if (!take(f, org.data(), org.size() * 4) || !take(f, dir.data(), dir.size() * 4) || !take(f, bounds.data(), bounds.size() * 4) ||
        !take(f, want, sizeof want))
      return 2;
    if (emu_commit(h, 1) != 0) { fprintf(stderr, "scene %u: build_scene failed\n", s); return 1; }
    std::vector<uint32_t> nested(4 * (size_t)n), flat(4 * (size_t)n), counted(4 * (size_t)n);
    std::vector<int32_t> deepest(n);
    uint32_t tree[2];
    for (int slot = 0; slot < 3; slot++) emu_hit(h, org.data(), dir.data(), bounds.data(), n, slot, nested.data(), flat.data());
    emu_hit_depth(h, org.data(), dir.data(), bounds.data(), n, deepest.data(), counted.data(), tree);
    int32_t top = -1; uint32_t hits = 0;
    for (uint32_t i = 0; i < n; i++) { top = deepest[i] > top ? deepest[i] : top; hits += flat[4 * (size_t)i]; }
    const bool same = nested == flat && flat == counted;
    printf("scene %u: %u objects, %u rays, %u hits, max_tlas_depth %u, max_blas_depth %u, deepest frame index %d, walks agree: %s\n", s, nobj, n,
           hits, tree[0], tree[1], top, same ? "yes" : "NO");
    if (!same || tree[0] != want[0] || tree[1] != want[1] || top >= (int32_t)(tree[0] + tree[1])) return 1;
    emu_destroy(h);
  }
  fclose(f);
  printf("ok\n");
  return 0;
}
