// The host emulation of the traversal headers with host top-level refits in between (refit_flat_host.cpp plus one call):
// prepare_top_refit / apply_top_refit on the built scene - the definition srt_pt_repose_refit[_device] is held to - then the
// device headers' nested walk, flattened walk and per-sample path over the refitted arrays, one lane at a time.  A refitted
// BVH<Object> is not the tree a fresh commit of the new poses builds, so this, not the oracle, says what a refitted scene
// computes; tests/test_pt_repose_refit_host.py compares it with the oracle where the two must agree (closest hits),
// tests/test_pt_repose_refit_gpu.py takes it as the expectation for the GPU.
#include "refit_flat_host.cpp"

extern "C" {

// 0 applied, 1 refused list
int emu_repose_refit(void* h, const uint32_t* objects, const float* trans, uint32_t n) {
  Emu* e = (Emu*)h;
  std::vector<Mat4> T(n);
  if (n) std::memcpy(T.data(), trans, (size_t)n * sizeof(Mat4));
  TopRefit R;
  if (!prepare_top_refit(e->built, objects, T.data(), n, &R).empty()) return 1;
  apply_top_refit(&e->built, &R);
  bind_scene(e);
  return 0;
}

// srt_pt_repose on the emulated scene (a rebuild of the BVH<Object>): 0 applied, 1 refused
int emu_repose(void* h, const uint32_t* objects, const float* trans, uint32_t n) {
  Emu* e = (Emu*)h;
  std::vector<Mat4> T(n);
  if (n) std::memcpy(T.data(), trans, (size_t)n * sizeof(Mat4));
  ReposedTop top;
  bool bad = false;
  if (!prepare_repose(e->built, objects, T.data(), n, &top, &bad).empty()) return 1;
  apply_repose(&e->built, &top);
  bind_scene(e);
  return 0;
}

// srt_pt_dump_bvh(-1) of the emulated scene: boxes (6 per node), links (4 per node), order (1-based ids); returns the node count
long emu_dump_top(void* h, float* boxes, uint32_t* links, size_t cap, uint32_t* order) {
  Emu* e = (Emu*)h;
  const HostBVH& b = e->built.tlas;
  for (size_t i = 0; i < b.nodes.size() && i < cap; i++) {
    const HostNode& nd = b.nodes[i];
    for (int a = 0; a < 3; a++) { boxes[6 * i + a] = nd.mn[a]; boxes[6 * i + 3 + a] = nd.mx[a]; }
    links[4 * i] = nd.start; links[4 * i + 1] = nd.size; links[4 * i + 2] = nd.l; links[4 * i + 3] = nd.r;
  }
  for (size_t i = 0; i < b.prim.size(); i++) order[i] = b.prim[i] + 1;
  return (long)b.nodes.size();
}

double emu_top_cost(void* h) { return tree_cost(((Emu*)h)->built.tlas); }

}  // extern "C"
