// The host emulation of the traversal headers with host in-place refits in between (repose_refit_flat_host.cpp plus one call):
// prepare_mesh_refit_inplace / apply_mesh_refit_inplace on the built scene - the definition srt_pt_refit_mesh_inplace[_device] is
// held to: new vertices for one mesh with BOTH trees kept - then the device headers' nested walk, flattened walk and per-sample path
// over the refitted arrays, one lane at a time.  Neither tree is the one a fresh commit of the new vertices builds, so this, not
// the oracle, says what such a scene computes; tests/test_pt_refit_inplace_host.py compares it with the oracle where the two must
// agree (closest hits), tests/test_pt_refit_inplace_gpu.py takes it as the expectation for the GPU.
#include "repose_refit_flat_host.cpp"

extern "C" {

// 0 applied, 1 refused argument
int emu_refit_inplace(void* h, uint32_t object, const float* pos, const float* nrm, uint32_t nverts) {
  Emu* e = (Emu*)h;
  MeshRefit R;
  if (!prepare_mesh_refit_inplace(e->built, object, pos, nrm, nverts, nullptr, true, &R).empty()) return 1;
  apply_mesh_refit_inplace(&e->built, &R);
  bind_scene(e);
  return 0;
}

// srt_pt_set_active on the emulated scene: 0 applied, 1 refused list
int emu_set_active(void* h, const uint32_t* objects, const uint8_t* active, uint32_t n) {
  Emu* e = (Emu*)h;
  bool unsupported = false;
  if (!check_active_list(e->built, objects, n, &unsupported).empty()) return 1;
  apply_set_active(&e->built, objects, active, n);
  bind_scene(e);
  return 0;
}

}  // extern "C"
