// The host emulation of the traversal headers with srt_pt_set_active in between (repose_refit_flat_host.cpp plus the calls below):
// check_active_list / apply_set_active on the built scene - the definition srt_pt_set_active[_device] is held to - then the device
// headers' nested walk, flattened walk and per-sample path over the masked arrays, one lane at a time.  A scene with hidden objects
// keeps the tree of the commit, so this, not the oracle, says what it computes; tests/test_pt_active_host.py compares it with the
// oracle on a fresh commit without the hidden objects where the two must agree (closest hits), tests/test_pt_active_gpu.py takes it
// as the expectation for the GPU.
#include "repose_refit_flat_host.cpp"

extern "C" {

// 0 applied (or nothing to change), 1 refused argument, 2 unsupported scene
int emu_set_active(void* h, const uint32_t* objects, const uint8_t* active, uint32_t n) {
  Emu* e = (Emu*)h;
  bool unsupported = false;
  if (!check_active_list(e->built, objects, n, &unsupported).empty()) return unsupported ? 2 : 1;
  apply_set_active(&e->built, objects, active, n);
  bind_scene(e);
  return 0;
}

// srt_pt_get_active of the emulated scene; returns the object count
long emu_get_active(void* h, uint8_t* out, size_t cap) {
  Emu* e = (Emu*)h;
  for (size_t i = 0; i < e->built.active.size() && i < cap; i++) out[i] = e->built.active[i];
  return (long)e->built.active.size();
}

}  // extern "C"
