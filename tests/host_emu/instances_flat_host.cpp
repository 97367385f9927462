// The host emulation of the traversal headers (flat_host.cpp) with one more feeding call: an instance of a mesh added before.
// tests/test_pt_instances_emu_host.py walks scenes with shared triangle / BVH<Triangle> ranges through scene_hit and flat_trace3.
#include "flat_host.cpp"

extern "C" int emu_add_instance(void* h, uint32_t source, const float* T, uint32_t material) {
  Emu* e = (Emu*)h;
  ObjectInput o; o.kind = OBJ_MESH; o.material = material; o.source = (int32_t)source;
  for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) o.trans.c[c][r] = T[4 * c + r];
  e->inputs.push_back(o);
  return 0;
}
