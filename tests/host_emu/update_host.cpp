// Host module of the mesh-update tests (tests/_update_cases.py builds it with g++): the scene layer's prepare_mesh_update /
// apply_mesh_update and prepare_repose / apply_repose over a BuiltScene, comparisons of two BuiltScenes, and the per-triangle
// device functions of pt_mesh_update.h against triangle_box / append_triangles.  pt_scene.cpp is included as text so that the
// functions of its unnamed namespace can be called.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "pt_scene.cpp"

#include "pt_mesh_update.h"

using namespace srt;

namespace {

constexpr uint32_t kTlasDepthLimit = 24, kBlasDepthLimit = 48;   // kMaxTlasDepth / kMaxBlasDepth of pt_trace.h

struct Upd {
  std::vector<ObjectInput> inputs;
  std::vector<Material> materials;
  BuiltScene built;
  std::string error;
};

Mat4 mat_from(const float* T) {
  Mat4 m;
  std::memcpy(&m, T, sizeof m);
  return m;
}

template <class V>
bool same_bytes(const V& a, const V& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

bool same_tree(const HostBVH& a, const HostBVH& b) { return same_bytes(a.nodes, b.nodes) && a.prim == b.prim; }

// Everything the kernels compute from, wherever a mesh's ranges are stored.
bool same_computed(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (a.use_bvh != b.use_bvh || a.tlas_nodes != b.tlas_nodes || a.max_tlas_depth != b.max_tlas_depth || a.max_blas_depth != b.max_blas_depth) return false;
  if (!same_tree(A.tlas, B.tlas) || A.blas.size() != B.blas.size() || !same_bytes(A.local_boxes, B.local_boxes)) return false;
  for (size_t i = 0; i < A.blas.size(); i++)
    if (!same_tree(A.blas[i], B.blas[i])) return false;
  if (a.tlas_nodes && std::memcmp(a.nodes.data(), b.nodes.data(), a.tlas_nodes * sizeof(Node)) != 0) return false;
  if (!same_bytes(a.wave_tlas, b.wave_tlas) || a.wave_lazy != b.wave_lazy || a.lazy_objects != b.lazy_objects) return false;
  if (!same_bytes(a.materials, b.materials) || !same_bytes(a.light_tris, b.light_tris) || a.lights.size() != b.lights.size()) return false;
  if (a.nodes.size() != b.nodes.size() || a.blas_recs.size() != b.blas_recs.size() || a.tris.size() != b.tris.size() ||
      a.tri_nrm.size() != b.tri_nrm.size() || a.tri_packed.size() != b.tri_packed.size() || a.objects.size() != b.objects.size())
    return false;
  auto same_run = [&](uint32_t ta, uint32_t tb, uint32_t n) {
    return std::memcmp(&a.tris[ta], &b.tris[tb], n * sizeof(Tri)) == 0 && std::memcmp(&a.tri_nrm[ta], &b.tri_nrm[tb], n * sizeof(TriNrm)) == 0 &&
           std::memcmp(&a.tri_packed[9 * (size_t)ta], &b.tri_packed[9 * (size_t)tb], 9 * (size_t)n * sizeof(float)) == 0;
  };
  for (size_t k = 0; k < a.lights.size(); k++) {
    Light x = a.lights[k], y = b.lights[k];
    if (x.ntri != y.ntri || x.tri_base - a.light_tri_first != y.tri_base - b.light_tri_first || !same_run(x.tri_base, y.tri_base, x.ntri)) return false;
    x.tri_base = y.tri_base = 0;
    if (std::memcmp(&x, &y, sizeof x) != 0) return false;
  }
  for (size_t k = 0; k < a.objects.size(); k++) {
    Object x = a.objects[k], y = b.objects[k];
    if (x.ntri != y.ntri || x.nnodes != y.nnodes || x.nrec != y.nrec) return false;
    if (x.ntri && !same_run(x.tri_base, y.tri_base, x.ntri)) return false;
    if (x.nrec && std::memcmp(&a.blas_recs[x.rec_base], &b.blas_recs[y.rec_base], x.nrec * sizeof(WaveInterior)) != 0) return false;
    if (x.nnodes && std::memcmp(&a.nodes[x.node_base], &b.nodes[y.node_base], x.nnodes * sizeof(Node)) != 0) return false;
    x.tri_base = y.tri_base = x.node_base = y.node_base = x.rec_base = y.rec_base = 0;   // the ranges may lie elsewhere
    if (std::memcmp(&x, &y, sizeof x) != 0) return false;
  }
  // and the inputs a later commit or update starts from
  if (A.inputs.size() != B.inputs.size()) return false;
  for (size_t i = 0; i < A.inputs.size(); i++) {
    const ObjectInput &x = A.inputs[i], &y = B.inputs[i];
    if (x.kind != y.kind || x.source != y.source || x.material != y.material || x.is_light != y.is_light || std::memcmp(&x.trans, &y.trans, sizeof(Mat4)) != 0 ||
        !same_bytes(x.mesh.pos, y.mesh.pos) || !same_bytes(x.mesh.nrm, y.mesh.nrm) || x.mesh.idx != y.mesh.idx)
      return false;
  }
  return true;
}

// Byte for byte, storage included.
bool identical(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  return same_computed(A, B) && same_bytes(a.nodes, b.nodes) && same_bytes(a.tris, b.tris) && same_bytes(a.tri_nrm, b.tri_nrm) &&
         same_bytes(a.tri_packed, b.tri_packed) && same_bytes(a.objects, b.objects) && same_bytes(a.lights, b.lights) &&
         same_bytes(a.blas_recs, b.blas_recs) && same_bytes(A.store, B.store) && a.light_tri_first == b.light_tri_first;
}

}  // namespace

extern "C" {

void* upd_create() { return new Upd(); }
void upd_destroy(void* h) { delete (Upd*)h; }
void* upd_clone(void* h) { return new Upd(*(Upd*)h); }
const char* upd_error(void* h) { return ((Upd*)h)->error.c_str(); }

int upd_add_material(void* h, uint32_t type, const float* a, const float* b, float ior) {
  Material m;
  m.type = type; m.ior = ior;
  for (int i = 0; i < 3; i++) { m.a[i] = a[i]; m.b[i] = b[i]; }
  ((Upd*)h)->materials.push_back(m);
  return (int)((Upd*)h)->materials.size() - 1;
}

int upd_add_mesh(void* h, const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const float* T, uint32_t material, int is_light) {
  ObjectInput o;
  o.kind = OBJ_MESH; o.trans = mat_from(T); o.material = material; o.is_light = is_light != 0;
  o.mesh.pos.assign(pos, pos + 3 * (size_t)nverts);
  o.mesh.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  o.mesh.idx.assign(idx, idx + nidx);
  ((Upd*)h)->inputs.push_back(o);
  return 0;
}

int upd_add_sphere(void* h, float radius, const float* T, uint32_t material) {
  ObjectInput o;
  o.kind = OBJ_SPHERE; o.trans = mat_from(T); o.material = material; o.radius = radius;
  ((Upd*)h)->inputs.push_back(o);
  return 0;
}

int upd_add_sphere_light(void* h, float radius, const float* T, uint32_t material, const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t nidx) {
  ObjectInput o;
  o.kind = OBJ_SPHERE; o.trans = mat_from(T); o.material = material; o.radius = radius; o.is_light = true;
  o.mesh.pos.assign(pos, pos + 3 * (size_t)nverts);
  o.mesh.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  o.mesh.idx.assign(idx, idx + nidx);
  ((Upd*)h)->inputs.push_back(o);
  return 0;
}

int upd_add_instance(void* h, uint32_t source, const float* T, uint32_t material) {
  ObjectInput o;
  o.kind = OBJ_MESH; o.trans = mat_from(T); o.material = material; o.source = (int32_t)source;
  ((Upd*)h)->inputs.push_back(o);
  return 0;
}

int upd_commit(void* h, int use_bvh) {
  Upd* u = (Upd*)h;
  u->error = build_scene(u->inputs, u->materials, use_bvh != 0, &u->built);
  return u->error.empty() ? 0 : 2;
}

// 0: applied; 1: a refused argument; 2: a build that does not terminate or a tree too deep - as srt_pt_update_mesh tells them apart
int upd_update(void* h, uint32_t object, const float* pos, const float* nrm, uint32_t nverts) {
  Upd* u = (Upd*)h;
  MeshUpdate U;
  bool bad = false;
  u->error = prepare_mesh_update(u->built, object, pos, nrm, nverts, nullptr, &U, &bad);
  if (!u->error.empty()) return bad ? 1 : 2;
  if (U.top.max_tlas_depth > kTlasDepthLimit || U.max_blas_depth > kBlasDepthLimit) { u->error = "BVH too deep"; return 2; }
  apply_mesh_update(&u->built, &U);
  return 0;
}

int upd_repose(void* h, const uint32_t* objects, const float* T, uint32_t n) {
  Upd* u = (Upd*)h;
  std::vector<Mat4> t(n);
  if (n) std::memcpy(t.data(), T, (size_t)n * sizeof(Mat4));
  ReposedTop top;
  bool bad = false;
  u->error = prepare_repose(u->built, objects, t.data(), n, &top, &bad);
  if (!u->error.empty()) return bad ? 1 : 2;
  apply_repose(&u->built, &top);
  return 0;
}

int upd_same_computed(void* a, void* b) { return same_computed(((Upd*)a)->built, ((Upd*)b)->built) ? 1 : 0; }
int upd_identical(void* a, void* b) { return identical(((Upd*)a)->built, ((Upd*)b)->built) ? 1 : 0; }

// {BVH<Triangle> nodes, interior records, node offset, record base} of an object's storage; {max_tlas_depth, max_blas_depth}
void upd_store(void* h, uint32_t object, uint32_t out[4]) {
  const MeshStore& m = ((Upd*)h)->built.store[object];
  out[0] = m.nnodes; out[1] = m.nrec; out[2] = m.node_off; out[3] = m.rec_base;
}
void upd_depths(void* h, uint32_t out[2]) {
  out[0] = ((Upd*)h)->built.flat.max_tlas_depth; out[1] = ((Upd*)h)->built.flat.max_blas_depth;
}
void upd_local_box(void* h, uint32_t object, float out[6]) { std::memcpy(out, &((Upd*)h)->built.local_boxes[6 * (size_t)object], 6 * sizeof(float)); }

// The device functions of pt_mesh_update.h, one "lane" after the other, against triangle_box and append_triangles over the same
// mesh in `order` (index order when NULL).  Returns the number of triangles whose box or records differ in any bit;
// signed_zero_bounds counts the box bounds that are +0 / -0.
long upd_emu_mismatches(const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t ntri, const uint32_t* order, uint32_t signed_zero_bounds[2]) {
  MeshInput m;
  m.pos.assign(pos, pos + 3 * (size_t)nverts);
  m.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  m.idx.assign(idx, idx + 3 * (size_t)ntri);
  std::vector<uint32_t> ord;
  if (order) ord.assign(order, order + ntri);
  std::vector<Tri> tris;
  std::vector<TriNrm> tn;
  std::vector<float> packed;
  append_triangles(m, order ? &ord : nullptr, &tris, &tn, &packed);
  long bad = 0;
  signed_zero_bounds[0] = signed_zero_bounds[1] = 0;
  for (uint32_t k = 0; k < ntri; k++) {
    const uint32_t t = order ? order[k] : k;
    const Box want = triangle_box(&m.pos[3 * m.idx[3 * t]], &m.pos[3 * m.idx[3 * t + 1]], &m.pos[3 * m.idx[3 * t + 2]]);
    float got[6];
    mesh_triangle_box(pos, idx, t, got);
    Tri g;
    TriNrm nn;
    std::memset(&g, 0xff, sizeof g);
    std::memset(&nn, 0xff, sizeof nn);
    mesh_triangle_record(pos, nrm, idx, t, &g, &nn);
    const float p9[9] = {g.p0[0], g.p0[1], g.p0[2], g.e1[0], g.e1[1], g.e1[2], g.e2[0], g.e2[1], g.e2[2]};
    if (std::memcmp(got, &want, sizeof got) != 0 || std::memcmp(&g, &tris[k], sizeof g) != 0 || std::memcmp(&nn, &tn[k], sizeof nn) != 0 ||
        std::memcmp(p9, &packed[9 * (size_t)k], sizeof p9) != 0)
      bad++;
    for (int a = 0; a < 6; a++)
      if (got[a] == 0.0f) signed_zero_bounds[std::signbit(got[a]) ? 1 : 0]++;
  }
  return bad;
}

}  // extern "C"
