// Host module of the dynamic-light tests (tests/_light_cases.py builds it with g++): everything of update_host.cpp - which is
// included as text, with pt_scene.cpp inside it, so that its Upd handles, its upd_* entry points and its comparisons are this
// module's too - plus the switch, the refit of the scene layer, a comparison that looks at the light tables explicitly, the dump
// of the light tables in srt_pt_dump_lights' layout, and the device functions of pt_light_update.h against light_record /
// light_area_term / light_tri_record of pt_scene.cpp.
#include "update_host.cpp"

#include "pt_light_update.h"

namespace {

// light tables byte for byte, wherever the light range starts: records (tri_base relative to the first light triangle), LightTri
// records, and the light range of the three triangle arrays
bool same_lights(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (a.lights.size() != b.lights.size() || !same_bytes(a.light_tris, b.light_tris)) return false;
  const size_t na = a.tris.size() - a.light_tri_first, nb = b.tris.size() - b.light_tri_first;
  if (na != nb || na != a.light_tris.size()) return false;
  if (a.tri_nrm.size() != a.tris.size() || a.tri_packed.size() != 9 * a.tris.size() || b.tri_nrm.size() != b.tris.size() || b.tri_packed.size() != 9 * b.tris.size())
    return false;
  if (na && (std::memcmp(&a.tris[a.light_tri_first], &b.tris[b.light_tri_first], na * sizeof(Tri)) != 0 ||
             std::memcmp(&a.tri_nrm[a.light_tri_first], &b.tri_nrm[b.light_tri_first], na * sizeof(TriNrm)) != 0 ||
             std::memcmp(&a.tri_packed[9 * (size_t)a.light_tri_first], &b.tri_packed[9 * (size_t)b.light_tri_first], 9 * na * sizeof(float)) != 0))
    return false;
  for (size_t k = 0; k < a.lights.size(); k++) {
    Light x = a.lights[k], y = b.lights[k];
    x.tri_base -= a.light_tri_first;
    y.tri_base -= b.light_tri_first;
    if (std::memcmp(&x, &y, sizeof x) != 0) return false;
  }
  return true;
}

// bit equality, except that a NaN equals a NaN whatever its sign or payload
bool same_float(float a, float b) {
  if (a != a || b != b) return a != a && b != b;
  return std::memcmp(&a, &b, sizeof a) == 0;
}
bool same_floats(const float* a, const float* b, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!same_float(a[i], b[i])) return false;
  return true;
}

}  // namespace

extern "C" {

void lit_set_dynamic(void* h, int on) { ((Upd*)h)->built.dynamic_lights = on != 0; }
int lit_get_dynamic(void* h) { return ((Upd*)h)->built.dynamic_lights ? 1 : 0; }

// 0: applied; 1: a refused argument; 2: unsupported - as srt_pt_refit_mesh tells them apart
int lit_refit(void* h, uint32_t object, const float* pos, const float* nrm, uint32_t nverts) {
  Upd* u = (Upd*)h;
  MeshRefit R;
  bool bad = false;
  u->error = prepare_mesh_refit(u->built, object, pos, nrm, nverts, nullptr, &R, &bad);
  if (!u->error.empty()) return bad ? 1 : 2;
  if (R.top.max_tlas_depth > kTlasDepthLimit) { u->error = "BVH too deep"; return 2; }
  apply_mesh_refit(&u->built, &R);
  return 0;
}

int lit_same_computed(void* a, void* b) { return same_computed(((Upd*)a)->built, ((Upd*)b)->built) && same_lights(((Upd*)a)->built, ((Upd*)b)->built) ? 1 : 0; }
int lit_same_lights(void* a, void* b) { return same_lights(((Upd*)a)->built, ((Upd*)b)->built) ? 1 : 0; }
int lit_identical(void* a, void* b) {
  return identical(((Upd*)a)->built, ((Upd*)b)->built) && same_lights(((Upd*)a)->built, ((Upd*)b)->built) &&
                 ((Upd*)a)->built.dynamic_lights == ((Upd*)b)->built.dynamic_lights
             ? 1 : 0;
}
// refit keeps the tree where an update builds a new one: everything but the BVH<Triangle>s, which the caller compares by content
int lit_same_but_trees(void* a, void* b) {
  const BuiltScene &A = ((Upd*)a)->built, &B = ((Upd*)b)->built;
  const FlatScene &x = A.flat, &y = B.flat;
  if (!same_lights(A, B) || !same_tree(A.tlas, B.tlas) || !same_bytes(A.local_boxes, B.local_boxes) || !same_bytes(x.wave_tlas, y.wave_tlas)) return 0;
  if (x.objects.size() != y.objects.size() || A.inputs.size() != B.inputs.size()) return 0;
  for (size_t i = 0; i < A.inputs.size(); i++)
    if (std::memcmp(&A.inputs[i].trans, &B.inputs[i].trans, sizeof(Mat4)) != 0 || !same_bytes(A.inputs[i].mesh.pos, B.inputs[i].mesh.pos) ||
        !same_bytes(A.inputs[i].mesh.nrm, B.inputs[i].mesh.nrm))
      return 0;
  for (size_t k = 0; k < x.objects.size(); k++)
    if (x.objects[k].id != y.objects[k].id || std::memcmp(&x.objects[k].trans, &y.objects[k].trans, 2 * sizeof(Mat4)) != 0) return 0;
  return 1;
}

uint32_t lit_light_count(void* h) { return (uint32_t)((Upd*)h)->built.flat.lights.size(); }
uint32_t lit_light_tri_count(void* h) { return (uint32_t)((Upd*)h)->built.flat.light_tris.size(); }
// srt_pt_dump_lights' layout from the BuiltScene: heads 4 words, mats 64 floats per light; 31 floats per light triangle
void lit_dump(void* h, uint32_t* heads, float* mats, float* tris) {
  const BuiltScene& B = ((Upd*)h)->built;
  const FlatScene& F = B.flat;
  size_t li = 0;
  for (size_t i = 0; i < B.inputs.size(); i++) {
    if (light_of(B, (uint32_t)i) < 0) continue;
    const Light& L = F.lights[li];
    heads[4 * li] = L.has_trans; heads[4 * li + 1] = L.tri_base - F.light_tri_first; heads[4 * li + 2] = L.ntri; heads[4 * li + 3] = (uint32_t)i;
    std::memcpy(mats + 64 * li, &L.trans, 64 * sizeof(float));
    li++;
  }
  for (size_t t = 0; t < F.light_tris.size(); t++) {
    float* o = tris + 31 * t;
    std::memcpy(o, &F.light_tris[t], 13 * sizeof(float));
    const Tri& g = F.tris[F.light_tri_first + t];
    const TriNrm& n = F.tri_nrm[F.light_tri_first + t];
    for (int a = 0; a < 3; a++) { o[13 + a] = g.p0[a]; o[16 + a] = g.e1[a]; o[19 + a] = g.e2[a]; o[22 + a] = n.n0[a]; o[25 + a] = n.n1[a]; o[28 + a] = n.n2[a]; }
  }
}

// The device functions of pt_light_update.h, one "lane" after the other, against the functions of pt_scene.cpp: for each of the
// nmat matrices (16 floats, column-major) the Light record of that pose (itrans and has_trans as the Object ctor makes them) and,
// under its pdfT, the area term and the whole LightTri of every triangle of the mesh (pos, idx).  Returns the number of
// (matrix, item) pairs that differ in any bit - a NaN equals a NaN; out[0..3] count the area terms that are inf, NaN, and the
// matrices with has_trans 0 / 1.
long lit_emu_mismatches(const float* mats, uint32_t nmat, const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t ntri, uint32_t out[4]) {
  MeshInput m;
  m.pos.assign(pos, pos + 3 * (size_t)nverts);
  m.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  m.idx.assign(idx, idx + 3 * (size_t)ntri);
  long bad = 0;
  out[0] = out[1] = out[2] = out[3] = 0;
  for (uint32_t k = 0; k < nmat; k++) {
    const Mat4 T = mat_from(mats + 16 * (size_t)k);
    const Mat4 iT = mat_inverse(T);
    const bool ht = mat_ne_identity(T);
    out[ht ? 3 : 2]++;
    Light want;
    std::memset(&want, 0, sizeof want);
    light_record(T, iT, ht, &want);
    float pdfT[16], pdfiT[16];
    std::memset(pdfT, 0xff, sizeof pdfT);
    std::memset(pdfiT, 0xff, sizeof pdfiT);
    light_matrices(&T.c[0][0], &iT.c[0][0], ht ? 1u : 0u, pdfT, pdfiT);
    if (!same_floats(pdfT, &want.pdfT.c[0][0], 16) || !same_floats(pdfiT, &want.pdfiT.c[0][0], 16)) bad++;
    for (uint32_t t = 0; t < ntri; t++) {
      const LightTri w = light_tri_record(want.pdfT, m, t);
      LightTri g;
      std::memset(&g, 0xff, sizeof g);
      light_triangle(pos, idx, t, &want.pdfT.c[0][0], &g);
      const float area = light_area(&want.pdfT.c[0][0], w.v0, w.v1, w.v2);
      if (!same_floats(&g.v0[0], &w.v0[0], sizeof(LightTri) / sizeof(float)) || !same_float(area, w.area_term)) bad++;
      if (std::isinf(w.area_term)) out[0]++;
      if (w.area_term != w.area_term) out[1]++;
    }
  }
  return bad;
}

}  // extern "C"
