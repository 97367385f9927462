// Stand-alone check of srt_pt_refit_mesh_inplace's scene layer (pt_scene.cpp alone; tests/test_pt_refit_inplace_host.py builds it
// with -fsanitize=address,undefined and runs it once): two meshes, instances, a light and a sphere.  Identity, refits of both
// meshes with both trees kept, the identity with srt_pt_refit_mesh + srt_pt_repose_refit, inactive objects, supplied node boxes,
// non-finite vertices taken and refused, every refusal; after every refit the links, orders, counts and tables of object order of
// both trees are the committed ones and every box of the BVH<Object> is the fold it is defined as.
#include <limits>

#include "scene_main_common.h"

static bool inplace(BuiltScene* S, uint32_t object, const MeshInput& m, const float* boxes = nullptr, bool refuse = true) {
  MeshRefit R;
  if (!prepare_mesh_refit_inplace(*S, object, m.pos.data(), m.nrm.data(), (uint32_t)m.pos.size() / 3, boxes, refuse, &R).empty()) return false;
  EXPECT(R.top.objects.empty() && R.top.tlas.nodes.empty());
  apply_mesh_refit_inplace(S, &R);
  return true;
}

// What stays of the BVH<Object> and the tables of object order, and every box of it against the definition.
static void check_top(const BuiltScene& S, const BuiltScene& was) {
  const FlatScene &F = S.flat, &G = was.flat;
  EXPECT(S.tlas.prim == was.tlas.prim && S.tlas.nodes.size() == was.tlas.nodes.size() && F.tlas_nodes == G.tlas_nodes);
  EXPECT(F.wave_lazy == G.wave_lazy && F.lazy_objects == G.lazy_objects && F.max_tlas_depth == G.max_tlas_depth && F.max_blas_depth == G.max_blas_depth);
  EXPECT(F.nodes.size() == G.nodes.size() && F.wave_tlas.size() == G.wave_tlas.size() && F.objects.size() == G.objects.size());
  EXPECT(same_bytes(F.objects, G.objects));                 // no record holds a box: not one byte of them changes
  std::vector<float> posed, boxes;
  posed_boxes(S, &posed);
  effective_boxes(S, &posed);
  top_refit_boxes(S.tlas, posed.data(), &boxes);
  size_t q = 0;
  for (size_t n = 0; n < S.tlas.nodes.size(); n++) {
    const HostNode &h = S.tlas.nodes[n], &w = was.tlas.nodes[n];
    EXPECT(h.start == w.start && h.size == w.size && h.l == w.l && h.r == w.r);
    EXPECT(std::memcmp(h.mn, &boxes[6 * n], 12) == 0 && std::memcmp(h.mx, &boxes[6 * n + 3], 12) == 0);
    EXPECT(std::memcmp(F.nodes[n].mn, h.mn, 12) == 0 && std::memcmp(F.nodes[n].mx, h.mx, 12) == 0 && F.nodes[n].left == G.nodes[n].left);
    if (h.l == h.r) continue;
    const WaveInterior &wi = F.wave_tlas[q], &wo = G.wave_tlas[q];
    q++;
    EXPECT(std::memcmp(wi.boxl, &boxes[6 * (size_t)h.l], 24) == 0 && std::memcmp(wi.boxr, &boxes[6 * (size_t)h.r], 24) == 0);
    EXPECT(wi.l_ref == wo.l_ref && wi.r_ref == wo.r_ref);
  }
}

int main() {
  const std::vector<Material> mats = two_materials();
  const MeshInput A0 = sheet(7, 0.05f, 1.0f), A1 = sheet(7, 0.6f, 2.5f), B0 = sheet(5, 0.1f, 1.5f), B1 = sheet(5, 0.9f, 0.5f);

  BuiltScene S, first;
  bool bad = false;
  EXPECT(build_scene(scene(A0, B0), mats, true, &S).empty());
  first = S;
  // identity: the committed vertices give the committed scene back (as values: compare the boxes with ==)
  EXPECT(inplace(&S, 1, A0));
  check_top(S, first);
  for (size_t n = 0; n < S.tlas.nodes.size(); n++)
    for (int a = 0; a < 3; a++) EXPECT(S.tlas.nodes[n].mn[a] == first.tlas.nodes[n].mn[a] && S.tlas.nodes[n].mx[a] == first.tlas.nodes[n].mx[a]);
  // both meshes in turn; the mesh's half is srt_pt_refit_mesh's, the top half srt_pt_repose_refit's of the family
  for (int round = 0; round < 2; round++) {
    const uint32_t object = round ? 2u : 1u;
    const MeshInput& m = round ? B1 : A1;
    BuiltScene viaRefit = S;
    EXPECT(inplace(&S, object, m));
    check_top(S, first);
    MeshRefit R;
    EXPECT(prepare_mesh_refit(viaRefit, object, m.pos.data(), m.nrm.data(), (uint32_t)m.pos.size() / 3, nullptr, &R, &bad).empty());
    apply_mesh_refit(&viaRefit, &R);
    EXPECT(same_bytes(S.blas[object].nodes, viaRefit.blas[object].nodes) && same_bytes(S.flat.tris, viaRefit.flat.tris) &&
           same_bytes(S.flat.tri_nrm, viaRefit.flat.tri_nrm) && S.flat.tri_packed == viaRefit.flat.tri_packed && same_bytes(S.flat.blas_recs, viaRefit.flat.blas_recs) &&
           S.local_boxes == viaRefit.local_boxes);
    // .. and a rebuild of the BVH<Object> on top of the in-place refit is the rebuild srt_pt_refit_mesh made
    std::vector<uint32_t> family;
    std::vector<Mat4> T;
    for (uint32_t i = 0; i < S.inputs.size(); i++)
      if (i == object || S.inputs[i].source == (int32_t)object) { family.push_back(i); T.push_back(S.inputs[i].trans); }
    BuiltScene C = S;
    ReposedTop top;
    EXPECT(prepare_repose(C, family.data(), T.data(), (uint32_t)family.size(), &top, &bad).empty());
    apply_repose(&C, &top);
    EXPECT(identical(C, viaRefit));
    // the top-level refit of the family with its own transforms changes nothing any more
    BuiltScene D = S;
    TopRefit TR;
    EXPECT(prepare_top_refit(D, family.data(), T.data(), (uint32_t)family.size(), &TR).empty());
    apply_top_refit(&D, &TR);
    EXPECT(identical(D, S));
  }
  // an inactive mesh and an inactive instance: the masked fold and the counts; after reactivation the unmasked fold
  {
    BuiltScene C = first;
    const uint32_t off[2] = {2, 3};
    const uint8_t zero[2] = {0, 0}, one[2] = {1, 1};
    EXPECT(apply_set_active(&C, off, zero, 2));
    const BuiltScene masked = C;
    EXPECT(inplace(&C, 1, A1) && inplace(&C, 2, B1));
    check_top(C, masked);
    for (size_t n = 0; n < C.tlas.nodes.size(); n++) EXPECT(C.flat.nodes[n].count == masked.flat.nodes[n].count);
    for (size_t q = 0; q < C.flat.wave_tlas.size(); q++)
      EXPECT(C.flat.wave_tlas[q].l_cnt == masked.flat.wave_tlas[q].l_cnt && C.flat.wave_tlas[q].r_cnt == masked.flat.wave_tlas[q].r_cnt);
    EXPECT(C.active == masked.active);
    EXPECT(apply_set_active(&C, off, one, 2));
    BuiltScene E = first;
    EXPECT(inplace(&E, 1, A1) && inplace(&E, 2, B1));
    EXPECT(identical(C, E));
  }
  // boxes handed in (as the device paths do) are taken as they are; non-finite vertices are taken only where the caller says so
  {
    std::vector<float> boxes;
    refit_boxes(first.blas[1], A1.pos.data(), A1.idx, &boxes);
    BuiltScene C = first, D = first;
    EXPECT(inplace(&C, 1, A1, boxes.data(), false) && inplace(&D, 1, A1));
    EXPECT(identical(C, D));
    MeshInput P = A1;
    P.pos[3 * 17 + 2] = std::numeric_limits<float>::quiet_NaN();
    BuiltScene N = first;
    EXPECT(!inplace(&N, 1, P) && identical(N, first));
    EXPECT(inplace(&N, 1, P, nullptr, false));
    check_top(N, first);
    EXPECT(inplace(&N, 1, A1));                              // a finite refit afterwards leaves no trace of it
    EXPECT(identical(N, D));
  }
  // refusals leave the scene alone: a light, an instance, a sphere, out of range, another vertex count, Inf, a list scene
  const BuiltScene before = S;
  MeshRefit R;
  const MeshInput L = sheet(1, 0.0f, 1.0f);
  EXPECT(!prepare_mesh_refit_inplace(S, 0, L.pos.data(), L.nrm.data(), 4, nullptr, true, &R).empty());
  EXPECT(!prepare_mesh_refit_inplace(S, 3, A1.pos.data(), A1.nrm.data(), 64, nullptr, true, &R).empty());
  EXPECT(!prepare_mesh_refit_inplace(S, 6, A1.pos.data(), A1.nrm.data(), 64, nullptr, true, &R).empty());
  EXPECT(!prepare_mesh_refit_inplace(S, 7, A1.pos.data(), A1.nrm.data(), 64, nullptr, true, &R).empty());
  EXPECT(!prepare_mesh_refit_inplace(S, 1, A1.pos.data(), A1.nrm.data(), 63, nullptr, true, &R).empty());
  {
    MeshInput P = A1;
    P.pos[5] = -std::numeric_limits<float>::infinity();
    EXPECT(!prepare_mesh_refit_inplace(S, 1, P.pos.data(), P.nrm.data(), 64, nullptr, true, &R).empty());
    BuiltScene Lst;
    EXPECT(build_scene(scene(A0, B0), mats, false, &Lst).empty());
    EXPECT(!prepare_mesh_refit_inplace(Lst, 1, A1.pos.data(), A1.nrm.data(), 64, nullptr, true, &R).empty());
  }
  EXPECT(identical(S, before));
  if (failures) return 1;
  std::printf("refit_inplace_sanitized: ok\n");
  return 0;
}
