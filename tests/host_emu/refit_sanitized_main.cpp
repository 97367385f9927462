// Stand-alone check of srt_pt_refit_mesh's scene layer (pt_scene.cpp alone; tests/test_pt_refit_host.py builds it with
// -fsanitize=address,undefined and runs it once) over scene_main_common.h:scene(): two meshes, instances, a light and
// a sphere.  Identity refit, refits of both meshes with a repose in between, every refusal, then an update on top of a refit;
// after every refit the tree's links and order are the committed ones, every box is the fold it is defined as, and the flattened
// nodes, records and triangle records say the same as the host tree.
#include <algorithm>
#include <limits>

#include "scene_main_common.h"

static bool refit(BuiltScene* S, uint32_t object, const MeshInput& m, bool* bad) {
  MeshRefit R;
  const std::string err = prepare_mesh_refit(*S, object, m.pos.data(), m.nrm.data(), (uint32_t)m.pos.size() / 3, nullptr, &R, bad);
  if (!err.empty()) return false;
  apply_mesh_refit(S, &R);
  return true;
}

// The refitted mesh `object` of S against its definition, from the vertices m and the committed tree `was`.
static void check_refitted(const BuiltScene& S, uint32_t object, const MeshInput& m, const HostBVH& was) {
  const HostBVH& t = S.blas[object];
  const FlatScene& F = S.flat;
  const MeshStore st = S.store[object];
  EXPECT(t.prim == was.prim && t.nodes.size() == was.nodes.size());
  uint32_t rec = st.rec_base;
  for (size_t n = 0; n < t.nodes.size(); n++) {
    const HostNode& h = t.nodes[n];
    EXPECT(h.start == was.nodes[n].start && h.size == was.nodes[n].size && h.l == was.nodes[n].l && h.r == was.nodes[n].r);
    float mn[3] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), std::numeric_limits<float>::max()}, mx[3] = {-mn[0], -mn[1], -mn[2]};
    if (h.l == h.r) {
      for (uint32_t k = h.start; k < h.start + h.size; k++)
        for (int a = 0; a < 3; a++) {
          float lo = mn[0], hi = lo;
          for (int c = 0; c < 3; c++) {
            const float v = m.pos[3 * (size_t)m.idx[3 * (size_t)t.prim[k] + c] + a];
            lo = c ? std::min(lo, v) : v; hi = c ? std::max(hi, v) : v;
          }
          if (lo >= hi) hi = lo + 1.0f;
          mn[a] = std::min(mn[a], lo); mx[a] = std::max(mx[a], hi);
        }
    } else {
      for (int a = 0; a < 3; a++) { mn[a] = std::min(t.nodes[h.l].mn[a], t.nodes[h.r].mn[a]); mx[a] = std::max(t.nodes[h.l].mx[a], t.nodes[h.r].mx[a]); }
      const WaveInterior& w = F.blas_recs[rec++];
      EXPECT(std::memcmp(w.boxl, t.nodes[h.l].mn, 24) == 0 && std::memcmp(w.boxr, t.nodes[h.r].mn, 24) == 0);
      EXPECT(w.l_cnt == t.nodes[h.l].size && w.r_cnt == t.nodes[h.r].size);
    }
    for (int a = 0; a < 3; a++) EXPECT(h.mn[a] == mn[a] && h.mx[a] == mx[a]);
    const Node& f = F.nodes[(size_t)F.tlas_nodes + st.node_off + n];
    EXPECT(std::memcmp(f.mn, h.mn, 12) == 0 && std::memcmp(f.mx, h.mx, 12) == 0);
    EXPECT(h.l == h.r ? (f.left == h.start && f.count == (LEAF_BIT | h.size)) : (f.left == h.l && f.count == 0));
  }
  EXPECT(rec == st.rec_base + st.nrec);
  for (uint32_t k = 0; k < st.ntri; k++) {
    const float* p0 = &m.pos[3 * (size_t)m.idx[3 * (size_t)t.prim[k]]];
    const float* p1 = &m.pos[3 * (size_t)m.idx[3 * (size_t)t.prim[k] + 1]];
    const Tri& g = F.tris[st.tri_base + k];
    for (int a = 0; a < 3; a++) EXPECT(g.p0[a] == p0[a] && g.e1[a] == p1[a] - p0[a] && F.tri_packed[9 * (size_t)(st.tri_base + k) + a] == p0[a]);
  }
  // the mesh and its instances carry the root box
  for (size_t i = 0; i < S.inputs.size(); i++)
    if (i == object || S.inputs[i].source == (int32_t)object) EXPECT(std::memcmp(&S.local_boxes[6 * i], t.nodes[0].mn, 24) == 0);
  EXPECT(S.inputs[object].mesh.pos == m.pos && S.inputs[object].mesh.nrm == m.nrm);
}

int main() {
  const std::vector<Material> mats = two_materials();
  const MeshInput A0 = sheet(7, 0.05f, 1.0f), A1 = sheet(7, 0.6f, 2.5f), A2 = sheet(7, 0.0f, 1.0f), B0 = sheet(5, 0.1f, 1.5f), B1 = sheet(5, 0.9f, 0.5f);

  BuiltScene S, first, fresh;
  bool bad = false;
  EXPECT(build_scene(scene(A0, B0), mats, true, &S).empty());
  first = S;
  const HostBVH treeA = S.blas[1], treeB = S.blas[2];
  const double cost0 = tree_cost(S.blas[1]);
  // identity: the committed vertices give the committed scene back
  EXPECT(refit(&S, 1, A0, &bad));
  EXPECT(identical(S, first));
  EXPECT(tree_cost(S.blas[1]) == cost0);
  // the first mesh, a ripple and then flat (every box widened by +1 on the flat axis); the other mesh's tree is not touched
  EXPECT(refit(&S, 1, A1, &bad));
  check_refitted(S, 1, A1, treeA);
  EXPECT(same_bytes(S.blas[2].nodes, first.blas[2].nodes));
  EXPECT(build_scene(scene(A1, B0), mats, true, &fresh).empty());
  EXPECT(same_bytes(S.tlas.nodes, fresh.tlas.nodes) && S.tlas.prim == fresh.tlas.prim && S.local_boxes == fresh.local_boxes);   // the top half is a fresh commit's
  EXPECT(tree_cost(S.blas[1]) >= tree_cost(fresh.blas[1]) * 0.5);
  EXPECT(refit(&S, 1, A2, &bad));
  check_refitted(S, 1, A2, treeA);
  EXPECT(S.blas[1].nodes[0].mx[1] == 1.0f && S.blas[1].nodes[0].mn[1] == 0.0f);
  // repose the instances and the sphere, then refit the other mesh
  const uint32_t idx[3] = {3, 5, 6};
  const Mat4 nt[3] = {pose(0.35f, 0.9f, 0.4f, -0.7f), pose(0.5f, -1.4f, 0.9f, 0.6f), pose(1.0f, 0.4f, 1.2f, -1.3f)};
  ReposedTop top;
  EXPECT(prepare_repose(S, idx, nt, 3, &top, &bad).empty());
  apply_repose(&S, &top);
  EXPECT(refit(&S, 2, B1, &bad));
  check_refitted(S, 2, B1, treeB);
  check_refitted(S, 1, A2, treeA);
  std::vector<ObjectInput> moved = scene(A2, B1);
  for (int k = 0; k < 3; k++) moved[idx[k]].trans = nt[k];
  EXPECT(build_scene(moved, mats, true, &fresh).empty());
  EXPECT(same_bytes(S.tlas.nodes, fresh.tlas.nodes) && S.tlas.prim == fresh.tlas.prim);
  // refusals leave the scene alone: a light, an instance, a sphere, out of range, another vertex count, NaN, Inf
  const BuiltScene before = S;
  MeshRefit R;
  const MeshInput L = sheet(1, 0.0f, 1.0f);
  EXPECT(!prepare_mesh_refit(S, 0, L.pos.data(), L.nrm.data(), 4, nullptr, &R, &bad).empty() && bad);
  EXPECT(!prepare_mesh_refit(S, 3, A1.pos.data(), A1.nrm.data(), 64, nullptr, &R, &bad).empty() && bad);
  EXPECT(!prepare_mesh_refit(S, 6, A1.pos.data(), A1.nrm.data(), 64, nullptr, &R, &bad).empty() && bad);
  EXPECT(!prepare_mesh_refit(S, 7, A1.pos.data(), A1.nrm.data(), 64, nullptr, &R, &bad).empty() && bad);
  EXPECT(!prepare_mesh_refit(S, 1, A1.pos.data(), A1.nrm.data(), 63, nullptr, &R, &bad).empty() && bad);
  for (const float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
    MeshInput P = A1;
    P.pos[3 * 17 + 2] = v;
    EXPECT(!prepare_mesh_refit(S, 1, P.pos.data(), P.nrm.data(), 64, nullptr, &R, &bad).empty() && bad);
  }
  EXPECT(identical(S, before));
  {  // every vertex at one point: no build runs, so nothing can fail to terminate - unless the top half does
    MeshInput P = A1;
    for (float& v : P.pos) v = 0.25f;
    BuiltScene C = S;
    EXPECT(refit(&C, 1, P, &bad));
    check_refitted(C, 1, P, treeA);
  }
  {  // a scene without BVHs has no tree to refit
    BuiltScene Lst;
    EXPECT(build_scene(scene(A0, B0), mats, false, &Lst).empty());
    EXPECT(!prepare_mesh_refit(Lst, 1, A1.pos.data(), A1.nrm.data(), 64, nullptr, &R, &bad).empty() && bad);
  }
  // boxes handed in (as the device path does) are taken as they are
  {
    std::vector<float> boxes;
    refit_boxes(S.blas[1], A1.pos.data(), A1.idx, &boxes);
    BuiltScene C = S, D = S;
    EXPECT(prepare_mesh_refit(C, 1, A1.pos.data(), A1.nrm.data(), 64, boxes.data(), &R, &bad).empty());
    apply_mesh_refit(&C, &R);
    EXPECT(refit(&D, 1, A1, &bad));
    EXPECT(identical(C, D));
  }
  // an update on top of a refit is a fresh commit
  MeshUpdate U;
  EXPECT(refit(&S, 1, A1, &bad));
  EXPECT(prepare_mesh_update(S, 1, A1.pos.data(), A1.nrm.data(), 64, nullptr, &U, &bad).empty());
  apply_mesh_update(&S, &U);
  moved = scene(A1, B1);
  for (int k = 0; k < 3; k++) moved[idx[k]].trans = nt[k];
  EXPECT(build_scene(moved, mats, true, &fresh).empty());
  EXPECT(same_bytes(S.blas[1].nodes, fresh.blas[1].nodes) && S.blas[1].prim == fresh.blas[1].prim && same_bytes(S.tlas.nodes, fresh.tlas.nodes));
  if (failures) return 1;
  std::printf("refit_sanitized: ok\n");
  return 0;
}
