// Stand-alone check of srt_pt_refit_mesh's scene layer (pt_scene.cpp alone; tests/test_pt_refit_host.py builds it with
// -fsanitize=address,undefined and runs it once) over the scene of update_sanitized_main.cpp: two meshes, instances, a light and
// a sphere.  Identity refit, refits of both meshes with a repose in between, every refusal, then an update on top of a refit;
// after every refit the tree's links and order are the committed ones, every box is the fold it is defined as, and the flattened
// nodes, records and triangle records say the same as the host tree.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pt_scene.h"

using namespace srt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static Mat4 pose(float s, float x, float y, float z) {
  Mat4 m = mat_identity();
  m.c[0][0] = m.c[1][1] = m.c[2][2] = s;
  m.c[3][0] = x; m.c[3][1] = y; m.c[3][2] = z;
  return m;
}

// n x n quads over [0,1]^2 lifted by amp * a ripple of `waves` periods (amp == 0: a flat sheet, every triangle box widened by +1)
static MeshInput sheet(int n, float amp, float waves) {
  MeshInput m;
  for (int j = 0; j <= n; j++)
    for (int i = 0; i <= n; i++) {
      const float x = (float)i / n, z = (float)j / n;
      const float p[3] = {x, amp * std::sin(6.2831853f * waves * x) * std::cos(6.2831853f * waves * z), z};
      const float nn[3] = {0.0f, 1.0f, 0.0f};
      m.pos.insert(m.pos.end(), p, p + 3);
      m.nrm.insert(m.nrm.end(), nn, nn + 3);
    }
  for (int j = 0; j < n; j++)
    for (int i = 0; i < n; i++) {
      const uint32_t a = (uint32_t)(j * (n + 1) + i), b = a + 1, c = a + (uint32_t)n + 1, d = c + 1;
      const uint32_t t[6] = {a, c, b, b, c, d};
      m.idx.insert(m.idx.end(), t, t + 6);
    }
  return m;
}

// 0: an area light; 1: sheet A; 2: sheet B; 3, 4: instances of A; 5: an instance of B; 6: a sphere
static std::vector<ObjectInput> scene(const MeshInput& A, const MeshInput& B) {
  std::vector<ObjectInput> in;
  ObjectInput light;
  light.trans = pose(0.5f, 0.0f, 2.0f, 0.0f);
  light.material = 1; light.is_light = true; light.mesh = sheet(1, 0.0f, 1.0f);
  in.push_back(light);
  ObjectInput a; a.trans = mat_identity(); a.mesh = A; in.push_back(a);
  ObjectInput b; b.trans = pose(0.7f, 1.5f, 0.2f, -0.4f); b.mesh = B; in.push_back(b);
  ObjectInput i1; i1.trans = pose(0.3f, -1.0f, 0.5f, 0.8f); i1.source = 1; in.push_back(i1);
  ObjectInput i2; i2.trans = pose(0.6f, 0.2f, -1.1f, 1.9f); i2.source = 1; in.push_back(i2);
  ObjectInput i3; i3.trans = pose(0.4f, -2.0f, 0.1f, -1.2f); i3.source = 2; in.push_back(i3);
  ObjectInput s; s.kind = OBJ_SPHERE; s.radius = 0.2f; s.trans = pose(1.0f, -1.0f, 1.5f, 0.3f); in.push_back(s);
  return in;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// Byte for byte: host trees, inputs and every flattened array.
static bool identical(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (!same_bytes(a.nodes, b.nodes) || !same_bytes(a.tris, b.tris) || !same_bytes(a.tri_nrm, b.tri_nrm) || a.tri_packed != b.tri_packed ||
      !same_bytes(a.objects, b.objects) || !same_bytes(a.wave_tlas, b.wave_tlas) || !same_bytes(a.blas_recs, b.blas_recs) || a.wave_lazy != b.wave_lazy ||
      a.lazy_objects != b.lazy_objects || a.tlas_nodes != b.tlas_nodes || a.max_tlas_depth != b.max_tlas_depth || a.max_blas_depth != b.max_blas_depth)
    return false;
  if (A.local_boxes != B.local_boxes || !same_bytes(A.tlas.nodes, B.tlas.nodes) || A.tlas.prim != B.tlas.prim || A.blas.size() != B.blas.size()) return false;
  for (size_t i = 0; i < A.blas.size(); i++)
    if (!same_bytes(A.blas[i].nodes, B.blas[i].nodes) || A.blas[i].prim != B.blas[i].prim || A.inputs[i].mesh.pos != B.inputs[i].mesh.pos ||
        A.inputs[i].mesh.nrm != B.inputs[i].mesh.nrm)
      return false;
  return true;
}

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
  std::vector<Material> mats(2);
  std::memset(mats.data(), 0, 2 * sizeof(Material));
  mats[0].a[0] = mats[0].a[1] = mats[0].a[2] = 0.5f;
  mats[1].type = 3; mats[1].a[0] = mats[1].a[1] = mats[1].a[2] = 5.0f;
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
