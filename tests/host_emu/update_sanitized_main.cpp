// Stand-alone check of srt_pt_update_mesh's scene layer (pt_scene.cpp alone; tests/test_pt_update_host.py builds it with
// -fsanitize=address,undefined and runs it once): commit a scene with two meshes and instances, update one mesh - more nodes,
// fewer nodes, the same -, repose, update the other, refused updates, and back; after every step the scene is compared with a
// fresh build_scene of the same inputs.
#include <cmath>
#include <cstdio>
#include <cstring>
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

// n x n quads over [0,1]^2 lifted by amp * a ripple of `waves` periods: 2 n^2 triangles whose tree depends on amp and waves.
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

static bool same_tree(const HostBVH& a, const HostBVH& b) {
  return a.nodes.size() == b.nodes.size() && a.prim == b.prim &&
         (a.nodes.empty() || std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(HostNode)) == 0);
}

// Everything a kernel reads, wherever a mesh is stored.
static bool same_scene(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (a.tlas_nodes != b.tlas_nodes || a.objects.size() != b.objects.size() || a.wave_tlas.size() != b.wave_tlas.size() || a.wave_lazy != b.wave_lazy ||
      a.lazy_objects != b.lazy_objects || a.max_tlas_depth != b.max_tlas_depth || a.max_blas_depth != b.max_blas_depth || a.nodes.size() != b.nodes.size() ||
      a.blas_recs.size() != b.blas_recs.size() || a.tris.size() != b.tris.size() || A.local_boxes != B.local_boxes || !same_tree(A.tlas, B.tlas))
    return false;
  for (size_t i = 0; i < A.blas.size(); i++)
    if (!same_tree(A.blas[i], B.blas[i])) return false;
  if (a.tlas_nodes && std::memcmp(a.nodes.data(), b.nodes.data(), a.tlas_nodes * sizeof(Node)) != 0) return false;
  if (!a.wave_tlas.empty() && std::memcmp(a.wave_tlas.data(), b.wave_tlas.data(), a.wave_tlas.size() * sizeof(WaveInterior)) != 0) return false;
  for (size_t k = 0; k < a.objects.size(); k++) {
    const Object &x = a.objects[k], &y = b.objects[k];
    if (x.kind != y.kind || x.has_trans != y.has_trans || x.material != y.material || x.use_bvh != y.use_bvh || x.id != y.id || x.ntri != y.ntri ||
        x.nnodes != y.nnodes || x.nrec != y.nrec || std::memcmp(&x.trans, &y.trans, 2 * sizeof(Mat4)) != 0)
      return false;
    for (uint32_t t = 0; t < x.ntri; t++)
      if (std::memcmp(&a.tris[x.tri_base + t], &b.tris[y.tri_base + t], sizeof(Tri)) != 0 ||
          std::memcmp(&a.tri_nrm[x.tri_base + t], &b.tri_nrm[y.tri_base + t], sizeof(TriNrm)) != 0 ||
          std::memcmp(&a.tri_packed[9 * (size_t)(x.tri_base + t)], &b.tri_packed[9 * (size_t)(y.tri_base + t)], 9 * sizeof(float)) != 0)
        return false;
    for (uint32_t r = 0; r < x.nrec; r++)
      if (std::memcmp(&a.blas_recs[x.rec_base + r], &b.blas_recs[y.rec_base + r], sizeof(WaveInterior)) != 0) return false;
    for (uint32_t n = 0; n < x.nnodes; n++)
      if (std::memcmp(&a.nodes[x.node_base + n], &b.nodes[y.node_base + n], sizeof(Node)) != 0) return false;
  }
  return true;
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

static bool update(BuiltScene* S, uint32_t object, const MeshInput& m, bool* bad) {
  MeshUpdate U;
  const std::string err = prepare_mesh_update(*S, object, m.pos.data(), m.nrm.data(), (uint32_t)m.pos.size() / 3, nullptr, &U, bad);
  if (!err.empty()) return false;
  apply_mesh_update(S, &U);
  return true;
}

int main() {
  std::vector<Material> mats(2);
  std::memset(mats.data(), 0, 2 * sizeof(Material));
  mats[0].a[0] = mats[0].a[1] = mats[0].a[2] = 0.5f;
  mats[1].type = 3; mats[1].a[0] = mats[1].a[1] = mats[1].a[2] = 5.0f;
  const MeshInput A0 = sheet(7, 0.05f, 1.0f), A1 = sheet(7, 0.6f, 2.5f), A2 = sheet(7, 0.0f, 1.0f), B0 = sheet(5, 0.1f, 1.5f), B1 = sheet(5, 0.9f, 0.5f);

  for (int use_bvh = 1; use_bvh >= 0; use_bvh--) {
    BuiltScene S, first, fresh;
    bool bad = false;
    EXPECT(build_scene(scene(A0, B0), mats, use_bvh != 0, &S).empty());
    first = S;
    const uint64_t nodes0 = S.store[1].nnodes;
    // the first mesh, twice
    EXPECT(update(&S, 1, A1, &bad));
    EXPECT(build_scene(scene(A1, B0), mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_scene(S, fresh));
    EXPECT(S.store[3].nnodes == S.store[1].nnodes && S.store[4].rec_base == S.store[1].rec_base);
    EXPECT(update(&S, 1, A2, &bad));
    EXPECT(build_scene(scene(A2, B0), mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_scene(S, fresh));
    if (use_bvh) EXPECT(fresh.store[1].nnodes != nodes0 || S.store[1].nnodes == nodes0);
    // repose the instances and the sphere, then update the other mesh
    const uint32_t idx[3] = {3, 5, 6};
    const Mat4 nt[3] = {pose(0.35f, 0.9f, 0.4f, -0.7f), pose(0.5f, -1.4f, 0.9f, 0.6f), pose(1.0f, 0.4f, 1.2f, -1.3f)};
    ReposedTop top;
    EXPECT(prepare_repose(S, idx, nt, 3, &top, &bad).empty());
    apply_repose(&S, &top);
    EXPECT(update(&S, 2, B1, &bad));
    std::vector<ObjectInput> moved = scene(A2, B1);
    for (int k = 0; k < 3; k++) moved[idx[k]].trans = nt[k];
    EXPECT(build_scene(moved, mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_scene(S, fresh));
    // refused updates leave the scene alone: a light, an instance, a sphere, out of range, another vertex count, one point
    const BuiltScene before = S;
    MeshUpdate U;
    const MeshInput L = sheet(1, 0.0f, 1.0f);
    EXPECT(!prepare_mesh_update(S, 0, L.pos.data(), L.nrm.data(), 4, nullptr, &U, &bad).empty() && bad);
    EXPECT(!prepare_mesh_update(S, 3, A1.pos.data(), A1.nrm.data(), 64, nullptr, &U, &bad).empty() && bad);
    EXPECT(!prepare_mesh_update(S, 6, A1.pos.data(), A1.nrm.data(), 64, nullptr, &U, &bad).empty() && bad);
    EXPECT(!prepare_mesh_update(S, 7, A1.pos.data(), A1.nrm.data(), 64, nullptr, &U, &bad).empty() && bad);
    EXPECT(!prepare_mesh_update(S, 1, A1.pos.data(), A1.nrm.data(), 63, nullptr, &U, &bad).empty() && bad);
    if (use_bvh) {
      MeshInput P = A1;
      for (float& v : P.pos) v = 0.25f;
      EXPECT(!prepare_mesh_update(S, 1, P.pos.data(), P.nrm.data(), 64, nullptr, &U, &bad).empty() && !bad);
    }
    EXPECT(same_scene(S, before) && S.flat.nodes.size() == before.flat.nodes.size() && S.inputs[1].mesh.pos == before.inputs[1].mesh.pos);
    // and back to the first scene
    const Mat4 back[3] = {pose(0.3f, -1.0f, 0.5f, 0.8f), pose(0.4f, -2.0f, 0.1f, -1.2f), pose(1.0f, -1.0f, 1.5f, 0.3f)};
    ReposedTop again;
    EXPECT(prepare_repose(S, idx, back, 3, &again, &bad).empty());
    apply_repose(&S, &again);
    EXPECT(update(&S, 2, B0, &bad) && update(&S, 1, A0, &bad));
    EXPECT(same_scene(S, first));
    // a second commit of the inputs the updates left behind
    BuiltScene S2;
    EXPECT(build_scene(S.inputs, mats, use_bvh != 0, &S2).empty());
    EXPECT(same_scene(S2, first));
  }
  if (failures) return 1;
  std::printf("update_sanitized: ok\n");
  return 0;
}
