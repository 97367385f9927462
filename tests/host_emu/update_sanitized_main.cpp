// Stand-alone check of srt_pt_update_mesh's scene layer (pt_scene.cpp alone; tests/test_pt_update_host.py builds it with
// -fsanitize=address,undefined and runs it once): commit a scene with two meshes and instances, update one mesh - more nodes,
// fewer nodes, the same -, repose, update the other, refused updates, and back; after every step the scene is compared with a
// fresh build_scene of the same inputs.
#include "scene_main_common.h"

// Everything a kernel reads, wherever a mesh is stored.
static bool same_scene(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (a.max_blas_depth != b.max_blas_depth || a.nodes.size() != b.nodes.size() || a.blas_recs.size() != b.blas_recs.size() || a.tris.size() != b.tris.size() ||
      A.local_boxes != B.local_boxes || !same_tree(A.tlas, B.tlas))
    return false;
  for (size_t i = 0; i < A.blas.size(); i++)
    if (!same_tree(A.blas[i], B.blas[i])) return false;
  return same_contents(a, b);
}

static bool update(BuiltScene* S, uint32_t object, const MeshInput& m, bool* bad) {
  MeshUpdate U;
  const std::string err = prepare_mesh_update(*S, object, m.pos.data(), m.nrm.data(), (uint32_t)m.pos.size() / 3, nullptr, &U, bad);
  if (!err.empty()) return false;
  apply_mesh_update(S, &U);
  return true;
}

int main() {
  const std::vector<Material> mats = two_materials();
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
