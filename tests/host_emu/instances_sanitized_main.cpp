// Stand-alone check of instanced scenes and re-posing on the host side (pt_scene.cpp alone; tests/test_pt_instances_host.py builds
// it with -fsanitize=address,undefined and runs it once): commit a scene with instances, compare it with the same scene made of
// copies, repose it - good lists, refused lists, poses whose BVH<Object> build does not terminate -, commit again.
#include "scene_main_common.h"

// A grid of n x n quads over [0,1]^2 lifted into a shallow bowl: 2 n^2 triangles, enough for a BVH<Triangle> with interior nodes.
static MeshInput bowl(int n) {
  MeshInput m;
  for (int j = 0; j <= n; j++)
    for (int i = 0; i <= n; i++) {
      const float x = (float)i / n, z = (float)j / n;
      const float p[3] = {x, 0.3f * ((x - 0.5f) * (x - 0.5f) + (z - 0.5f) * (z - 0.5f)), z};
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

static std::vector<ObjectInput> scene(bool instanced, const std::vector<Mat4>& poses) {
  std::vector<ObjectInput> in;
  const MeshInput m = bowl(6);
  ObjectInput light;                                 // 0: an area light, a mesh of its own
  light.trans = pose(0.5f, 0.0f, 2.0f, 0.0f);
  light.material = 1; light.is_light = true; light.mesh = bowl(1);
  in.push_back(light);
  for (size_t k = 0; k < poses.size(); k++) {        // 1 ..: the mesh and its instances (or copies)
    ObjectInput o;
    o.trans = poses[k];
    if (k == 0 || !instanced) o.mesh = m; else o.source = 1;
    in.push_back(o);
  }
  ObjectInput s;                                     // last: a sphere
  s.kind = OBJ_SPHERE; s.radius = 0.2f; s.trans = pose(1.0f, -1.0f, 0.5f, 0.3f);
  in.push_back(s);
  return in;
}

int main() {
  const std::vector<Material> mats = two_materials();
  std::vector<Mat4> poses;
  for (int k = 0; k < 24; k++) poses.push_back(pose(0.1f + 0.01f * (k % 5), 0.37f * k - 3.0f, 0.11f * ((k * 7) % 9), 0.53f * ((k * 5) % 11) - 2.0f));
  poses[0] = mat_identity();                         // the source itself has no transform

  for (int use_bvh = 1; use_bvh >= 0; use_bvh--) {
    BuiltScene S, C;
    EXPECT(build_scene(scene(true, poses), mats, use_bvh != 0, &S).empty());
    EXPECT(build_scene(scene(false, poses), mats, use_bvh != 0, &C).empty());
    EXPECT(same_contents(S.flat, C.flat) && same_tree(S.tlas, C.tlas));
    EXPECT(C.flat.tris.size() - S.flat.tris.size() == 23u * 72u);
    EXPECT(S.blas_builds + 23 * (uint64_t)use_bvh == C.blas_builds);

    // refused lists leave the scene alone
    ReposedTop top;
    bool bad = false;
    const Mat4 T1 = pose(0.2f, 0.4f, 0.4f, 0.4f);
    const uint32_t light_idx[1] = {0}, twice[2] = {3, 3}, beyond[1] = {26};
    const Mat4 two[2] = {T1, T1};
    EXPECT(!prepare_repose(S, light_idx, &T1, 1, &top, &bad).empty() && bad);
    EXPECT(!prepare_repose(S, twice, two, 2, &top, &bad).empty() && bad);
    EXPECT(!prepare_repose(S, beyond, &T1, 1, &top, &bad).empty() && bad);
    EXPECT(same_contents(S.flat, C.flat));

    // a good list: the source, a few instances, the sphere - against a fresh commit of the new poses
    std::vector<uint32_t> idx = {1, 4, 9, 17, 24, 25};
    std::vector<Mat4> nt;
    std::vector<Mat4> moved = poses;
    for (size_t k = 0; k < idx.size(); k++) nt.push_back(pose(0.15f, 0.21f * k - 1.0f, 1.0f + 0.17f * k, -0.4f * k));
    nt[0].c[1][1] = 0.4f;                              // the source: non-uniform scale
    for (size_t k = 0; k + 1 < idx.size(); k++) moved[idx[k] - 1] = nt[k];
    EXPECT(prepare_repose(S, idx.data(), nt.data(), (uint32_t)idx.size(), &top, &bad).empty() && !bad);
    EXPECT(same_contents(S.flat, C.flat));                 // prepared aside: nothing has changed yet
    apply_repose(&S, &top);
    std::vector<ObjectInput> fresh_in = scene(false, moved);
    fresh_in.back().trans = nt.back();
    BuiltScene fresh;
    EXPECT(build_scene(fresh_in, mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_contents(S.flat, fresh.flat) && same_tree(S.tlas, fresh.tlas));
    EXPECT(S.flat.tris.size() + 23u * 72u == fresh.flat.tris.size() && S.flat.light_tri_first + 23u * 72u == fresh.flat.light_tri_first);

    // two instances on one pose: BVH<Object>::build would never return; refused, the scene stays
    if (use_bvh) {
      const uint32_t pair[2] = {5, 6};
      const BuiltScene before = S;
      ReposedTop stuck;
      EXPECT(!prepare_repose(S, pair, two, 2, &stuck, &bad).empty() && !bad);
      EXPECT(same_contents(S.flat, before.flat) && same_tree(S.tlas, before.tlas));
    }

    // back to the first poses, then a second commit of the same inputs
    std::vector<Mat4> back;
    for (size_t k = 0; k + 1 < idx.size(); k++) back.push_back(poses[idx[k] - 1]);
    back.push_back(pose(1.0f, -1.0f, 0.5f, 0.3f));
    ReposedTop again;
    EXPECT(prepare_repose(S, idx.data(), back.data(), (uint32_t)idx.size(), &again, &bad).empty());
    apply_repose(&S, &again);
    EXPECT(same_contents(S.flat, C.flat) && same_tree(S.tlas, C.tlas));
    BuiltScene S2;
    EXPECT(build_scene(S.inputs, mats, use_bvh != 0, &S2).empty());
    EXPECT(same_contents(S2.flat, C.flat) && same_tree(S2.tlas, C.tlas));
    // an instance of an instance, of a sphere, of something later: refused by build_scene as well
    std::vector<ObjectInput> bad_in = scene(true, poses);
    bad_in[5].source = 4;
    EXPECT(!build_scene(bad_in, mats, use_bvh != 0, &S2).empty());
    bad_in[5].source = 25;
    EXPECT(!build_scene(bad_in, mats, use_bvh != 0, &S2).empty());
  }
  if (failures) return 1;
  std::printf("instances_sanitized: ok\n");
  return 0;
}
