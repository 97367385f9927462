// Stand-alone check of srt_pt_set_dynamic_lights' scene layer (pt_scene.cpp alone; tests/test_pt_lights_host.py builds it with
// -fsanitize=address,undefined and runs it once): commit a scene with an emissive sheet, an emissive sphere and a plain mesh,
// repose the lights, update and refit the emissive sheet, make refused calls; after every step the light tables are compared
// with a fresh build_scene of the same inputs.
#include <limits>

#include "scene_main_common.h"

// The light tables and what a pose decides, wherever the light range starts.
static bool same_lights(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (a.lights.size() != b.lights.size() || !same_bytes(a.light_tris, b.light_tris) || a.objects.size() != b.objects.size()) return false;
  const size_t n = a.tris.size() - a.light_tri_first;
  if (n != b.tris.size() - b.light_tri_first || n != a.light_tris.size()) return false;
  if (n && (std::memcmp(&a.tris[a.light_tri_first], &b.tris[b.light_tri_first], n * sizeof(Tri)) != 0 ||
            std::memcmp(&a.tri_nrm[a.light_tri_first], &b.tri_nrm[b.light_tri_first], n * sizeof(TriNrm)) != 0 ||
            std::memcmp(&a.tri_packed[9 * (size_t)a.light_tri_first], &b.tri_packed[9 * (size_t)b.light_tri_first], 9 * n * sizeof(float)) != 0))
    return false;
  for (size_t k = 0; k < a.lights.size(); k++) {
    Light x = a.lights[k], y = b.lights[k];
    x.tri_base -= a.light_tri_first; y.tri_base -= b.light_tri_first;
    if (std::memcmp(&x, &y, sizeof x) != 0) return false;
  }
  for (size_t k = 0; k < a.objects.size(); k++)
    if (a.objects[k].id != b.objects[k].id || a.objects[k].has_trans != b.objects[k].has_trans ||
        std::memcmp(&a.objects[k].trans, &b.objects[k].trans, 2 * sizeof(Mat4)) != 0)
      return false;
  return A.local_boxes == B.local_boxes;
}

// 0: a plain sheet; 1: an emissive sheet; 2: an emissive sphere (its light mesh: a quad); 3: an instance of 0
static std::vector<ObjectInput> scene(const MeshInput& E, const Mat4& light_pose, const Mat4& sphere_pose) {
  std::vector<ObjectInput> in;
  ObjectInput a; a.trans = pose(2.0f, -1.0f, 0.0f, -1.0f); a.mesh = sheet(6, 0.1f, 1.0f); in.push_back(a);
  ObjectInput e; e.trans = light_pose; e.material = 1; e.is_light = true; e.mesh = E; in.push_back(e);
  ObjectInput s; s.kind = OBJ_SPHERE; s.radius = 0.2f; s.trans = sphere_pose; s.material = 1; s.is_light = true; s.mesh = sheet(1, 0.0f, 1.0f); in.push_back(s);
  ObjectInput i; i.trans = pose(0.5f, 1.5f, 0.4f, 0.3f); i.source = 0; in.push_back(i);
  return in;
}

static bool build(const std::vector<ObjectInput>& in, const std::vector<Material>& mats, bool use_bvh, bool dynamic, BuiltScene* out) {
  out->dynamic_lights = dynamic;
  return build_scene(in, mats, use_bvh, out).empty() && out->dynamic_lights == dynamic;
}

int main() {
  const std::vector<Material> mats = two_materials();
  const MeshInput E0 = sheet(5, 0.05f, 1.0f), E1 = sheet(5, 0.5f, 2.0f), E2 = sheet(5, 0.0f, 1.0f);
  const Mat4 L0 = pose(0.5f, 0.0f, 2.0f, 0.0f), S0 = pose(1.0f, -1.0f, 1.5f, 0.3f);
  Mat4 L1 = pose(0.8f, 0.3f, 1.7f, -0.2f);
  L1.c[0][0] = 0.6f; L1.c[0][2] = -0.35f; L1.c[2][0] = 0.45f; L1.c[2][2] = 0.9f;   // a rotation with a non-uniform scale
  const Mat4 S1 = pose(1.0f, 0.5f, 1.1f, -0.6f);

  for (int use_bvh = 1; use_bvh >= 0; use_bvh--) {
    BuiltScene S, first, fresh;
    bool bad = false;
    EXPECT(build(scene(E0, L0, S0), mats, use_bvh != 0, true, &S));
    first = S;
    EXPECT(light_of(S, 0) == -1 && light_of(S, 1) == 0 && light_of(S, 2) == 1 && light_of(S, 3) == -1 && light_of(S, 4) == -1);
    // repose both lights, then the mesh light into the identity (has_trans 1 -> 0) and out of it again
    const uint32_t both[2] = {1, 2};
    const Mat4 nt[2] = {L1, S1};
    ReposedTop top;
    EXPECT(prepare_repose(S, both, nt, 2, &top, &bad).empty());
    apply_repose(&S, &top);
    EXPECT(build(scene(E0, L1, S1), mats, use_bvh != 0, false, &fresh) && same_lights(S, fresh));
    const uint32_t one[1] = {1};
    const Mat4 id = mat_identity();
    ReposedTop t2;
    EXPECT(prepare_repose(S, one, &id, 1, &t2, &bad).empty());
    apply_repose(&S, &t2);
    EXPECT(build(scene(E0, id, S1), mats, use_bvh != 0, false, &fresh) && same_lights(S, fresh) && S.flat.lights[0].has_trans == 0u);
    ReposedTop t3;
    EXPECT(prepare_repose(S, one, &L1, 1, &t3, &bad).empty());
    apply_repose(&S, &t3);
    EXPECT(build(scene(E0, L1, S1), mats, use_bvh != 0, false, &fresh) && same_lights(S, fresh) && S.flat.lights[0].has_trans == 1u);
    // update the emissive sheet
    MeshUpdate U;
    EXPECT(prepare_mesh_update(S, 1, E1.pos.data(), E1.nrm.data(), (uint32_t)E1.pos.size() / 3, nullptr, &U, &bad).empty());
    apply_mesh_update(&S, &U);
    EXPECT(build(scene(E1, L1, S1), mats, use_bvh != 0, false, &fresh) && same_lights(S, fresh));
    // refit it (a scene with trees only)
    if (use_bvh) {
      MeshRefit R;
      EXPECT(prepare_mesh_refit(S, 1, E2.pos.data(), E2.nrm.data(), (uint32_t)E2.pos.size() / 3, nullptr, &R, &bad).empty());
      apply_mesh_refit(&S, &R);
      EXPECT(build(scene(E2, L1, S1), mats, use_bvh != 0, false, &fresh) && same_lights(S, fresh));
    }
    // refused calls leave everything alone: the sphere light's vertices, a duplicate, a non-finite refit, and - the switch
    // cleared - the lights themselves
    const BuiltScene before = S;
    const MeshInput Q = sheet(1, 0.0f, 1.0f);
    MeshUpdate U2;
    MeshRefit R2;
    ReposedTop t4;
    EXPECT(!prepare_mesh_update(S, 2, Q.pos.data(), Q.nrm.data(), 4, nullptr, &U2, &bad).empty() && bad);
    const uint32_t twice[2] = {1, 1};
    EXPECT(!prepare_repose(S, twice, nt, 2, &t4, &bad).empty() && bad);
    if (use_bvh) {
      MeshInput N = E1;
      N.pos[7] = std::numeric_limits<float>::infinity();
      EXPECT(!prepare_mesh_refit(S, 1, N.pos.data(), N.nrm.data(), (uint32_t)N.pos.size() / 3, nullptr, &R2, &bad).empty() && bad);
    }
    S.dynamic_lights = false;
    EXPECT(prepare_repose(S, one, &L0, 1, &t4, &bad).find("is an area light") != std::string::npos && bad);
    EXPECT(prepare_mesh_update(S, 1, E0.pos.data(), E0.nrm.data(), (uint32_t)E0.pos.size() / 3, nullptr, &U2, &bad).find("is an area light") != std::string::npos && bad);
    S.dynamic_lights = true;
    EXPECT(same_lights(S, before) && same_bytes(S.flat.nodes, before.flat.nodes) && same_bytes(S.flat.tris, before.flat.tris) &&
           S.inputs[1].mesh.pos == before.inputs[1].mesh.pos);
    // and back to the first scene
    const Mat4 back[2] = {L0, S0};
    ReposedTop t5;
    EXPECT(prepare_repose(S, both, back, 2, &t5, &bad).empty());
    apply_repose(&S, &t5);
    MeshUpdate U3;
    EXPECT(prepare_mesh_update(S, 1, E0.pos.data(), E0.nrm.data(), (uint32_t)E0.pos.size() / 3, nullptr, &U3, &bad).empty());
    apply_mesh_update(&S, &U3);
    EXPECT(same_lights(S, first) && same_bytes(S.flat.nodes, first.flat.nodes) && same_bytes(S.flat.tris, first.flat.tris));
  }
  if (failures) return 1;
  std::printf("lights_sanitized: ok\n");
  return 0;
}
