// Stand-alone check of srt_pt_repose_device's scene layer (pt_scene.cpp alone; tests/test_pt_repose_device_host.py builds it
// with -fsanitize=address,undefined and runs it once): prepare_repose_supplied - the per-object values supplied by the caller
// instead of computed - against prepare_repose on the scene and the list of the file given as argv[1], with the posed boxes and
// with a tree built beforehand, in a scene with BVHs and in a list scene; and refused lists, which leave the scene alone.
#include "scene_main_common.h"

static bool same_top(const ReposedTop& a, const ReposedTop& b) {
  return a.listed == b.listed && same_bytes(a.trans, b.trans) && same_bytes(a.tlas.nodes, b.tlas.nodes) && a.tlas.prim == b.tlas.prim &&
         same_bytes(a.tlas_nodes, b.tlas_nodes) && a.max_tlas_depth == b.max_tlas_depth && same_bytes(a.wave_tlas, b.wave_tlas) &&
         a.wave_lazy == b.wave_lazy && a.lazy_objects == b.lazy_objects && same_bytes(a.objects, b.objects);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s scene-file\n", argv[0]); return 2; }
  std::vector<Material> mats;
  std::vector<ObjectInput> inputs;
  std::vector<uint32_t> listed;
  std::vector<Mat4> moved;
  const bool read = load_scene_file(argv[1], &mats, &inputs, &listed, &moved);
  const uint32_t n = (uint32_t)listed.size();
  if (!read || inputs.empty() || !n) { std::printf("cannot read %s\n", argv[1]); return 2; }
  const uint32_t nobj = (uint32_t)inputs.size();

  for (int use_bvh = 1; use_bvh >= 0; use_bvh--) {
    BuiltScene S;
    EXPECT(build_scene(inputs, mats, use_bvh != 0, &S).empty());
    const BuiltScene first = S;
    // what the caller supplies: the listed objects' values, and every object's posed box under the new poses
    std::vector<Mat4> all(nobj);
    for (uint32_t i = 0; i < nobj; i++) all[i] = inputs[i].trans;
    for (uint32_t k = 0; k < n; k++) all[listed[k]] = moved[k];
    std::vector<Mat4> itrans(n);
    std::vector<uint32_t> has(n);
    std::vector<float> boxes(6 * (size_t)nobj), scratch(6);
    for (uint32_t k = 0; k < n; k++) posed_values(moved[k], &S.local_boxes[6 * (size_t)listed[k]], &itrans[k], &has[k], scratch.data());
    for (uint32_t i = 0; i < nobj; i++) {
      Mat4 unused;
      uint32_t h = 0;
      posed_values(all[i], &S.local_boxes[6 * (size_t)i], &unused, &h, &boxes[6 * (size_t)i]);
    }
    bool bad = true;
    ReposedTop want, from_boxes, from_tree;
    EXPECT(prepare_repose(S, listed.data(), moved.data(), n, &want, &bad).empty() && !bad);
    SuppliedPoses P;
    P.trans = moved.data(); P.itrans = itrans.data(); P.has_trans = has.data();
    P.boxes6 = use_bvh ? boxes.data() : nullptr;
    EXPECT(prepare_repose_supplied(S, listed.data(), n, P, &from_boxes, &bad).empty() && !bad);
    EXPECT(same_top(from_boxes, want));
    if (use_bvh) {
      HostBVH tree = want.tlas;                          // a tree the caller built (here: a copy of the host build's)
      P.boxes6 = nullptr; P.prebuilt = &tree;
      EXPECT(prepare_repose_supplied(S, listed.data(), n, P, &from_tree, &bad).empty() && !bad);
      EXPECT(same_top(from_tree, want) && tree.nodes.empty());
      // neither boxes nor a tree: refused as an argument
      ReposedTop none;
      P.prebuilt = nullptr;
      EXPECT(!prepare_repose_supplied(S, listed.data(), n, P, &none, &bad).empty() && bad);
      P.boxes6 = boxes.data();
    }
    EXPECT(same_posed_scene(S, first));                        // preparing leaves the scene alone
    // refused lists: a duplicate, out of range, an area light
    ReposedTop refused;
    std::vector<uint32_t> dup(listed);
    dup[n - 1] = dup[0];
    EXPECT(prepare_repose_supplied(S, dup.data(), n, P, &refused, &bad).find("listed twice") != std::string::npos && bad);
    std::vector<uint32_t> range(listed);
    range[0] = nobj;
    EXPECT(prepare_repose_supplied(S, range.data(), n, P, &refused, &bad).find("out of range") != std::string::npos && bad);
    for (uint32_t i = 0; i < nobj; i++)
      if (inputs[i].is_light) {
        std::vector<uint32_t> light(listed);
        light[0] = i;
        EXPECT(prepare_repose_supplied(S, light.data(), n, P, &refused, &bad).find("area light") != std::string::npos && bad);
        EXPECT(check_repose_list(S, light.data(), n) == prepare_repose(S, light.data(), moved.data(), n, &refused, &bad));
        break;
      }
    EXPECT(same_posed_scene(S, first));
    // applied: the scene of a fresh build on the new poses, and of srt_pt_repose's path
    BuiltScene H = S, fresh;
    apply_repose(&S, &from_boxes);
    apply_repose(&H, &want);
    std::vector<ObjectInput> posed_inputs = inputs;
    for (uint32_t i = 0; i < nobj; i++) posed_inputs[i].trans = all[i];
    EXPECT(build_scene(posed_inputs, mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_posed_scene(S, H) && same_posed_scene(S, fresh));
    // and back, supplied again: the unlisted objects take their values from the records the first repose left
    std::vector<Mat4> home(n), home_inv(n);
    std::vector<uint32_t> home_has(n);
    for (uint32_t k = 0; k < n; k++) home[k] = inputs[listed[k]].trans;
    for (uint32_t k = 0; k < n; k++) posed_values(home[k], &S.local_boxes[6 * (size_t)listed[k]], &home_inv[k], &home_has[k], scratch.data());
    for (uint32_t i = 0; i < nobj; i++) {
      Mat4 unused;
      uint32_t h = 0;
      posed_values(inputs[i].trans, &S.local_boxes[6 * (size_t)i], &unused, &h, &boxes[6 * (size_t)i]);
    }
    SuppliedPoses Q;
    Q.trans = home.data(); Q.itrans = home_inv.data(); Q.has_trans = home_has.data();
    Q.boxes6 = use_bvh ? boxes.data() : nullptr;
    ReposedTop back;
    EXPECT(prepare_repose_supplied(S, listed.data(), n, Q, &back, &bad).empty() && !bad);
    apply_repose(&S, &back);
    EXPECT(same_posed_scene(S, first));
  }
  if (failures) return 1;
  std::printf("repose_device_sanitized: ok (%u objects, %u listed)\n", nobj, n);
  return 0;
}
