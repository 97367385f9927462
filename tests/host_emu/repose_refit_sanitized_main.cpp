// Stand-alone check of srt_pt_repose_refit's scene layer (pt_scene.cpp alone; tests/test_pt_repose_refit_host.py builds it with
// -fsanitize=address,undefined and runs it once) on the scene and the list of the file given as argv[1] (the format of
// scene_main_common.h:load_scene_file): the definition - prepare_top_refit / apply_top_refit - and the settle path, which applies
// records and boxes that were computed elsewhere (here: copied out of a refitted scene, as srt_pt_repose_refit_device's
// read-back delivers them), in a scene with BVHs and in a list scene.  After every refit the tree's links and order are the
// committed ones, every box is the fold it is defined as, and the flattened nodes and sweep records say what the host tree says.
#include <algorithm>
#include <limits>

#include "scene_main_common.h"

// The refitted top of S against its definition: the transforms `all` of every object, the committed scene `was`.
static void check_refitted(const BuiltScene& S, const std::vector<Mat4>& all, const BuiltScene& was) {
  const HostBVH& t = S.tlas;
  const FlatScene& F = S.flat;
  EXPECT(t.prim == was.tlas.prim && t.nodes.size() == was.tlas.nodes.size() && F.tlas_nodes == was.flat.tlas_nodes);
  EXPECT(F.wave_lazy == was.flat.wave_lazy && F.lazy_objects == was.flat.lazy_objects && F.max_tlas_depth == was.flat.max_tlas_depth);
  EXPECT(F.nodes.size() == was.flat.nodes.size() && F.nodes.size() >= F.tlas_nodes);
  EXPECT(F.nodes.size() == F.tlas_nodes ||
         std::memcmp(F.nodes.data() + F.tlas_nodes, was.flat.nodes.data() + F.tlas_nodes, (F.nodes.size() - F.tlas_nodes) * sizeof(Node)) == 0);
  const float big = std::numeric_limits<float>::max();
  size_t rec = 0;
  for (size_t n = t.nodes.size(); n-- > 0;) {
    const HostNode& h = t.nodes[n];
    EXPECT(h.start == was.tlas.nodes[n].start && h.size == was.tlas.nodes[n].size && h.l == was.tlas.nodes[n].l && h.r == was.tlas.nodes[n].r);
    float mn[3] = {big, big, big}, mx[3] = {-big, -big, -big};
    if (h.l == h.r) {
      EXPECT(h.size <= 1u);
      for (uint32_t k = h.start; k < h.start + h.size; k++) {
        Mat4 it;
        uint32_t has = 0;
        float box[6];
        posed_values(all[t.prim[k]], &S.local_boxes[6 * (size_t)t.prim[k]], &it, &has, box);
        for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], box[a]); mx[a] = std::max(mx[a], box[3 + a]); }
      }
    } else {
      for (int a = 0; a < 3; a++) { mn[a] = std::min(std::min(mn[a], t.nodes[h.l].mn[a]), t.nodes[h.r].mn[a]); mx[a] = std::max(std::max(mx[a], t.nodes[h.l].mx[a]), t.nodes[h.r].mx[a]); }
    }
    EXPECT(std::memcmp(h.mn, mn, 12) == 0 && std::memcmp(h.mx, mx, 12) == 0);
    const Node& f = F.nodes[n];
    EXPECT(std::memcmp(f.mn, h.mn, 12) == 0 && std::memcmp(f.mx, h.mx, 12) == 0);
    EXPECT(h.l == h.r ? (f.left == h.start && f.count == (LEAF_BIT | h.size)) : (f.left == h.l && f.count == 0));
  }
  for (const HostNode& h : t.nodes) {
    if (h.l == h.r) continue;
    const WaveInterior& w = F.wave_tlas[rec];
    EXPECT(std::memcmp(w.boxl, t.nodes[h.l].mn, 24) == 0 && std::memcmp(w.boxr, t.nodes[h.r].mn, 24) == 0);
    EXPECT(w.l_ref == was.flat.wave_tlas[rec].l_ref && w.r_ref == was.flat.wave_tlas[rec].r_ref && w.l_cnt == t.nodes[h.l].size && w.r_cnt == t.nodes[h.r].size);
    rec++;
  }
  EXPECT(rec == F.wave_tlas.size());
  // every record: the Object ctor's values of its object's transform, everything else as committed
  for (size_t s = 0; s < F.objects.size(); s++) {
    const Object& o = F.objects[s];
    Object c = was.flat.objects[s];
    float box[6];
    c.trans = all[o.id - 1u];
    posed_values(c.trans, &S.local_boxes[6 * (size_t)(o.id - 1u)], &c.itrans, &c.has_trans, box);
    EXPECT(std::memcmp(&o, &c, sizeof(Object)) == 0);
    EXPECT(std::memcmp(&S.inputs[o.id - 1u].trans, &c.trans, sizeof(Mat4)) == 0);
  }
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
    S.dynamic_lights = true;                             // listed lights, if the file lists any, take new records
    EXPECT(build_scene(inputs, mats, use_bvh != 0, &S).empty());
    const BuiltScene first = S;
    std::vector<Mat4> home(nobj), all(nobj);
    for (uint32_t i = 0; i < nobj; i++) home[i] = all[i] = inputs[i].trans;
    for (uint32_t k = 0; k < n; k++) all[listed[k]] = moved[k];
    // the committed poses give the committed scene back
    std::vector<Mat4> same(n);
    for (uint32_t k = 0; k < n; k++) same[k] = inputs[listed[k]].trans;
    TopRefit R;
    EXPECT(prepare_top_refit(S, listed.data(), same.data(), n, &R).empty());
    EXPECT(same_posed_scene(S, first));                        // preparing leaves the scene alone
    apply_top_refit(&S, &R);
    EXPECT(same_posed_scene(S, first));
    // the new poses
    EXPECT(prepare_top_refit(S, listed.data(), moved.data(), n, &R).empty());
    EXPECT(R.boxes.size() == (use_bvh ? 6 * S.tlas.nodes.size() : 0));
    apply_top_refit(&S, &R);
    check_refitted(S, all, first);
    if (use_bvh) EXPECT(!same_bytes(S.tlas.nodes, first.tlas.nodes) && tree_cost(S.tlas) > 0.0);
    // the settle path: the records by insertion index and the node boxes, as read back, applied to a scene that lags two calls
    {
      BuiltScene L = first;
      L.dynamic_lights = true;
      std::vector<Object> by_index(nobj);
      for (const Object& o : S.flat.objects) by_index[o.id - 1u] = o;
      TopRefit Q;
      std::vector<uint32_t> pending(listed);
      pending.insert(pending.end(), listed.begin(), listed.end());     // two calls with the same list: every object once
      std::vector<bool> seen(nobj, false);
      for (uint32_t i : pending) {
        if (seen[i]) continue;
        seen[i] = true;
        Q.listed.push_back(i);
        Q.trans.push_back(by_index[i].trans); Q.itrans.push_back(by_index[i].itrans); Q.has_trans.push_back(by_index[i].has_trans);
      }
      if (use_bvh)
        for (const HostNode& h : S.tlas.nodes) { Q.boxes.insert(Q.boxes.end(), h.mn, h.mn + 3); Q.boxes.insert(Q.boxes.end(), h.mx, h.mx + 3); }
      apply_top_refit(&L, &Q);
      EXPECT(same_posed_scene(L, S));
    }
    // a rebuild of the same poses is a fresh build's; refitting the rebuilt tree with its own poses changes nothing
    {
      BuiltScene B = S, fresh;
      ReposedTop top;
      bool bad = true;
      EXPECT(prepare_repose(B, listed.data(), moved.data(), n, &top, &bad).empty() && !bad);
      apply_repose(&B, &top);
      std::vector<ObjectInput> posed_inputs = inputs;
      for (uint32_t i = 0; i < nobj; i++) posed_inputs[i].trans = all[i];
      fresh.dynamic_lights = true;
      EXPECT(build_scene(posed_inputs, mats, use_bvh != 0, &fresh).empty());
      EXPECT(same_posed_scene(B, fresh));
      EXPECT(prepare_top_refit(B, listed.data(), moved.data(), n, &R).empty());
      apply_top_refit(&B, &R);
      EXPECT(same_posed_scene(B, fresh));
      if (use_bvh) EXPECT(tree_cost(B.tlas) == tree_cost(fresh.tlas));
    }
    // and home again
    EXPECT(prepare_top_refit(S, listed.data(), same.data(), n, &R).empty());
    apply_top_refit(&S, &R);
    EXPECT(same_posed_scene(S, first));
    // refused lists leave the scene alone: a duplicate, out of range, an area light without the switch
    const BuiltScene before = S;
    std::vector<uint32_t> dup(listed);
    dup[n - 1] = dup[0];
    EXPECT(n < 2 || prepare_top_refit(S, dup.data(), moved.data(), n, &R).find("listed twice") != std::string::npos);
    std::vector<uint32_t> range(listed);
    range[0] = nobj;
    EXPECT(prepare_top_refit(S, range.data(), moved.data(), n, &R).find("out of range") != std::string::npos);
    S.dynamic_lights = false;
    for (uint32_t i = 0; i < nobj; i++)
      if (inputs[i].is_light) {
        const Mat4 m = inputs[i].trans;
        EXPECT(prepare_top_refit(S, &i, &m, 1, &R).find("area light") != std::string::npos);
        EXPECT(prepare_top_refit(S, &i, &m, 1, &R) == check_repose_list(S, &i, 1));
        break;
      }
    S.dynamic_lights = true;
    EXPECT(same_posed_scene(S, before));
    // non-finite matrices are not refused: the scene takes what the definition computes
    {
      BuiltScene C = S;
      Mat4 nan = moved[0];
      nan.c[1][1] = std::numeric_limits<float>::quiet_NaN();
      Mat4 singular = mat_identity();
      singular.c[2][2] = 0.0f;
      const uint32_t two[2] = {listed[0], listed[n - 1]};
      const Mat4 T2[2] = {nan, singular};
      EXPECT(prepare_top_refit(C, two, T2, n > 1 ? 2 : 1, &R).empty());
      apply_top_refit(&C, &R);
      EXPECT(C.tlas.prim == first.tlas.prim && C.tlas.nodes.size() == first.tlas.nodes.size());
    }
  }
  if (failures) return 1;
  std::printf("repose_refit_sanitized: ok (%u objects, %u listed)\n", nobj, n);
  return 0;
}
