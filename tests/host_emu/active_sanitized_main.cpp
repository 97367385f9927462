// Stand-alone check of srt_pt_set_active's scene layer (pt_scene.cpp alone; tests/test_pt_active_host.py builds it with
// -fsanitize=address,undefined and runs it once) on the scene and the list of the file given as argv[1] (the format of
// scene_main_common.h:load_scene_file): the definition - check_active_list / apply_set_active / mask_top - the fold of the effective
// boxes, the empty-node rule of tree_cost, the rebuild and refit paths while objects are hidden, and the settle bookkeeping (the
// table and the boxes applied as srt_pt_set_active_device's read-back delivers them).
#include <algorithm>
#include <limits>

#include "scene_main_common.h"

static bool same_links(const HostBVH& a, const HostBVH& b) {
  if (a.prim != b.prim || a.nodes.size() != b.nodes.size()) return false;
  for (size_t n = 0; n < a.nodes.size(); n++)
    if (a.nodes[n].start != b.nodes[n].start || a.nodes[n].size != b.nodes[n].size || a.nodes[n].l != b.nodes[n].l || a.nodes[n].r != b.nodes[n].r) return false;
  return true;
}

static bool empty_box(const float mn[3], const float mx[3]) { return mn[0] > mx[0] || mn[1] > mx[1] || mn[2] > mx[2]; }

// What a node holds for the walks: an interior node and a leaf with an active object their size, a leaf with none 0.
static uint32_t held(const BuiltScene& S, const HostNode& h) {
  if (h.l != h.r) return h.size;
  for (uint32_t k = h.start; k < h.start + h.size; k++)
    if (S.active[S.tlas.prim[k]]) return h.size;
  return 0;
}

// The top of S against the definition: every node box the fold of the effective boxes, restated here; the flattened nodes and the
// sweep records say what the host tree says; the cost counts what is not empty.
static void check_masked(const BuiltScene& S) {
  const HostBVH& t = S.tlas;
  const FlatScene& F = S.flat;
  const float big = std::numeric_limits<float>::max();
  for (size_t n = t.nodes.size(); n-- > 0;) {
    const HostNode& h = t.nodes[n];
    float mn[3] = {big, big, big}, mx[3] = {-big, -big, -big};
    if (h.l == h.r) {
      for (uint32_t k = h.start; k < h.start + h.size; k++) {
        if (!S.active[t.prim[k]]) continue;
        Mat4 it;
        uint32_t has = 0;
        float box[6];
        posed_values(S.inputs[t.prim[k]].trans, &S.local_boxes[6 * (size_t)t.prim[k]], &it, &has, box);
        for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], box[a]); mx[a] = std::max(mx[a], box[3 + a]); }
      }
    } else {
      for (int a = 0; a < 3; a++) { mn[a] = std::min(std::min(mn[a], t.nodes[h.l].mn[a]), t.nodes[h.r].mn[a]); mx[a] = std::max(std::max(mx[a], t.nodes[h.l].mx[a]), t.nodes[h.r].mx[a]); }
    }
    EXPECT(std::memcmp(h.mn, mn, 12) == 0 && std::memcmp(h.mx, mx, 12) == 0);
    const Node& f = F.nodes[n];
    EXPECT(std::memcmp(f.mn, h.mn, 12) == 0 && std::memcmp(f.mx, h.mx, 12) == 0);
    // a leaf whose objects are all inactive holds nothing for the walks; the host tree keeps its size
    EXPECT(h.l == h.r ? (f.left == h.start && f.count == (LEAF_BIT | held(S, h))) : (f.left == h.l && f.count == 0));
  }
  size_t rec = 0;
  for (const HostNode& h : t.nodes) {
    if (h.l == h.r) continue;
    const WaveInterior& w = F.wave_tlas[rec++];
    EXPECT(std::memcmp(w.boxl, t.nodes[h.l].mn, 24) == 0 && std::memcmp(w.boxr, t.nodes[h.r].mn, 24) == 0);
    EXPECT(w.l_cnt == held(S, t.nodes[h.l]) && w.r_cnt == held(S, t.nodes[h.r]));
  }
  EXPECT(rec == F.wave_tlas.size());
  // tree_cost with the empty-node rule, restated
  auto area = [](const HostNode& h) {
    if (empty_box(h.mn, h.mx)) return 0.0;
    const double x = (double)h.mx[0] - h.mn[0], y = (double)h.mx[1] - h.mn[1], z = (double)h.mx[2] - h.mn[2];
    return 2.0 * (x * y + y * z + z * x);
  };
  double cost = 0.0;
  if (!empty_box(t.nodes[0].mn, t.nodes[0].mx))
    for (const HostNode& h : t.nodes) cost += (h.l == h.r ? (double)h.size : 1.0) * (area(h) / area(t.nodes[0]));
  EXPECT(tree_cost(t) == cost);
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s scene-file\n", argv[0]); return 2; }
  std::vector<Material> mats;
  std::vector<ObjectInput> inputs;
  std::vector<uint32_t> listed;
  std::vector<Mat4> moved;
  const bool read = load_scene_file(argv[1], &mats, &inputs, &listed, &moved);
  const uint32_t n = (uint32_t)listed.size();
  if (!read || inputs.size() < 2 || n < 2) { std::printf("cannot read %s\n", argv[1]); return 2; }
  const uint32_t nobj = (uint32_t)inputs.size();

  BuiltScene S;
  EXPECT(build_scene(inputs, mats, true, &S).empty());
  const BuiltScene first = S;
  EXPECT(S.active.size() == nobj && !any_inactive(S));
  check_masked(S);                                        // every object active: the committed boxes are the fold's
  bool unsupported = true;
  EXPECT(check_active_list(S, listed.data(), n, &unsupported).empty() && !unsupported);

  // every other listed object off; a call that changes nothing writes nothing
  std::vector<uint8_t> flags(n), ones(n, 1);
  for (uint32_t k = 0; k < n; k++) flags[k] = (k & 1u) ? 7 : 0;
  EXPECT(!apply_set_active(&S, listed.data(), ones.data(), n) && same_posed_scene(S, first));
  EXPECT(apply_set_active(&S, listed.data(), flags.data(), n));
  EXPECT(!apply_set_active(&S, listed.data(), flags.data(), n));
  for (uint32_t k = 0; k < n; k++) EXPECT(S.active[listed[k]] == ((k & 1u) ? 1 : 0));
  EXPECT(any_inactive(S) && same_links(S.tlas, first.tlas) && same_bytes(S.flat.objects, first.flat.objects));
  EXPECT(!same_bytes(S.tlas.nodes, first.tlas.nodes));
  check_masked(S);
  const BuiltScene masked = S;

  // a refit and a rebuild while objects are hidden: the flags persist, the topology is the all-active call's, the boxes the masked fold
  {
    TopRefit T;
    EXPECT(prepare_top_refit(S, listed.data(), moved.data(), n, &T).empty());
    EXPECT(same_posed_scene(S, masked));
    apply_top_refit(&S, &T);
    EXPECT(S.active == masked.active && same_links(S.tlas, first.tlas));
    check_masked(S);
    BuiltScene A = first;                                 // the same rebuild with every object active
    ReposedTop top, top_a;
    bool bad = true;
    EXPECT(prepare_repose(S, listed.data(), moved.data(), n, &top, &bad).empty() && !bad);
    EXPECT(prepare_repose(A, listed.data(), moved.data(), n, &top_a, &bad).empty() && !bad);
    apply_repose(&S, &top);
    apply_repose(&A, &top_a);
    EXPECT(S.active == masked.active && same_links(S.tlas, A.tlas) && same_bytes(S.flat.objects, A.flat.objects));
    check_masked(S);
    check_masked(A);
    // everything on again: the hidden objects sit where they were moved to
    EXPECT(apply_set_active(&S, listed.data(), ones.data(), n) && !any_inactive(S));
    for (size_t k = 0; k < S.tlas.nodes.size(); k++)
      for (int a = 0; a < 3; a++) EXPECT(S.tlas.nodes[k].mn[a] == A.tlas.nodes[k].mn[a] && S.tlas.nodes[k].mx[a] == A.tlas.nodes[k].mx[a]);
    EXPECT(tree_cost(S.tlas) == tree_cost(A.tlas));
  }

  // the settle bookkeeping: a record that lags takes the table and the boxes as they are read back
  {
    BuiltScene L = first;
    TopRefit Q;
    for (const HostNode& h : masked.tlas.nodes) { Q.boxes.insert(Q.boxes.end(), h.mn, h.mn + 3); Q.boxes.insert(Q.boxes.end(), h.mx, h.mx + 3); }
    std::vector<uint8_t> table(masked.active);
    L.active.swap(table);
    apply_top_refit(&L, &Q);
    write_top_counts(&L);                                 // (what settle() does behind a srt_pt_set_active_device call)
    EXPECT(same_posed_scene(L, masked));
  }

  // every object that may be hidden hidden: the root is empty and the cost 0 only when nothing is left
  {
    BuiltScene E = first;
    std::vector<uint32_t> all;
    for (uint32_t i = 0; i < nobj; i++)
      if (!inputs[i].is_light) all.push_back(i);
    std::vector<uint8_t> zeros(all.size(), 0);
    EXPECT(check_active_list(E, all.data(), (uint32_t)all.size(), &unsupported).empty());
    EXPECT(apply_set_active(&E, all.data(), zeros.data(), (uint32_t)all.size()));
    check_masked(E);
    if (all.size() == nobj) EXPECT(tree_cost(E.tlas) == 0.0 && empty_box(E.tlas.nodes[0].mn, E.tlas.nodes[0].mx));
    else EXPECT(tree_cost(E.tlas) > 0.0);
  }

  // refusals leave the scene alone
  {
    S = masked;
    std::vector<uint32_t> dup(listed);
    dup[n - 1] = dup[0];
    EXPECT(check_active_list(S, dup.data(), n, &unsupported).find("listed twice") != std::string::npos && !unsupported);
    std::vector<uint32_t> range(listed);
    range[0] = nobj;
    EXPECT(check_active_list(S, range.data(), n, &unsupported).find("out of range") != std::string::npos && !unsupported);
    for (int dynamic = 0; dynamic < 2; dynamic++) {
      S.dynamic_lights = dynamic != 0;
      for (uint32_t i = 0; i < nobj; i++)
        if (inputs[i].is_light) { EXPECT(check_active_list(S, &i, 1, &unsupported).find("area light") != std::string::npos && !unsupported); break; }
    }
    S.dynamic_lights = false;
    EXPECT(same_posed_scene(S, masked));
    BuiltScene list_scene, one;
    EXPECT(build_scene(inputs, mats, false, &list_scene).empty());
    EXPECT(!check_active_list(list_scene, listed.data(), n, &unsupported).empty() && unsupported);
    std::vector<ObjectInput> single;
    for (const ObjectInput& o : inputs)
      if (o.source < 0 && !o.is_light) { single.push_back(o); break; }
    EXPECT(build_scene(single, mats, true, &one).empty());
    const uint32_t zero = 0;
    EXPECT(!check_active_list(one, &zero, 1, &unsupported).empty() && unsupported);
  }
  if (failures) return 1;
  std::printf("active_sanitized: ok (%u objects, %u listed)\n", nobj, n);
  return 0;
}
