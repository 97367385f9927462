// ik_ref.cpp - the reference's own Skeleton::set_time, Skeleton::do_ik / step_ik / Joint::compute_gradient, Skeleton::joint_to_posed and
// Scene_Object::posed_mesh run on a rig, handles and targets the caller describes, for tests/golden/make_ik_golden.py to record
// (tests/golden/ik_*.npz: data only).
//
// INTEGRATION HARNESS, part of integration/_build/libdropin_pt_full.so, where scene/skeleton.cpp, student/skeleton.cpp and
// scene/object.cpp are compiled where they lie.  Nothing of the product runs here.  The library is built with
// -fno-access-control, so the handles go straight into Skeleton::handles with the target as given (Skeleton::add_handle would
// subtract base_pos) and `target` / `enabled` are set per call, as Skeleton::set_time does from a handle's keys.
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "scene/object.h"
#include "scene/pose.h"
#include "scene/skeleton.h"

extern "C" {

// A rig as harness/anim_ref.cpp builds it (parent[j]: -1 a root, parents first; extent3, radius; base3; rest_pose3 in Joint::pose; the
// knots [knot_offsets[j], knot_offsets[j + 1]) of times / quats in Joint::anim), with a mesh (nverts > 0) or without, and nhandles
// handles on handle_joint[h] (the caller's joint indices).  Then ncalls times: set_times[c], unless NaN, through Skeleton::set_time;
// target and enabled of every handle from targets[c][h] / enabled[c][h]; Skeleton::do_ik().
// Out: order[k] = the caller's index of the k-th joint Skeleton::for_joints visits; handle_order[k] = the caller's index of the k-th
// handle `handles` iterates over - the order do_ik collects them in; pose_before[c][k] / pose_out[c][k] = Joint::pose before do_ik
// (after set_time) and after it in call c, in for_joints order;
// did[c] = what do_ik returned; after the last call posed16[k] = Skeleton::joint_to_posed and, with a mesh, posed_mesh()'s vertices
// (smooth normals: Skeleton::skin alone).  Returns 0, or -1 when a joint or a handle was not visited.
__attribute__((visibility("default")))
int dropin_ik_reference(const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const int32_t* parent,
                        const float* extent3, const float* radius, const float* rest_pose3, uint32_t njoints, const float* base3,
                        const uint32_t* knot_offsets, const float* times, const float* quats, const uint32_t* handle_joint, uint32_t nhandles,
                        const float* targets, const uint8_t* enabled, const float* set_times, uint32_t ncalls, uint32_t* order, uint32_t* handle_order,
                        float* pose_before, float* pose_out, uint8_t* did, float* posed16, float* mesh_pos) {
  std::unique_ptr<Scene_Object> obj;
  std::unique_ptr<Skeleton> bare;
  if (nverts) {
    std::vector<GL::Mesh::Vert> verts(nverts);
    for (uint32_t v = 0; v < nverts; v++)
      verts[v] = {Vec3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]), Vec3(nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]), 0};
    std::vector<GL::Mesh::Index> indices(idx, idx + nidx);
    obj.reset(new Scene_Object(1, Pose::id(), GL::Mesh(std::move(verts), std::move(indices))));
    obj->opt.smooth_normals = true;
  } else {
    bare.reset(new Skeleton(1));
  }
  Skeleton& sk = obj ? obj->armature : *bare;
  sk.base() = Vec3(base3[0], base3[1], base3[2]);
  std::vector<Joint*> made(njoints, nullptr);
  for (uint32_t j = 0; j < njoints; j++) {
    const Vec3 e(extent3[3 * j], extent3[3 * j + 1], extent3[3 * j + 2]);
    made[j] = parent[j] < 0 ? sk.add_root(e) : sk.add_child(made[parent[j]], e);
    made[j]->radius = radius[j];
  }
  for (uint32_t j = 0; j < njoints; j++) {
    made[j]->pose = Vec3(rest_pose3[3 * j], rest_pose3[3 * j + 1], rest_pose3[3 * j + 2]);
    for (uint32_t k = knot_offsets[j]; k < knot_offsets[j + 1]; k++)
      made[j]->anim.values[times[k]] = Quat(quats[4 * k], quats[4 * k + 1], quats[4 * k + 2], quats[4 * k + 3]);
  }
  std::vector<Skeleton::IK_Handle*> hmade(nhandles, nullptr);
  for (uint32_t h = 0; h < nhandles; h++) {
    hmade[h] = new Skeleton::IK_Handle{Vec3(), made[handle_joint[h]], {}, false, sk.next_id++};
    sk.handles.insert(hmade[h]);                                     // (the skeleton's destructor deletes them)
  }
  std::vector<Joint*> visited;
  sk.for_joints([&](Joint* j) { visited.push_back(j); });
  if (visited.size() != njoints) return -1;
  for (uint32_t k = 0; k < njoints; k++) {
    order[k] = njoints;
    for (uint32_t j = 0; j < njoints; j++)
      if (made[j] == visited[k]) order[k] = j;
  }
  uint32_t seen = 0;
  for (Skeleton::IK_Handle* h : sk.handles) {
    if (seen >= nhandles) return -1;
    handle_order[seen] = nhandles;
    for (uint32_t i = 0; i < nhandles; i++)
      if (hmade[i] == h) handle_order[seen] = i;
    seen++;
  }
  if (seen != nhandles) return -1;
  for (uint32_t c = 0; c < ncalls; c++) {
    if (!std::isnan(set_times[c])) sk.set_time(set_times[c]);
    for (uint32_t h = 0; h < nhandles; h++) {
      const float* t = targets + 3 * ((size_t)c * nhandles + h);
      hmade[h]->target = Vec3(t[0], t[1], t[2]);
      hmade[h]->enabled = enabled[(size_t)c * nhandles + h] != 0;
    }
    for (int after = 0; after < 2; after++) {
      if (after) did[c] = sk.do_ik() ? 1 : 0;
      for (uint32_t k = 0; k < njoints; k++) {
        const Vec3 e = visited[k]->pose;
        float* e3 = (after ? pose_out : pose_before) + 3 * ((size_t)c * njoints + k);
        e3[0] = e.x; e3[1] = e.y; e3[2] = e.z;
      }
    }
  }
  for (uint32_t k = 0; k < njoints; k++) {
    const Mat4 p = sk.joint_to_posed(visited[k]);
    for (int a = 0; a < 16; a++) posed16[16 * (size_t)k + a] = p.data[a];
  }
  if (obj) {
    obj->set_skel_dirty();
    obj->set_pose_dirty();
    const GL::Mesh& m = obj->posed_mesh();
    for (uint32_t v = 0; v < nverts; v++) {
      const GL::Mesh::Vert& x = m.verts()[v];
      mesh_pos[3 * (size_t)v] = x.pos.x; mesh_pos[3 * (size_t)v + 1] = x.pos.y; mesh_pos[3 * (size_t)v + 2] = x.pos.z;
    }
  }
  return 0;
}

}  // extern "C"
