// anim_ref.cpp - the reference's own Animate-mode timeline (Anim_Pose::at, Pose::transform, Skeleton::set_time, Joint::joint_to_posed,
// Scene_Object::posed_mesh) run on keys the caller describes, for tests/golden/make_anim_golden.py to record
// (tests/golden/anim_*.npz: data only).
//
// INTEGRATION HARNESS, part of integration/_build/libdropin_pt_full.so, where scene/pose.cpp, scene/skeleton.cpp, student/skeleton.cpp
// and scene/object.cpp are compiled where they lie.  Nothing of the product runs here.  The library is built with
// -fno-access-control, so the knots go straight into the splines' maps: any quaternion can be stored, unit or not, which
// Anim_Pose::set (through Quat::euler) would not allow.
#include <cstdint>
#include <vector>

#include "scene/object.h"
#include "scene/pose.h"
#include "scene/skeleton.h"

extern "C" {

// One Anim_Pose.  offsets[4]: the knots of the position, rotation and scale tracks are [offsets[i], offsets[i + 1]) of times /
// values (4 floats per knot: xyz_ or xyzw).  Out, per requested time: pose9 = Anim_Pose::at(t) as {pos, euler, scale} and trans16 =
// that pose's Pose::transform() in Mat4::data order.
__attribute__((visibility("default")))
void dropin_anim_pose_reference(const uint32_t* offsets, const float* times, const float* values, const float* ts, uint32_t nt, float* pose9, float* trans16) {
  Anim_Pose anim;
  for (uint32_t k = offsets[0]; k < offsets[1]; k++) anim.splines.head.control_points[times[k]] = Vec3(values[4 * k], values[4 * k + 1], values[4 * k + 2]);
  for (uint32_t k = offsets[1]; k < offsets[2]; k++)
    anim.splines.tail.head.values[times[k]] = Quat(values[4 * k], values[4 * k + 1], values[4 * k + 2], values[4 * k + 3]);
  for (uint32_t k = offsets[2]; k < offsets[3]; k++) anim.splines.tail.tail.head.control_points[times[k]] = Vec3(values[4 * k], values[4 * k + 1], values[4 * k + 2]);
  for (uint32_t i = 0; i < nt; i++) {
    const Pose p = anim.at(ts[i]);
    const float nine[9] = {p.pos.x, p.pos.y, p.pos.z, p.euler.x, p.euler.y, p.euler.z, p.scale.x, p.scale.y, p.scale.z};
    for (int a = 0; a < 9; a++) pose9[9 * i + a] = nine[a];
    const Mat4 m = p.transform();
    for (int a = 0; a < 16; a++) trans16[16 * i + a] = m.data[a];
  }
}

// A rig as harness/skin_ref.cpp builds it (parent[j]: -1 a root, parents first; extent3, radius; base3), with rest_pose3 in
// Joint::pose and the knots [knot_offsets[j], knot_offsets[j + 1]) of times / quats (xyzw) in Joint::anim, in the caller's order.
// Out: order[k] = the caller's index of the k-th joint Skeleton::for_joints visits; then per requested time, after
// Skeleton::set_time(t), in for_joints order: euler3 = Joint::pose, posed16 = Skeleton::joint_to_posed; and posed_mesh()'s vertices
// with smooth normals (Skeleton::skin alone).  Returns 0, or -1 when a joint was not visited.
__attribute__((visibility("default")))
int dropin_anim_rig_reference(const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const int32_t* parent,
                              const float* extent3, const float* radius, const float* rest_pose3, uint32_t njoints, const float* base3,
                              const uint32_t* knot_offsets, const float* times, const float* quats, const float* ts, uint32_t nt, uint32_t* order,
                              float* euler3, float* posed16, float* mesh_pos) {
  std::vector<GL::Mesh::Vert> verts(nverts);
  for (uint32_t v = 0; v < nverts; v++)
    verts[v] = {Vec3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]), Vec3(nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]), 0};
  std::vector<GL::Mesh::Index> indices(idx, idx + nidx);
  Scene_Object obj(1, Pose::id(), GL::Mesh(std::move(verts), std::move(indices)));
  obj.opt.smooth_normals = true;
  Skeleton& sk = obj.armature;
  sk.base() = Vec3(base3[0], base3[1], base3[2]);
  std::vector<Joint*> made(njoints, nullptr);
  for (uint32_t j = 0; j < njoints; j++) {
    const Vec3 e(extent3[3 * j], extent3[3 * j + 1], extent3[3 * j + 2]);
    made[j] = parent[j] < 0 ? sk.add_root(e) : sk.add_child(made[parent[j]], e);
    made[j]->radius = radius[j];
  }
  // (the keys go in once the hierarchy stands: add_root / add_child give a new joint a Quat{} key at every time the skeleton has keys at)
  for (uint32_t j = 0; j < njoints; j++) {
    made[j]->pose = Vec3(rest_pose3[3 * j], rest_pose3[3 * j + 1], rest_pose3[3 * j + 2]);
    for (uint32_t k = knot_offsets[j]; k < knot_offsets[j + 1]; k++)
      made[j]->anim.values[times[k]] = Quat(quats[4 * k], quats[4 * k + 1], quats[4 * k + 2], quats[4 * k + 3]);
  }
  std::vector<Joint*> visited;
  sk.for_joints([&](Joint* j) { visited.push_back(j); });
  if (visited.size() != njoints) return -1;
  for (uint32_t k = 0; k < njoints; k++) {
    order[k] = njoints;
    for (uint32_t j = 0; j < njoints; j++)
      if (made[j] == visited[k]) order[k] = j;
  }
  for (uint32_t i = 0; i < nt; i++) {
    sk.set_time(ts[i]);
    obj.set_skel_dirty();
    obj.set_pose_dirty();
    for (uint32_t k = 0; k < njoints; k++) {
      const Vec3 e = visited[k]->pose;
      float* e3 = euler3 + 3 * ((size_t)i * njoints + k);
      e3[0] = e.x; e3[1] = e.y; e3[2] = e.z;
      const Mat4 p = sk.joint_to_posed(visited[k]);
      for (int a = 0; a < 16; a++) posed16[16 * ((size_t)i * njoints + k) + a] = p.data[a];
    }
    const GL::Mesh& m = obj.posed_mesh();
    for (uint32_t v = 0; v < nverts; v++) {
      const GL::Mesh::Vert& x = m.verts()[v];
      float* o = mesh_pos + 3 * ((size_t)i * nverts + v);
      o[0] = x.pos.x; o[1] = x.pos.y; o[2] = x.pos.z;
    }
  }
  return 0;
}

}  // extern "C"
