// skin_ref.cpp - the reference's own Skeleton::find_joints / Skeleton::skin / Scene_Object::sync_anim_mesh run on a rig the caller
// describes, for tests/golden/make_skin_golden.py to record (tests/golden/skin_*.npz: data only).
//
// INTEGRATION HARNESS, part of integration/_build/libdropin_pt_full.so, where student/skeleton.cpp, scene/skeleton.cpp and
// scene/object.cpp are compiled where they lie.  Nothing of the product runs here: a Scene_Object gets an armature through
// Skeleton::add_root / add_child, Joint::pose / extent / radius and Skeleton::base(), posed_mesh() is called for both settings of
// opt.smooth_normals, and everything a test needs comes back in Skeleton::for_joints order - which, children being an
// unordered_set of pointers, is the reference's to decide and is therefore part of what is recorded.
#include <cstdint>
#include <vector>

#include "scene/object.h"
#include "scene/skeleton.h"

extern "C" {

// Joints: parent[j] (-1: a root; parents come before children), extent3, radius, pose3 (Euler angles in degrees), in the
// caller's order.  Out, all in for_joints order: order[k] = the caller's index of the k-th joint visited; bind / posed =
// Skeleton::joint_to_bind / joint_to_posed, 16 floats each; off[nverts + 1], jidx[..] = vertex_joints as indices (jcap: what jidx
// holds); and posed_mesh()'s vertices with smooth_normals (skin alone) and without (the flat-normal loop).
// Returns the number of influences, or -1 when jcap is too small or a joint was not visited.
__attribute__((visibility("default")))
long dropin_skin_reference(const float* pos, const float* nrm, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const int32_t* parent,
                           const float* extent3, const float* radius, const float* pose3, uint32_t njoints, const float* base3, uint32_t* order,
                           float* bind, float* posed, uint32_t* off, uint32_t* jidx, uint32_t jcap, float* smooth_pos, float* smooth_nrm,
                           float* flat_pos, float* flat_nrm) {
  std::vector<GL::Mesh::Vert> verts(nverts);
  for (uint32_t v = 0; v < nverts; v++)
    verts[v] = {Vec3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]), Vec3(nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]), 0};
  std::vector<GL::Mesh::Index> indices(idx, idx + nidx);
  Scene_Object obj(1, Pose::id(), GL::Mesh(std::move(verts), std::move(indices)));
  Skeleton& sk = obj.armature;
  sk.base() = Vec3(base3[0], base3[1], base3[2]);
  std::vector<Joint*> made(njoints, nullptr);
  for (uint32_t j = 0; j < njoints; j++) {
    const Vec3 e(extent3[3 * j], extent3[3 * j + 1], extent3[3 * j + 2]);
    made[j] = parent[j] < 0 ? sk.add_root(e) : sk.add_child(made[parent[j]], e);
    made[j]->radius = radius[j];
    made[j]->pose = Vec3(pose3[3 * j], pose3[3 * j + 1], pose3[3 * j + 2]);
  }
  std::vector<Joint*> visited;
  sk.for_joints([&](Joint* j) { visited.push_back(j); });
  if (visited.size() != njoints) return -1;
  auto index_of = [&](const std::vector<Joint*>& list, const Joint* j) {
    for (uint32_t k = 0; k < list.size(); k++) if (list[k] == j) return k;
    return (uint32_t)list.size();
  };
  for (uint32_t k = 0; k < njoints; k++) {
    order[k] = index_of(made, visited[k]);
    const Mat4 b = sk.joint_to_bind(visited[k]), p = sk.joint_to_posed(visited[k]);
    for (int i = 0; i < 16; i++) { bind[16 * k + i] = b.data[i]; posed[16 * k + i] = p.data[i]; }
  }
  auto take = [&](bool smooth, float* out_pos, float* out_nrm) {
    obj.opt.smooth_normals = smooth;
    obj.set_skel_dirty();
    obj.set_pose_dirty();
    const GL::Mesh& m = obj.posed_mesh();
    for (uint32_t v = 0; v < nverts; v++) {
      const GL::Mesh::Vert& x = m.verts()[v];
      out_pos[3 * v] = x.pos.x; out_pos[3 * v + 1] = x.pos.y; out_pos[3 * v + 2] = x.pos.z;
      out_nrm[3 * v] = x.norm.x; out_nrm[3 * v + 1] = x.norm.y; out_nrm[3 * v + 2] = x.norm.z;
    }
  };
  take(true, smooth_pos, smooth_nrm);
  take(false, flat_pos, flat_nrm);
  long n = 0;
  for (uint32_t v = 0; v < nverts; v++) {
    off[v] = (uint32_t)n;
    for (const Joint* j : obj.vertex_joints[v]) {
      if ((uint32_t)n >= jcap) return -1;
      jidx[n++] = index_of(visited, j);
    }
  }
  off[nverts] = (uint32_t)n;
  return n;
}

}  // extern "C"
