// Host-side scene assembly for the path tracer and the flattened layout the kernels read.
//
// build_scene of the reference (rays/pathtracer.cpp:66-176) creates, per scene object, an
// Object{trans, itrans = trans.inverse(), has_trans, material, Tri_Mesh | Shape}, builds a BVH<Triangle>
// (leaf size 4) per mesh and one BVH<Object> (leaf size 1) over all objects.  FlatScene is the same
// information laid out for the GPU:
//   nodes      32-byte nodes, TLAS first, then every BLAS; children of an interior node are adjacent
//              (the reference allocates them back to back, student/bvh.inl:144-145)
//   tris       48 B per triangle {p0, e1 = p1 - p0, e2 = p2 - p0}, stored in BVH primitive order so a leaf
//              is a contiguous run; e1/e2 are the same fp32 subtractions Triangle::hit performs per test
//   tri_nrm    48 B per triangle {n0, n1, n2}, read only for the winning triangle of an indirect/camera ray
//   objects    one record per object in BVH<Object> primitive order: transform pair + BLAS range
//   lights     the area-light copies (List<Object> of Tri_Mesh(.., use_bvh = false)) with the matrices
//              Object::pdf composes (T = I*trans, iT = itrans*I) and, per triangle, the sample corners and
//              the 2/|cross| factor of Triangle::pdf
#ifndef SRT_PT_SCENE_H
#define SRT_PT_SCENE_H

#include <cstdint>
#include <string>
#include <vector>

namespace srt {

constexpr uint32_t LEAF_BIT = 0x80000000u;

struct Mat4 { float c[4][4]; };  // c[col][row], Mat4::cols of the reference

struct Node {
  float mn[3];
  uint32_t left;   // interior: index of the left child (right = left + 1); leaf: first primitive
  float mx[3];
  uint32_t count;  // leaf: LEAF_BIT | number of primitives; interior: 0
};
static_assert(sizeof(Node) == 32, "node layout");

struct Tri { float p0[4], e1[4], e2[4]; };     // xyz + pad
struct TriNrm { float n0[4], n1[4], n2[4]; };
static_assert(sizeof(Tri) == 48 && sizeof(TriNrm) == 48, "triangle layout");

enum : uint32_t { OBJ_MESH = 0, OBJ_SPHERE = 1 };

struct Object {
  uint32_t kind, has_trans;
  int32_t material;
  uint32_t use_bvh;            // bit 0: the mesh was built with a BVH<Triangle>; bits 8..: ordinal among the meshes with nrec > 0
  uint32_t node_base, nnodes;  // BLAS nodes [node_base, node_base + nnodes)
  uint32_t tri_base, ntri;     // triangles [tri_base, tri_base + ntri)
  float radius;
  uint32_t id;                 // 1-based insertion index (diagnostics)
  uint32_t rec_base, nrec;     // BLAS interior records [rec_base, rec_base + nrec) in blas_recs; nrec == 0: the root is a leaf
  Mat4 trans, itrans;
};
static_assert(sizeof(Object) == 48 + 128, "object layout");

struct LightTri {
  float v0[4], v1[4], v2[4];   // object-space corners (Samplers::Triangle)
  float area_term;             // 2 / |cross(T*v1 - T*v0, T*v2 - T*v0)|  (Triangle::pdf)
  float pad[3];
};

struct Light {
  uint32_t has_trans, tri_base, ntri, pad;  // tri_base indexes tris / tri_nrm / light_tris alike
  Mat4 trans, itrans;  // Object::sample
  Mat4 pdfT, pdfiT;    // Object::pdf: T = I * trans, iT = itrans * I
};

// Delta_Light (rays/light.h:57-96): Directional / Point / Spot light with the object's pose.
enum : uint32_t { DL_DIRECTIONAL = 0, DL_POINT = 1, DL_SPOT = 2 };
struct DeltaLight {
  uint32_t type, has_trans;
  float radiance[3];
  float angle_bounds[2];     // spot only (degrees, Spot_Light::angle_bounds)
  float pad;
  Mat4 trans, itrans;
};
static_assert(sizeof(DeltaLight) == 32 + 128, "delta light layout");

struct Material {
  uint32_t type;
  float a[3], b[3];
  float ior;
};

// Top-level tree in the form the wave-uniform kernel sweeps: one record per INTERIOR node of the BVH<Object>,
// in node-index order (parents before children).  A child is either another interior node (ref = its rank in
// this array) or a leaf (ref = ~first object slot, cnt = number of objects in the leaf, 0 or 1).
struct WaveInterior {
  float boxl[6], boxr[6];   // mn.xyz, mx.xyz of the left / right child
  int32_t l_ref, r_ref;
  uint32_t l_cnt, r_cnt;
};
static_assert(sizeof(WaveInterior) == 64, "wave interior layout");

struct Camera {
  Mat4 iview;
  float vert_fov, aspect_ratio;
  float screen_h, screen_w;  // tanf(Radians(fov) / 2) * 1 * 2 and ar * that (student/camera.cpp:17-18), host libm
};

// Image-tile shard of one rank: tiles t with t % world == rank, numbered row-major.
struct TileMap { uint32_t tile_w, tile_h, tiles_x, tiles_y, rank, world, local_tiles; };

enum { C_RAYS = 0, C_BOX, C_OBJ, C_TRI, C_SPH, C_TLAS, C_BLAS, C_LTRI, C_COUNT };   // what the instrumented kernels count (Counters, pt_trace.h)

// What the host refuses at commit and at every update: trees deeper than the kernels' traversal stacks (pt_trace.h)
constexpr int kMaxTlasDepth = 24;   // interior-node nesting the traversal stacks can hold
constexpr int kMaxBlasDepth = 48;

struct FlatScene {
  bool use_bvh = true;
  std::vector<Node> nodes;        // [0, tlas_nodes) = BVH<Object>
  uint32_t tlas_nodes = 0;
  std::vector<Tri> tris;
  std::vector<TriNrm> tri_nrm;
  // The same records without their padding (nine floats: p0, e1, e2): what the streamed forms' cast kernel reads (pt_stream.h) - a big
  // mesh's triangles are most of what its walks miss their XCD's L2 with, and a leaf's <= 4 triangles are 144 bytes this way, 192 padded.
  std::vector<float> tri_packed;
  std::vector<Object> objects;    // BVH<Object> primitive order (insertion order when !use_bvh)
  std::vector<Light> lights;
  std::vector<LightTri> light_tris;  // indexed by (global triangle index - first light triangle)
  uint32_t light_tri_first = 0;
  std::vector<Material> materials;
  std::vector<DeltaLight> delta_lights;   // Pathtracer::point_lights, in insertion order
  uint32_t max_tlas_depth = 0, max_blas_depth = 0;  // interior-node nesting (stack frames needed)
  std::vector<WaveInterior> wave_tlas;              // empty when the root is a leaf (or in list mode)
  // Per-mesh BVH<Triangle> as interior records (both child boxes in one 64-byte fetch).  Child refs: >= 0 interior
  // rank inside the mesh's range; < 0 leaf, ~ref = (first triangle slot << 3) | triangle count (<= 4).
  std::vector<WaveInterior> blas_recs;
  std::vector<uint32_t> lazy_objects;               // object slots whose mesh has a real BVH<Triangle> (nrec > 0), by ordinal
  std::vector<uint32_t> wave_lazy;                  // per wave_tlas record: bit 0 / 1 = the left / right child's subtree holds such a mesh
};

// Input side (what the C ABI collects between scene_begin and scene_commit).
struct MeshInput {
  std::vector<float> pos, nrm;  // 3 per vertex
  std::vector<uint32_t> idx;    // 3 per triangle
};
struct ObjectInput {
  uint32_t kind = OBJ_MESH;
  Mat4 trans;
  uint32_t material = 0;
  bool is_light = false;
  float radius = 0.f;
  MeshInput mesh;
  // >= 0: an instance (srt_pt_add_instance) of the mesh object with this insertion index - Object(<its Tri_Mesh>.copy(), ..) of
  // rays/pathtracer.cpp:134-155 without the copy: `mesh` stays empty, the triangles and the BVH<Triangle> are the source's
  int32_t source = -1;
};

// Host BVH kept for srt_pt_dump_bvh (reference Node layout: bbox + start,size,l,r).
struct HostNode { float mn[3], mx[3]; uint32_t start, size, l, r; };
struct HostBVH { std::vector<HostNode> nodes; std::vector<uint32_t> prim; };

// Where a mesh lives in the flattened arrays.  BLAS nodes are counted from the end of the TLAS nodes (node_off), so that a
// re-posed scene, whose BVH<Object> may have another number of nodes, leaves them where they are.
struct MeshStore { uint32_t tri_base = 0, ntri = 0, node_off = 0, nnodes = 0, rec_base = 0, nrec = 0; };

struct BuiltScene {
  FlatScene flat;
  HostBVH tlas;                 // prim = object insertion indices
  std::vector<HostBVH> blas;    // per object in insertion order (empty for spheres / instances / list mode)
  std::vector<ObjectInput> inputs;
  std::vector<float> local_boxes;   // six floats per object in insertion order: the object-space box Object::bbox poses
  std::vector<MeshStore> store;     // per object in insertion order: an instance's is its source's
  uint64_t blas_builds = 0;         // BVH<Triangle> builds this build_scene performed (one per mesh that is not an instance)
  // srt_pt_set_dynamic_lights: check_repose_list / check_mesh_update admit area lights, and the apply_* functions keep the light
  // tables true (light_record, light_area_term, write_light_mesh below).  build_scene keeps the switch of the scene it replaces.
  bool dynamic_lights = false;
  // srt_pt_set_active: one byte per object in insertion order, 1 = active.  build_scene sets every one.  An inactive object keeps
  // its record and its posed box; only the box the BVH<Object> folds for it is BBox() (effective_boxes), which no ray without a
  // NaN component passes.  The topology never depends on the table: every build is over the posed boxes of all objects.
  std::vector<uint8_t> active;
};

// What srt_pt_repose derives for new poses of a committed scene, built next to it: the BVH<Object> and everything that follows
// from object order.  prepare_repose leaves `built` untouched; apply_repose moves the tables in (it cannot fail).
struct ReposedTop {
  std::vector<uint32_t> listed;     // insertion indices ..
  std::vector<Mat4> trans;          // .. and their new transforms
  HostBVH tlas;
  std::vector<Node> tlas_nodes;
  uint32_t max_tlas_depth = 0;
  std::vector<WaveInterior> wave_tlas;
  std::vector<uint32_t> wave_lazy, lazy_objects;
  std::vector<Object> objects;
};

// BVH<Primitive>::build for large primitive sets on the device (pt_bvh_device.hip; same arrays as the host build, bit for
// bit).  The hook keeps pt_scene.cpp free of HIP: build_scene uses `fn` for sets of at least `min_prims` primitives when one
// is installed (thread-local: a context installs its choice around its own build_scene call).
typedef bool (*DeviceBvhBuilder)(const float* boxes6, uint32_t n, uint32_t max_leaf, HostBVH* out);
void set_device_bvh_builder(DeviceBvhBuilder fn, uint32_t min_prims);
bool build_bvh_device(const float* boxes6, uint32_t n, uint32_t max_leaf, HostBVH* out);

Mat4 mat_identity();
Mat4 mat_inverse(const Mat4& m);   // Mat4::inverse, same term order (lib/mat4.h:296-343)
Mat4 mat_mul(const Mat4& self, const Mat4& m);  // self * m  (lib/mat4.h:110-121)
bool mat_ne_identity(const Mat4& m);

// Returns "" on success, otherwise an error message (e.g. the reference's non-terminating BVH build).
std::string build_scene(const std::vector<ObjectInput>& objects, const std::vector<Material>& materials, bool use_bvh,
                        BuiltScene* out);

// What build_scene computes per area light, factored out so that a re-posed or deformed light takes the values a fresh commit
// would give it.  light_record: has_trans, trans, itrans and Object::pdf's pair pdfT = I * trans, pdfiT = itrans * I (identities
// when !has_trans; rays/object.h:90-94) - tri_base / ntri / pad are left alone.  light_area_term: 2 / |cross(T v1 - T v0, T v2 - T v0)|
// of Triangle::pdf (student/tri_mesh.cpp:137), T applied as Mat4 * Vec3 with the perspective divide; a zero-area triangle gives inf.
// light_tri_record: the whole LightTri of triangle t of `mesh` (corners, zeroed padding, area term under pdfT).
void light_record(const Mat4& trans, const Mat4& itrans, bool has_trans, Light* L);
float light_area_term(const Mat4& pdfT, const float v0[3], const float v1[3], const float v2[3]);
LightTri light_tri_record(const Mat4& pdfT, const MeshInput& mesh, uint32_t t);
// The index of object `object` (insertion index) in FlatScene::lights, -1 when it has no light record.
int32_t light_of(const BuiltScene& built, uint32_t object);
// The light-list copy of light `light` (its mesh in index order: Tri, TriNrm and packed records at its tri_base) and its LightTri
// records, rewritten in place from built->inputs and the light's current pdfT.  Counts and light_tri_first stay.
void write_light_mesh(BuiltScene* built, uint32_t light, uint32_t object);

// New transforms for `n` objects of a built scene (insertion indices; meshes, instances and spheres - area lights only while
// BuiltScene::dynamic_lights is set: apply_repose then gives each listed light its new Light record and area terms): itrans /
// has_trans / posed box of those, the BVH<Object> (or list order) and the tables that follow from it.  No BVH<Triangle> is
// rebuilt and no triangle moves.  Returns "" or an error message; *bad_argument tells a refused list (duplicate, out of range,
// a light) from a BVH<Object> build that does not terminate.
std::string prepare_repose(const BuiltScene& built, const uint32_t* objects, const Mat4* trans, uint32_t n, ReposedTop* out,
                           bool* bad_argument);
void apply_repose(BuiltScene* built, ReposedTop* top);
// srt_pt_repose's refusals alone: "" or why the list cannot be re-posed (out of range, a duplicate, an area light).
std::string check_repose_list(const BuiltScene& built, const uint32_t* objects, uint32_t n);
// prepare_repose with the pose-dependent values supplied by the caller instead of computed (srt_pt_repose_device: a kernel
// computed them, pt_pose.h): trans / itrans / has_trans of the n listed objects in list order, and either the posed boxes of ALL
// objects in insertion order (six floats each; the BVH<Object> is then built here, by build_scene's rule) or the BVH<Object> the
// caller built over them (moved from).  A list scene needs neither.  The objects that are not listed keep the values of their
// committed records.  mat_inverse, mat_ne_identity and Box::transform stay the definition the supplied values are held to
// (posed_values states them for one object); nothing here recomputes them.
struct SuppliedPoses {
  const Mat4* trans = nullptr;
  const Mat4* itrans = nullptr;
  const uint32_t* has_trans = nullptr;
  const float* boxes6 = nullptr;
  HostBVH* prebuilt = nullptr;
};
std::string prepare_repose_supplied(const BuiltScene& built, const uint32_t* objects, uint32_t n, const SuppliedPoses& poses, ReposedTop* out,
                                    bool* bad_argument);
// What the Object ctor and Object::bbox make of one transform and one object-space box (rays/object.h:18-21, 51-55).
void posed_values(const Mat4& trans, const float local_box6[6], Mat4* itrans, uint32_t* has_trans, float box6[6]);

// What srt_pt_update_mesh derives for new vertex arrays of ONE mesh of a built scene (an object added by srt_pt_add_mesh: not an
// instance, a sphere or an area light; same vertex count, same index buffer), built next to the scene: the mesh's
// BVH<Triangle> (leaf size 4; none in list mode), its flattened nodes, interior records and triangle records, the object-space
// box of the mesh and of its instances, and - because those boxes changed - the BVH<Object> and the tables that follow object
// order, as prepare_repose derives them.  The triangle range of the mesh never moves (the triangle count is fixed); its node
// and record ranges may have another length, and the ranges stored behind them are re-packed: `store` holds every object's new
// offsets.  prepare_mesh_update leaves `built` untouched; apply_mesh_update moves everything in (it cannot fail).
struct MeshUpdate {
  uint32_t object = 0;
  std::vector<float> pos, nrm;
  HostBVH blas;
  std::vector<Node> nodes;            // the mesh's BVH<Triangle>, flattened
  std::vector<WaveInterior> recs;     // its interior records
  std::vector<Tri> tris;              // its triangle range, in the new primitive order
  std::vector<TriNrm> tri_nrm;
  std::vector<float> tri_packed;
  std::vector<float> local_boxes;     // of every object
  std::vector<MeshStore> store;       // of every object
  uint32_t max_blas_depth = 0;        // over all stored meshes
  ReposedTop top;                     // (listed / trans stay empty: no pose changes)
};
// "" or why `object` of `built` cannot take new arrays of nverts vertices (out of range, a sphere, an instance, an area light,
// another vertex count).
std::string check_mesh_update(const BuiltScene& built, uint32_t object, uint32_t nverts);
// pos / nrm: 3 floats per vertex.  `prebuilt`: the BVH<Triangle> of the new arrays where the caller has built it already (on the
// device, from boxes computed there; bit-equal to the host build; its arrays are moved from) - otherwise it is built here, by
// build_scene's rule.  Returns ""
// or an error message; *bad_argument tells a refused argument (check_mesh_update) from a build that does not terminate.
std::string prepare_mesh_update(const BuiltScene& built, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                                HostBVH* prebuilt, MeshUpdate* out, bool* bad_argument);
void apply_mesh_update(BuiltScene* built, MeshUpdate* update);

// What srt_pt_refit_mesh derives for new vertex arrays of one mesh of a scene built with BVHs (the same objects
// check_mesh_update admits), built next to the scene: the mesh's BVH<Triangle> keeps its links and its primitive order and takes
// new boxes - a leaf's is the BBox::enclose fold of Triangle::bbox over its triangles in primitive order, an interior node's the
// enclose of its left and then its right child's (children lie behind their parent, so one backward pass does it) - which is how
// BVH<Primitive>::build forms every node box (student/bvh.inl:73-75, 119-123), so the committed vertices give the committed
// boxes back (as values: the sign of a zero bound that occurs as +0 and as -0 follows the fold's order).  Node, record and
// triangle counts stay; the object-space box of the mesh and of its instances becomes the new root box, and the BVH<Object> and the tables of object order follow as in prepare_repose.  prepare_mesh_refit leaves `built`
// untouched; apply_mesh_refit writes everything in place (it cannot fail).
struct MeshRefit {
  uint32_t object = 0;
  std::vector<float> pos, nrm;
  std::vector<float> boxes;           // six floats {mn, mx} per node of the mesh's BVH<Triangle>
  std::vector<float> local_boxes;     // of every object
  ReposedTop top;                     // (listed / trans stay empty: no pose changes)
  std::vector<float> top_boxes;       // prepare_mesh_refit_inplace only: six floats per node of the kept BVH<Object>
};
// The refitted boxes alone: six floats per node of `tree` over the triangles of (pos, idx).
void refit_boxes(const HostBVH& tree, const float* pos, const std::vector<uint32_t>& idx, std::vector<float>* boxes6);
// pos / nrm: 3 floats per vertex.  `node_boxes`: the refitted boxes where the caller has them already (from the device kernels,
// pt_mesh_update.hip; six floats per node) - otherwise refit_boxes computes them here.  Returns "" or an error message;
// *bad_argument tells a refused argument (check_mesh_update, a non-finite coordinate, a scene without BVHs) from a BVH<Object> build that
// does not terminate.
std::string prepare_mesh_refit(const BuiltScene& built, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                               const float* node_boxes, MeshRefit* out, bool* bad_argument);
void apply_mesh_refit(BuiltScene* built, MeshRefit* refit);
// srt_pt_refit_mesh_inplace, the definition: the refit above with BOTH trees kept.  The mesh's BVH<Triangle>, its triangle, normal and
// packed records, its light-list copy and the object-space boxes of the mesh and of its instances change exactly as
// prepare_mesh_refit / apply_mesh_refit change them; the BVH<Object> is not rebuilt but takes the boxes of top_refit_boxes over
// effective_boxes of the posed boxes - Object::bbox of every object from its unchanged transform and its (new) object-space box -
// through write_top_boxes, and write_top_counts runs while any object is inactive.  No link, order, count, slot, ordinal, lazy table
// or depth changes anywhere: the result is what srt_pt_refit_mesh would give if its last step were srt_pt_repose_refit of the mesh
// and its instances with their current transforms in place of the rebuild.  So nothing here can fail but the arguments:
// check_mesh_update's refusals, a scene without BVHs and - unless !refuse_non_finite: the device form's lagging record takes what the
// kernels computed - a non-finite coordinate.  `node_boxes` as in prepare_mesh_refit.  R->top stays empty.
std::string prepare_mesh_refit_inplace(const BuiltScene& built, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                                       const float* node_boxes, bool refuse_non_finite, MeshRefit* out);
void apply_mesh_refit_inplace(BuiltScene* built, MeshRefit* refit);
// What srt_pt_repose_refit derives for new poses of a committed scene: the BVH<Object> keeps its links {start, size, l, r} and its
// primitive order and takes new boxes, as a mesh's tree does in prepare_mesh_refit - a leaf's is the BBox::enclose fold, from
// BBox(), of Object::bbox of its objects in primitive order (a leaf holds 0 or 1), an interior node's the enclose of its left and
// then its right child's (student/bvh.inl:73-75, 119-123) - so the committed poses give the committed boxes back, as values (the
// zero-sign caveat of prepare_mesh_refit applies).  The listed objects take the Object ctor's values (posed_values); counts, object
// slots, node_base, ordinals, wave_lazy, lazy_objects, max_tlas_depth and every BVH<Triangle> stay.  Non-finite matrices are not
// refused.  A list scene has no tree: `boxes` stays empty and only the listed records change.  This is what the device kernels of
// srt_pt_repose_refit_device are held to, bit for bit.  prepare_top_refit leaves `built` untouched and can refuse the list only
// (check_repose_list); apply_top_refit writes in place (it cannot fail): inputs' transforms, the listed records of flat.objects,
// the boxes of tlas, flat.nodes[0 .. tlas_nodes) and flat.wave_tlas, and a listed light's record and area terms.
struct TopRefit {
  std::vector<uint32_t> listed;       // insertion indices ..
  std::vector<Mat4> trans, itrans;    // .. their new transforms, the inverses ..
  std::vector<uint32_t> has_trans;    // .. and trans != I
  std::vector<float> boxes;           // six floats {mn, mx} per node of the BVH<Object>
};
// The refitted boxes alone: six floats per node of `tree` over the posed boxes of all objects (six floats each, by insertion index).
void top_refit_boxes(const HostBVH& tree, const float* posed_boxes6, std::vector<float>* boxes6);
std::string prepare_top_refit(const BuiltScene& built, const uint32_t* objects, const Mat4* trans, uint32_t n, TopRefit* out);
void apply_top_refit(BuiltScene* built, TopRefit* refit);
// srt_pt_set_active, the definition.  effective_boxes: the boxes the BVH<Object>'s leaves fold - posed6 (six floats per object by
// insertion index: Object::bbox) with BBox(), min = +FLT_MAX and max = -FLT_MAX, in the place of every inactive object's.
// posed_boxes: Object::bbox of every object from the scene's own transforms and object-space boxes.  write_top_boxes: the one place
// that writes boxes (six floats per node) into the BVH<Object> - the host tree, flat.nodes[0 .. tlas_nodes) and flat.wave_tlas; links,
// references and counts stay.  write_top_counts: the number of objects a leaf of the BVH<Object> holds FOR THE WALKS - the count
// word of its flattened node and the l_cnt / r_cnt of the sweep record above it: the leaf's size, or 0 while every object in it is
// inactive.  The host tree (what srt_pt_dump_bvh shows) keeps its sizes.  An empty box alone does not hide a leaf: find_closest_hit
// visits the child whose box was MISSED whenever the other child returns a hit farther than ray.dist_bounds.x, because cur_far_t
// starts as ray.dist_bounds (student/bvh.inl:191-192, 216) - so a hidden leaf is also left without primitives, which the walks take
// as they take the empty leaves a build can produce (a leaf holds 0 or 1).  mask_top: top_refit_boxes over
// effective_boxes(posed_boxes), written by write_top_boxes, then write_top_counts - what apply_set_active runs, and what every call
// that replaces the BVH<Object> (apply_repose, apply_mesh_update, apply_mesh_refit) ends with while any_inactive(); with every
// object active those calls run no extra fold.
// check_active_list: "" or why the n listed objects cannot be switched - *unsupported: the scene has no BVH<Object> to hide an
// object from (committed without BVHs) or its root is a leaf (find_closest_hit tests children only, never the root's own box);
// otherwise a bad argument: out of range, a duplicate, an emissive object (the light list would go on sampling it).
// apply_set_active: the listed flags into the table (non-zero: active); false, and nothing written, when no flag changes.
bool any_inactive(const BuiltScene& built);
void effective_boxes(const BuiltScene& built, std::vector<float>* posed6);
void posed_boxes(const BuiltScene& built, std::vector<float>* posed6);
void write_top_boxes(BuiltScene* built, const std::vector<float>& boxes6);
void write_top_counts(BuiltScene* built);
void mask_top(BuiltScene* built);
std::string check_active_list(const BuiltScene& built, const uint32_t* objects, uint32_t n, bool* unsupported);
bool apply_set_active(BuiltScene* built, const uint32_t* objects, const uint8_t* active, uint32_t n);
// SAH cost of a BVH (what a caller compares before and after refits to decide when to rebuild), in double from the node boxes:
// sum over interior nodes of SA(n) / SA(root) + sum over leaves of size(n) * SA(n) / SA(root), SA = 2 (xy + yz + zx) of the extents.
// A node whose box is empty (mn > mx on an axis: nothing active below it) contributes 0, and an empty root gives cost 0.
double tree_cost(const HostBVH& tree);

Camera make_camera(const float iview[16], float vert_fov_deg, float aspect_ratio);

// Delta_Light ctor: itrans = T.inverse(), has_trans = T != I.
DeltaLight make_delta_light(uint32_t type, const float radiance[3], const float angle_bounds[2], const Mat4& trans);

}  // namespace srt

#endif
