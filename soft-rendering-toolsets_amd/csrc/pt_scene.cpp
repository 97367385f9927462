// Host-side build_scene for the MI355X path tracer: Object construction, BVH builds that are
// structure-identical to the reference's, and flattening into the layout of pt_scene.h.
// Reference paths are relative to /root/reference/Assignments/Scotty3D/src/.
#include "pt_scene.h"

#include <cfloat>
#include <cmath>
#include <algorithm>
#include <cstring>

namespace srt {

namespace {

struct Box {
  float mn[3], mx[3];
  Box() { for (int i = 0; i < 3; i++) { mn[i] = FLT_MAX; mx[i] = -FLT_MAX; } }  // BBox(), lib/bbox.h:17
  void enclose(const float p[3]) {
    for (int i = 0; i < 3; i++) { mn[i] = std::min(mn[i], p[i]); mx[i] = std::max(mx[i], p[i]); }
  }
  void enclose(const Box& b) {
    for (int i = 0; i < 3; i++) { mn[i] = std::min(mn[i], b.mn[i]); mx[i] = std::max(mx[i], b.mx[i]); }
  }
  float center(int axis) const { return (mn[axis] + mx[axis]) * 0.5f; }
  float surface_area() const {  // lib/bbox.h:50-54
    if (mn[0] > mx[0] || mn[1] > mx[1] || mn[2] > mx[2]) return 0.0f;
    const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
    return 2.0f * (ex * ez + ex * ey + ey * ez);
  }
  void transform(const Mat4& t) {  // lib/bbox.h:57-73
    float amin[3], amax[3];
    for (int i = 0; i < 3; i++) { amin[i] = mn[i]; amax[i] = mx[i]; mn[i] = mx[i] = t.c[3][i]; }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const float a = t.c[j][i] * amin[j], b = t.c[j][i] * amax[j];
        if (a < b) { mn[i] += a; mx[i] += b; } else { mn[i] += b; mx[i] += a; }
      }
  }
};

// Triangle::bbox (student/tri_mesh.cpp:7-30): zero-extent axes are widened by +1 on the max side.
Box triangle_box(const float* p0, const float* p1, const float* p2) {
  Box b;
  for (int a = 0; a < 3; a++) {
    const float lo = std::min({p0[a], p1[a], p2[a]});
    float hi = std::max({p0[a], p1[a], p2[a]});
    hi = (lo >= hi) ? (lo + 1.0f) : hi;
    b.mn[a] = lo; b.mx[a] = hi;
  }
  return b;
}

// std::partition as libstdc++ implements it for bidirectional iterators; the permutation it
// leaves behind decides the order of primitives inside leaves (and with it Trace::min tie-breaks).
uint32_t partition_by_center(std::vector<uint32_t>& prim, const std::vector<Box>& boxes, uint32_t first, uint32_t last,
                             int axis, float line) {
  auto pred = [&](uint32_t slot) { return boxes[prim[slot]].center(axis) < line; };
  while (true) {
    while (true) {
      if (first == last) return first;
      if (pred(first)) ++first; else break;
    }
    --last;
    while (true) {
      if (first == last) return first;
      if (!pred(last)) --last; else break;
    }
    std::swap(prim[first], prim[last]);
    ++first;
  }
}

// BVH<Primitive>::build (student/bvh.inl:35-163): level order; per axis up to nine candidate planes
// min + k*interval (float accumulation), SAH cost, axis chosen by exact float equality with the minimum.
thread_local DeviceBvhBuilder g_device_builder = nullptr;
thread_local uint32_t g_device_min = 0;

bool build_bvh(const std::vector<Box>& boxes, uint32_t max_leaf, HostBVH* out) {
  const uint32_t n = (uint32_t)boxes.size();
  static_assert(sizeof(Box) == 6 * sizeof(float), "Box is six floats");
  if (g_device_builder && n >= g_device_min && n > max_leaf && g_device_builder(&boxes[0].mn[0], n, max_leaf, out)) return true;
  // (a device build that fails - no termination, or no memory - falls through: the host build gives the verdict)
  out->nodes.clear();
  out->prim.resize(n);
  for (uint32_t i = 0; i < n; i++) out->prim[i] = i;
  auto new_node = [&](const Box& b, uint32_t start, uint32_t size) {
    HostNode nd;
    for (int i = 0; i < 3; i++) { nd.mn[i] = b.mn[i]; nd.mx[i] = b.mx[i]; }
    nd.start = start; nd.size = size; nd.l = 0; nd.r = 0;
    out->nodes.push_back(nd);
  };
  Box all;
  for (const Box& b : boxes) all.enclose(b);
  new_node(all, 0, n);
  const size_t node_limit = 8ull * n + 64;
  struct Split { Box left, right; int nl = 0, nr = 0; float line = 0; };
  for (size_t cur = 0; cur < out->nodes.size(); cur++) {
    if (out->nodes[cur].size <= max_leaf) continue;
    if (out->nodes.size() > node_limit) return false;  // the reference would never return
    const HostNode nd = out->nodes[cur];
    Box nbox;
    for (int i = 0; i < 3; i++) { nbox.mn[i] = nd.mn[i]; nbox.mx[i] = nd.mx[i]; }
    const uint32_t start = nd.start, end = nd.start + nd.size;
    float best_cost[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    Split best[3];
    for (int axis = 0; axis < 3; axis++) {
      Split best_axis;
      const float interval = (nbox.mx[axis] - nbox.mn[axis]) / (float)10;
      for (float plane = nbox.mn[axis] + interval; plane < nbox.mx[axis]; plane += interval) {
        const uint32_t mid = partition_by_center(out->prim, boxes, start, end, axis, plane);
        Split s;
        s.line = plane;
        for (uint32_t i = start; i < end; i++) {
          if (i >= mid) { s.right.enclose(boxes[out->prim[i]]); s.nr++; }
          else { s.left.enclose(boxes[out->prim[i]]); s.nl++; }
        }
        const float cost = s.left.surface_area() / nbox.surface_area() * (float)s.nl +
                           s.right.surface_area() / nbox.surface_area() * (float)s.nr + 1.0f;
        if (cost < best_cost[axis]) { best_cost[axis] = cost; best_axis = s; }
      }
      best[axis] = best_axis;
    }
    const float lowest = std::min(best_cost[0], std::min(best_cost[1], best_cost[2]));
    const int axis = (lowest == best_cost[0]) ? 0 : ((lowest == best_cost[1]) ? 1 : 2);
    const uint32_t l = (uint32_t)out->nodes.size();
    partition_by_center(out->prim, boxes, start, end, axis, best[axis].line);
    new_node(best[axis].left, nd.start, (uint32_t)best[axis].nl);
    new_node(best[axis].right, nd.start + (uint32_t)best[axis].nl, (uint32_t)best[axis].nr);
    out->nodes[cur].l = l;
    out->nodes[cur].r = l + 1;
  }
  return true;
}

}  // namespace
void set_device_bvh_builder(DeviceBvhBuilder fn, uint32_t min_prims) { g_device_builder = fn; g_device_min = min_prims; }
namespace {

// Interior-node nesting of the tree.  Children are allocated after their parent (level order, student/bvh.inl:144-145),
// so one backward pass over the node array does it - no recursion, however skewed the tree.
uint32_t interior_depth(const HostBVH& b) {
  if (b.nodes.empty()) return 0;
  std::vector<uint32_t> d(b.nodes.size(), 0u);
  for (size_t n = b.nodes.size(); n-- > 0;) {
    const HostNode& nd = b.nodes[n];
    if (nd.l != nd.r) d[n] = 1u + std::max(d[nd.l], d[nd.r]);
  }
  return d[0];
}

// Mat4 * Vec3 with perspective divide (lib/mat4.h:125-131).
void mat_point(const Mat4& m, const float v[3], float out[3]) {
  float o[4];
  for (int j = 0; j < 4; j++) o[j] = ((m.c[0][j] * v[0] + m.c[1][j] * v[1]) + m.c[2][j] * v[2]) + m.c[3][j] * 1.0f;
  out[0] = o[0] / o[3]; out[1] = o[1] / o[3]; out[2] = o[2] / o[3];
}

void append_nodes(const HostBVH& b, std::vector<Node>* out) {
  for (const HostNode& h : b.nodes) {
    Node n;
    for (int i = 0; i < 3; i++) { n.mn[i] = h.mn[i]; n.mx[i] = h.mx[i]; }
    if (h.l == h.r) { n.left = h.start; n.count = LEAF_BIT | h.size; }
    else { n.left = h.l; n.count = 0; }
    out->push_back(n);
  }
}

// One record per interior node of `b`, in node order (parents first): both child boxes and the child references.  A leaf
// child's reference is ~leaf_code(leaf).
template <class LeafCode>
void append_records(const HostBVH& b, LeafCode leaf_code, std::vector<WaveInterior>* out) {
  const std::vector<HostNode>& N = b.nodes;
  std::vector<int32_t> rank(N.size(), -1);
  int32_t q = 0;
  for (size_t n = 0; n < N.size(); n++)
    if (N[n].l != N[n].r) rank[n] = q++;
  for (size_t n = 0; n < N.size(); n++) {
    if (N[n].l == N[n].r) continue;
    WaveInterior wi;
    const HostNode& a = N[N[n].l];
    const HostNode& c = N[N[n].r];
    for (int i = 0; i < 3; i++) { wi.boxl[i] = a.mn[i]; wi.boxl[3 + i] = a.mx[i]; wi.boxr[i] = c.mn[i]; wi.boxr[3 + i] = c.mx[i]; }
    wi.l_ref = (a.l != a.r) ? rank[N[n].l] : ~(int32_t)leaf_code(a);
    wi.r_ref = (c.l != c.r) ? rank[N[n].r] : ~(int32_t)leaf_code(c);
    wi.l_cnt = a.size;
    wi.r_cnt = c.size;
    out->push_back(wi);
  }
}

// The pose-dependent half of build_scene, shared with prepare_repose: Object ctor values and Object::bbox per object, the
// BVH<Object> (leaf size 1) or List<Object> over them, its flattened nodes and its sweep records.
struct Top {
  std::vector<Mat4> itrans;
  std::vector<bool> has_trans;
  HostBVH tlas;
  std::vector<Node> nodes;
  std::vector<WaveInterior> wave;
  uint32_t depth = 0;
};
// The Object ctor values and Object::bbox of every object: what a pose decides.
void pose_objects(const std::vector<Mat4>& trans, const std::vector<float>& local_boxes, Top* T, std::vector<Box>* obj_boxes) {
  const uint32_t nobj = (uint32_t)trans.size();
  T->itrans.resize(nobj);
  T->has_trans.resize(nobj);
  obj_boxes->resize(nobj);
  for (uint32_t i = 0; i < nobj; i++) {
    T->itrans[i] = mat_inverse(trans[i]);            // Object ctor, rays/object.h:18-21
    T->has_trans[i] = mat_ne_identity(trans[i]);
    Box ob;
    for (int a = 0; a < 3; a++) { ob.mn[a] = local_boxes[6 * i + a]; ob.mx[a] = local_boxes[6 * i + 3 + a]; }
    if (T->has_trans[i]) ob.transform(trans[i]);     // Object::bbox, rays/object.h:51-55
    (*obj_boxes)[i] = ob;
  }
}
// The BVH<Object> (leaf size 1) or List<Object> over the posed boxes, flattened.  `prebuilt`: the tree where the caller has built
// it already (on the device, bit-equal to the host build; its arrays are moved from) - then obj_boxes is not read.
bool tree_top(const std::vector<Box>& obj_boxes, uint32_t nobj, bool use_bvh, HostBVH* prebuilt, Top* T) {
  if (use_bvh) {
    if (prebuilt) { T->tlas.nodes.swap(prebuilt->nodes); T->tlas.prim.swap(prebuilt->prim); }
    else if (!build_bvh(obj_boxes, 1, &T->tlas)) return false;
    append_nodes(T->tlas, &T->nodes);
    T->depth = interior_depth(T->tlas);
    // interior-node sweep order for the wave-uniform kernel: a leaf child is ~first object slot
    append_records(T->tlas, [](const HostNode& leaf) { return leaf.start; }, &T->wave);
  } else {
    T->tlas.nodes.clear();
    T->tlas.prim.resize(nobj);
    for (uint32_t i = 0; i < nobj; i++) T->tlas.prim[i] = i;
  }
  return true;
}
bool build_top(const std::vector<Mat4>& trans, const std::vector<float>& local_boxes, bool use_bvh, Top* T) {
  std::vector<Box> obj_boxes;
  pose_objects(trans, local_boxes, T, &obj_boxes);
  return tree_top(obj_boxes, (uint32_t)trans.size(), use_bvh, nullptr, T);
}

// The object records in BVH<Object> primitive order (insertion order in list mode): an instance's record carries its
// source's ranges and its own transform pair and material.
void make_objects(const std::vector<ObjectInput>& inputs, const std::vector<Mat4>& trans, const Top& T, const std::vector<MeshStore>& store,
                  uint32_t tlas_nodes, bool use_bvh, std::vector<Object>* objects, std::vector<uint32_t>* lazy_objects) {
  objects->clear();
  lazy_objects->clear();
  for (uint32_t slot = 0; slot < (uint32_t)inputs.size(); slot++) {
    const uint32_t i = T.tlas.prim[slot];
    const ObjectInput& in = inputs[i];
    Object o;
    std::memset(&o, 0, sizeof o);
    o.kind = in.kind;
    o.has_trans = T.has_trans[i] ? 1u : 0u;
    o.material = (int32_t)in.material;
    o.use_bvh = (in.kind == OBJ_MESH && use_bvh) ? 1u : 0u;
    o.radius = in.radius;
    o.id = i + 1;
    o.trans = trans[i];
    o.itrans = T.itrans[i];
    if (in.kind == OBJ_MESH) {
      const MeshStore& m = store[i];
      o.tri_base = m.tri_base; o.ntri = m.ntri;
      if (use_bvh) { o.node_base = tlas_nodes + m.node_off; o.nnodes = m.nnodes; o.rec_base = m.rec_base; o.nrec = m.nrec; }
    }
    if (o.kind == OBJ_MESH && o.use_bvh != 0u && o.nrec > 0u) {
      // a mesh with a real BVH<Triangle>: its ordinal among those (the streamed sweeps queue its walks per ordinal)
      o.use_bvh |= (uint32_t)lazy_objects->size() << 8;
      lazy_objects->push_back(slot);
    }
    objects->push_back(o);
  }
}

// Which children of the top-level records hold a mesh with a real BVH<Triangle> somewhere below (children come after
// their parent in sweep order, so one backward pass does it).
void make_wave_lazy(const std::vector<WaveInterior>& wave, const std::vector<Object>& objects, std::vector<uint32_t>* wave_lazy) {
  wave_lazy->assign(wave.size(), 0u);
  for (size_t q = wave.size(); q-- > 0;) {
    const WaveInterior& w = wave[q];
    auto child_has = [&](int32_t ref, uint32_t cnt) {
      if (ref >= 0) return (*wave_lazy)[(size_t)ref] != 0u;
      const uint32_t first = (uint32_t)~ref;
      for (uint32_t k = first; k < first + cnt && k < objects.size(); k++)
        if (objects[k].kind == OBJ_MESH && objects[k].use_bvh != 0u && objects[k].nrec > 0u) return true;
      return false;
    };
    (*wave_lazy)[q] = (child_has(w.l_ref, w.l_cnt) ? 1u : 0u) | (child_has(w.r_ref, w.r_cnt) ? 2u : 0u);
  }
}

// The triangle records of mesh `m` in `order` (index order without one), appended to the three arrays.
void append_triangles(const MeshInput& m, const std::vector<uint32_t>* order, std::vector<Tri>* tris, std::vector<TriNrm>* tri_nrm,
                      std::vector<float>* tri_packed) {
  const uint32_t ntri = (uint32_t)m.idx.size() / 3;
  for (uint32_t k = 0; k < ntri; k++) {
    const uint32_t t = order ? (*order)[k] : k;
    const float* p0 = &m.pos[3 * m.idx[3 * t]];
    const float* p1 = &m.pos[3 * m.idx[3 * t + 1]];
    const float* p2 = &m.pos[3 * m.idx[3 * t + 2]];
    Tri g;
    TriNrm nn;
    std::memset(&g, 0, sizeof g);
    std::memset(&nn, 0, sizeof nn);
    for (int a = 0; a < 3; a++) {
      g.p0[a] = p0[a];
      g.e1[a] = p1[a] - p0[a];  // p0p1, student/tri_mesh.cpp:60
      g.e2[a] = p2[a] - p0[a];  // p0p2
      nn.n0[a] = m.nrm[3 * m.idx[3 * t] + a];
      nn.n1[a] = m.nrm[3 * m.idx[3 * t + 1] + a];
      nn.n2[a] = m.nrm[3 * m.idx[3 * t + 2] + a];
    }
    tris->push_back(g);
    tri_nrm->push_back(nn);
    for (int a = 0; a < 3; a++) tri_packed->push_back(g.p0[a]);
    for (int a = 0; a < 3; a++) tri_packed->push_back(g.e1[a]);
    for (int a = 0; a < 3; a++) tri_packed->push_back(g.e2[a]);
  }
}

// A leaf child of a BVH<Triangle> interior record: ~((first triangle slot << 3) | triangle count)
uint32_t blas_leaf_code(const HostNode& leaf) { return (leaf.start << 3) | (leaf.size & 7u); }

// Term tables of Mat4::inverse / Mat4::det: digit pairs are (col,row); the order of terms and of the
// factors inside a term fixes the fp32 rounding, so it is data (lib/mat4.h:206-231, 296-343).
const char* const kInverseTerms[16] = {
    "+122331-132231+132132-112332-122133+112233", "+032231-022331-032132+012332+022133-012233",
    "+021331-031231+031132-011332-021133+011233", "+031221-021321-031122+011322+021123-011223",
    "+132230-122330-132032+102332+122033-102233", "+022330-032230+032032-002332-022033+002233",
    "+031230-021330-031032+001332+021033-001233", "+021320-031220+031022-001322-021023+001223",
    "+112330-132130+132031-102331-112033+102133", "+032130-012330-032031+002331+012033-002133",
    "+011330-031130+031031-001331-011033+001133", "+031120-011320-031021+001321+011023-001123",
    "+122130-112230-122031+102231+112032-102132", "+012230-022130+022031-002231-012032+002132",
    "+021130-011230-021031+001231+011032-001132", "+011220-021120+021021-001221-011022+001122"};
const char* const kDetTerms =
    "+03122130-02132130-03112230+01132230+02112330-01122330-03122031+02132031+03102231-00132231-02102331"
    "+00122331+03112032-01132032-03102132+00132132+01102332-00112332-02112033+01122033+02102133-00122133"
    "-01102233+00112233";

float signed_products(const Mat4& m, const char* t, int factors) {
  float acc = 0.0f;
  bool first = true;
  while (*t) {
    const bool minus = (*t++ == '-');
    float p = m.c[t[0] - '0'][t[1] - '0'];
    for (int f = 1; f < factors; f++) p = p * m.c[t[2 * f] - '0'][t[2 * f + 1] - '0'];
    t += 2 * factors;
    if (first) { acc = p; first = false; }
    else acc = minus ? acc - p : acc + p;
  }
  return acc;
}

}  // namespace

Mat4 mat_identity() {
  Mat4 r;
  std::memset(&r, 0, sizeof r);
  r.c[0][0] = r.c[1][1] = r.c[2][2] = r.c[3][3] = 1.0f;
  return r;
}

Mat4 mat_inverse(const Mat4& m) {
  Mat4 r;
  for (int e = 0; e < 16; e++) r.c[e / 4][e % 4] = signed_products(m, kInverseTerms[e], 3);
  const float det = signed_products(m, kDetTerms, 4);
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) r.c[i][j] /= det;
  return r;
}

Mat4 mat_mul(const Mat4& self, const Mat4& m) {
  Mat4 r;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      float acc = 0.0f;
      for (int k = 0; k < 4; k++) acc += m.c[i][k] * self.c[k][j];
      r.c[i][j] = acc;
    }
  return r;
}

bool mat_ne_identity(const Mat4& m) {  // operator!= compares values, so -0.0f equals 0.0f
  const Mat4 id = mat_identity();
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      if (m.c[i][j] != id.c[i][j]) return true;
  return false;
}

DeltaLight make_delta_light(uint32_t type, const float radiance[3], const float angle_bounds[2], const Mat4& trans) {
  DeltaLight l;
  std::memset(&l, 0, sizeof l);
  l.type = type;
  for (int i = 0; i < 3; i++) l.radiance[i] = radiance[i];
  l.angle_bounds[0] = angle_bounds ? angle_bounds[0] : 0.0f;
  l.angle_bounds[1] = angle_bounds ? angle_bounds[1] : 0.0f;
  l.trans = trans;
  l.itrans = mat_inverse(trans);
  l.has_trans = mat_ne_identity(trans) ? 1u : 0u;
  return l;
}

Camera make_camera(const float iview[16], float vert_fov_deg, float aspect_ratio) {
  Camera c;
  std::memcpy(&c.iview, iview, sizeof(Mat4));
  c.vert_fov = vert_fov_deg;
  c.aspect_ratio = aspect_ratio;
  // student/camera.cpp:17-18; Radians(v) = v * (PI_F / 180.0f).  tanf is host libm, as in the reference.
  const float PI_F = 3.14159265358979323846264338327950288f;
  c.screen_h = std::tan((vert_fov_deg * (PI_F / 180.0f)) / 2.0f) * 1.0f * 2.0f;
  c.screen_w = aspect_ratio * c.screen_h;
  return c;
}

void light_record(const Mat4& trans, const Mat4& itrans, bool has_trans, Light* L) {
  L->has_trans = has_trans ? 1u : 0u;
  L->trans = trans;
  L->itrans = itrans;
  const Mat4 id = mat_identity();
  L->pdfT = id;
  L->pdfiT = id;
  if (has_trans) {  // Object::pdf, rays/object.h:90-94
    L->pdfT = mat_mul(id, trans);
    L->pdfiT = mat_mul(itrans, id);
  }
}

float light_area_term(const Mat4& pdfT, const float v0[3], const float v1[3], const float v2[3]) {
  const float* v[3] = {v0, v1, v2};
  float w[3][3];
  for (int k = 0; k < 3; k++) mat_point(pdfT, v[k], w[k]);
  // a = 2.0f / cross(v_1 - v_0, v_2 - v_0).norm()   (student/tri_mesh.cpp:137)
  const float ax = w[1][0] - w[0][0], ay = w[1][1] - w[0][1], az = w[1][2] - w[0][2];
  const float bx = w[2][0] - w[0][0], by = w[2][1] - w[0][1], bz = w[2][2] - w[0][2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  return 2.0f / std::sqrt(cx * cx + cy * cy + cz * cz);
}

LightTri light_tri_record(const Mat4& pdfT, const MeshInput& mesh, uint32_t t) {
  LightTri lt;
  std::memset(&lt, 0, sizeof lt);
  const float* v[3] = {&mesh.pos[3 * (size_t)mesh.idx[3 * (size_t)t]], &mesh.pos[3 * (size_t)mesh.idx[3 * (size_t)t + 1]],
                       &mesh.pos[3 * (size_t)mesh.idx[3 * (size_t)t + 2]]};
  for (int a = 0; a < 3; a++) { lt.v0[a] = v[0][a]; lt.v1[a] = v[1][a]; lt.v2[a] = v[2][a]; }
  lt.area_term = light_area_term(pdfT, v[0], v[1], v[2]);
  return lt;
}

int32_t light_of(const BuiltScene& B, uint32_t object) {
  if (object >= B.inputs.size() || !B.inputs[object].is_light || B.inputs[object].mesh.idx.empty()) return -1;
  int32_t li = 0;   // lights are made in insertion order, one per emissive object that carries a mesh
  for (uint32_t i = 0; i < object; i++)
    if (B.inputs[i].is_light && !B.inputs[i].mesh.idx.empty()) li++;
  return (size_t)li < B.flat.lights.size() ? li : -1;
}

void write_light_mesh(BuiltScene* built, uint32_t light, uint32_t object) {
  FlatScene& F = built->flat;
  const Light& L = F.lights[light];
  const MeshInput& mesh = built->inputs[object].mesh;
  std::vector<Tri> tris;
  std::vector<TriNrm> tri_nrm;
  std::vector<float> packed;
  append_triangles(mesh, nullptr, &tris, &tri_nrm, &packed);
  std::copy(tris.begin(), tris.end(), F.tris.begin() + L.tri_base);
  std::copy(tri_nrm.begin(), tri_nrm.end(), F.tri_nrm.begin() + L.tri_base);
  std::copy(packed.begin(), packed.end(), F.tri_packed.begin() + 9 * (size_t)L.tri_base);
  for (uint32_t t = 0; t < L.ntri; t++) F.light_tris[(size_t)(L.tri_base - F.light_tri_first) + t] = light_tri_record(L.pdfT, mesh, t);
}

std::string build_scene(const std::vector<ObjectInput>& objects, const std::vector<Material>& materials, bool use_bvh,
                        BuiltScene* out) {
  BuiltScene& B = *out;
  const bool dynamic_lights = B.dynamic_lights;
  B = BuiltScene();
  B.dynamic_lights = dynamic_lights;
  B.inputs = objects;
  B.active.assign(objects.size(), 1);
  FlatScene& F = B.flat;
  F.use_bvh = use_bvh;
  F.materials = materials;
  for (Material& m : F.materials)
    if (m.type == 0)  // BSDF_Lambertian(albedo) : albedo(albedo / PI_F)   rays/bsdf.h:26
      for (int i = 0; i < 3; i++) m.a[i] = m.a[i] / 3.14159265358979323846264338327950288f;

  const uint32_t nobj = (uint32_t)objects.size();
  for (uint32_t i = 0; i < nobj; i++) {
    const ObjectInput& in = objects[i];
    if (in.material >= materials.size()) return "object " + std::to_string(i) + " references an unknown material";
    if (in.source >= 0) {
      if (in.kind != OBJ_MESH || in.is_light || (uint32_t)in.source >= i || objects[in.source].kind != OBJ_MESH || objects[in.source].source >= 0)
        return "object " + std::to_string(i) + " is not an instance of a mesh added before it";
      continue;
    }
    if (in.kind == OBJ_MESH || (in.is_light && !in.mesh.idx.empty())) {   // a mesh, or an emissive shape's light mesh
      if (in.mesh.idx.empty() || in.mesh.idx.size() % 3) return "mesh " + std::to_string(i) + " has no triangles";
      for (uint32_t v : in.mesh.idx)
        if ((size_t)v * 3 + 2 >= in.mesh.pos.size()) return "mesh " + std::to_string(i) + " has an out-of-range vertex index";
    }
  }

  // Per-mesh BVH<Triangle> (Tri_Mesh::build, student/tri_mesh.cpp:145-170, leaf size 4) and object-space boxes.  An instance
  // (rays/pathtracer.cpp:134-155 without mesh.copy()) takes its source's box: the copy's BVH has the same root.
  B.blas.resize(nobj);
  B.local_boxes.assign(6 * (size_t)nobj, 0.0f);
  std::vector<Mat4> trans(nobj);
  for (uint32_t i = 0; i < nobj; i++) {
    const ObjectInput& in = objects[i];
    trans[i] = in.trans;
    Box ob;
    if (in.kind == OBJ_SPHERE) {                  // Sphere::bbox, student/shapes.cpp:9-15
      const float lo[3] = {-in.radius, -in.radius, -in.radius}, hi[3] = {in.radius, in.radius, in.radius};
      ob.enclose(lo);
      ob.enclose(hi);
    } else if (in.source >= 0) {
      for (int a = 0; a < 3; a++) { ob.mn[a] = B.local_boxes[6 * (size_t)in.source + a]; ob.mx[a] = B.local_boxes[6 * (size_t)in.source + 3 + a]; }
    } else {
      const uint32_t ntri = (uint32_t)in.mesh.idx.size() / 3;
      std::vector<Box> tb(ntri);
      for (uint32_t t = 0; t < ntri; t++)
        tb[t] = triangle_box(&in.mesh.pos[3 * in.mesh.idx[3 * t]], &in.mesh.pos[3 * in.mesh.idx[3 * t + 1]],
                             &in.mesh.pos[3 * in.mesh.idx[3 * t + 2]]);
      if (use_bvh) {
        B.blas_builds++;
        if (!build_bvh(tb, 4, &B.blas[i]))
          return "BVH<Triangle> build of object " + std::to_string(i) +
                 " does not terminate (coincident centroids); the reference loops forever on this mesh";
        const HostNode& root = B.blas[i].nodes[0];
        for (int a = 0; a < 3; a++) { ob.mn[a] = root.mn[a]; ob.mx[a] = root.mx[a]; }
      } else {
        for (const Box& b : tb) ob.enclose(b);  // List<Triangle>::bbox
      }
    }
    for (int a = 0; a < 3; a++) { B.local_boxes[6 * (size_t)i + a] = ob.mn[a]; B.local_boxes[6 * (size_t)i + 3 + a] = ob.mx[a]; }
  }

  // BVH<Object> (leaf size 1) or List<Object>, flattened.
  Top T;
  if (!build_top(trans, B.local_boxes, use_bvh, &T)) return "BVH<Object> build does not terminate (coincident object centroids)";
  B.tlas = T.tlas;
  F.nodes = T.nodes;
  F.tlas_nodes = (uint32_t)F.nodes.size();
  F.max_tlas_depth = T.depth;
  F.wave_tlas = T.wave;

  // Every mesh is stored once, where object order first reaches it or one of its instances.
  B.store.assign(nobj, MeshStore());
  std::vector<bool> stored(nobj, false);
  for (uint32_t slot = 0; slot < nobj; slot++) {
    const uint32_t i = B.tlas.prim[slot];
    if (objects[i].kind != OBJ_MESH) continue;
    const uint32_t src = objects[i].source >= 0 ? (uint32_t)objects[i].source : i;
    if (!stored[src]) {
      stored[src] = true;
      const ObjectInput& in = objects[src];
      MeshStore& m = B.store[src];
      m.tri_base = (uint32_t)F.tris.size();
      m.ntri = (uint32_t)in.mesh.idx.size() / 3;
      if (use_bvh) {
        m.node_off = (uint32_t)F.nodes.size() - F.tlas_nodes;
        m.nnodes = (uint32_t)B.blas[src].nodes.size();
        append_nodes(B.blas[src], &F.nodes);
        F.max_blas_depth = std::max(F.max_blas_depth, interior_depth(B.blas[src]));
        // interior records of this BLAS: a leaf child is ~((first triangle slot << 3) | triangle count)
        m.rec_base = (uint32_t)F.blas_recs.size();
        append_records(B.blas[src], blas_leaf_code, &F.blas_recs);
        m.nrec = (uint32_t)F.blas_recs.size() - m.rec_base;
        append_triangles(in.mesh, &B.blas[src].prim, &F.tris, &F.tri_nrm, &F.tri_packed);
      } else {
        append_triangles(in.mesh, nullptr, &F.tris, &F.tri_nrm, &F.tri_packed);
      }
    }
    B.store[i] = B.store[src];
  }
  make_objects(objects, trans, T, B.store, F.tlas_nodes, use_bvh, &F.objects, &F.lazy_objects);
  make_wave_lazy(F.wave_tlas, F.objects, &F.wave_lazy);
  const std::vector<Mat4>& itrans = T.itrans;
  const std::vector<bool>& has_trans = T.has_trans;

  // Area lights: List<Object> of Tri_Mesh(mesh, false) in insertion order (rays/pathtracer.cpp:105-116,163).
  F.light_tri_first = (uint32_t)F.tris.size();
  for (uint32_t i = 0; i < nobj; i++) {
    const ObjectInput& in = objects[i];
    // an emissive analytic shape is intersected as the shape but lit through its triangle approximation
    // (obj.posed_mesh(), rays/pathtracer.cpp:105-116): its ObjectInput carries that mesh next to the radius
    if (!in.is_light || in.mesh.idx.empty()) continue;
    Light L;
    std::memset(&L, 0, sizeof L);
    L.tri_base = (uint32_t)F.tris.size();
    L.ntri = (uint32_t)in.mesh.idx.size() / 3;
    light_record(in.trans, itrans[i], has_trans[i], &L);
    append_triangles(in.mesh, nullptr, &F.tris, &F.tri_nrm, &F.tri_packed);
    for (uint32_t t = 0; t < L.ntri; t++) F.light_tris.push_back(light_tri_record(L.pdfT, in.mesh, t));
    F.lights.push_back(L);
  }
  return "";
}

std::string check_repose_list(const BuiltScene& B, const uint32_t* objects, uint32_t n) {
  const uint32_t nobj = (uint32_t)B.inputs.size();
  std::vector<bool> seen(nobj, false);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = objects[k];
    if (i >= nobj) return "object " + std::to_string(i) + " is out of range (the scene has " + std::to_string(nobj) + " objects)";
    if (seen[i]) return "object " + std::to_string(i) + " is listed twice";
    if (B.inputs[i].is_light && !B.dynamic_lights)
      return "object " + std::to_string(i) + " is an area light: its light tables depend on its pose, commit the scene again";
    seen[i] = true;
  }
  return "";
}

namespace {

// The tables of object order from a finished Top, moved into *out.
void finish_repose(const BuiltScene& B, const std::vector<Mat4>& trans, Top* T, ReposedTop* out) {
  make_objects(B.inputs, trans, *T, B.store, (uint32_t)T->nodes.size(), B.flat.use_bvh, &out->objects, &out->lazy_objects);
  make_wave_lazy(T->wave, out->objects, &out->wave_lazy);
  out->tlas.nodes.swap(T->tlas.nodes);
  out->tlas.prim.swap(T->tlas.prim);
  out->tlas_nodes.swap(T->nodes);
  out->wave_tlas.swap(T->wave);
  out->max_tlas_depth = T->depth;
}

}  // namespace

std::string prepare_repose(const BuiltScene& B, const uint32_t* objects, const Mat4* new_trans, uint32_t n, ReposedTop* out,
                           bool* bad_argument) {
  const uint32_t nobj = (uint32_t)B.inputs.size();
  *bad_argument = true;
  const std::string refused = check_repose_list(B, objects, n);
  if (!refused.empty()) return refused;
  std::vector<Mat4> trans(nobj);
  for (uint32_t i = 0; i < nobj; i++) trans[i] = B.inputs[i].trans;
  for (uint32_t k = 0; k < n; k++) trans[objects[k]] = new_trans[k];
  *bad_argument = false;
  Top T;
  if (!build_top(trans, B.local_boxes, B.flat.use_bvh, &T)) return "BVH<Object> build does not terminate (coincident object centroids)";
  out->listed.assign(objects, objects + n);
  out->trans.assign(new_trans, new_trans + n);
  finish_repose(B, trans, &T, out);
  return "";
}

std::string prepare_repose_supplied(const BuiltScene& B, const uint32_t* objects, uint32_t n, const SuppliedPoses& P, ReposedTop* out,
                                    bool* bad_argument) {
  const uint32_t nobj = (uint32_t)B.inputs.size();
  *bad_argument = true;
  const std::string refused = check_repose_list(B, objects, n);
  if (!refused.empty()) return refused;
  if (B.flat.use_bvh && !P.prebuilt && !P.boxes6) return "a scene with BVHs needs the posed boxes or the BVH<Object> built from them";
  *bad_argument = false;
  // the objects that are not listed keep what the committed records hold (their id is the insertion index + 1)
  Top T;
  std::vector<Mat4> trans(nobj);
  T.itrans.resize(nobj);
  T.has_trans.resize(nobj);
  for (const Object& o : B.flat.objects) {
    const uint32_t i = o.id - 1u;
    trans[i] = B.inputs[i].trans;
    T.itrans[i] = o.itrans;
    T.has_trans[i] = o.has_trans != 0u;
  }
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = objects[k];
    trans[i] = P.trans[k];
    T.itrans[i] = P.itrans[k];
    T.has_trans[i] = P.has_trans[k] != 0u;
  }
  std::vector<Box> obj_boxes;
  if (B.flat.use_bvh && !P.prebuilt) {
    obj_boxes.resize(nobj);
    std::memcpy(static_cast<void*>(obj_boxes.data()), P.boxes6, (size_t)nobj * sizeof(Box));
  }
  if (!tree_top(obj_boxes, nobj, B.flat.use_bvh, P.prebuilt, &T)) return "BVH<Object> build does not terminate (coincident object centroids)";
  out->listed.assign(objects, objects + n);
  out->trans.assign(P.trans, P.trans + n);
  finish_repose(B, trans, &T, out);
  return "";
}

void posed_values(const Mat4& trans, const float local_box6[6], Mat4* itrans, uint32_t* has_trans, float box6[6]) {
  *itrans = mat_inverse(trans);
  *has_trans = mat_ne_identity(trans) ? 1u : 0u;
  Box ob;
  for (int a = 0; a < 3; a++) { ob.mn[a] = local_box6[a]; ob.mx[a] = local_box6[3 + a]; }
  if (*has_trans) ob.transform(trans);
  for (int a = 0; a < 3; a++) { box6[a] = ob.mn[a]; box6[3 + a] = ob.mx[a]; }
}

void apply_repose(BuiltScene* built, ReposedTop* top) {
  BuiltScene& B = *built;
  FlatScene& F = B.flat;
  for (size_t k = 0; k < top->listed.size(); k++) B.inputs[top->listed[k]].trans = top->trans[k];
  // the BVH<Triangle> nodes stay behind the BVH<Object>'s, however many those are now
  std::vector<Node> nodes(top->tlas_nodes);
  nodes.insert(nodes.end(), F.nodes.begin() + F.tlas_nodes, F.nodes.end());
  F.nodes.swap(nodes);
  F.tlas_nodes = (uint32_t)top->tlas_nodes.size();
  F.max_tlas_depth = top->max_tlas_depth;
  F.wave_tlas.swap(top->wave_tlas);
  F.wave_lazy.swap(top->wave_lazy);
  F.lazy_objects.swap(top->lazy_objects);
  F.objects.swap(top->objects);
  B.tlas.nodes.swap(top->tlas.nodes);
  B.tlas.prim.swap(top->tlas.prim);
  // a listed area light (BuiltScene::dynamic_lights): its Light record from the pose values its new object record carries, and
  // the area terms of its triangles under the new pdfT; the object-space corners and the light-list triangle copies stay
  for (size_t k = 0; k < top->listed.size(); k++) {
    const int32_t li = light_of(B, top->listed[k]);
    if (li < 0) continue;
    for (const Object& o : F.objects) {
      if (o.id != top->listed[k] + 1u) continue;
      Light& L = F.lights[(size_t)li];
      light_record(o.trans, o.itrans, o.has_trans != 0u, &L);
      for (uint32_t t = 0; t < L.ntri; t++) {
        LightTri& lt = F.light_tris[(size_t)(L.tri_base - F.light_tri_first) + t];
        lt.area_term = light_area_term(L.pdfT, lt.v0, lt.v1, lt.v2);
      }
      break;
    }
  }
  if (any_inactive(B)) mask_top(built);              // (srt_pt_set_active: the build was over every posed box; the boxes are the masked fold)
}

std::string check_mesh_update(const BuiltScene& B, uint32_t object, uint32_t nverts) {
  const uint32_t nobj = (uint32_t)B.inputs.size();
  if (object >= nobj) return "object " + std::to_string(object) + " is out of range (the scene has " + std::to_string(nobj) + " objects)";
  const ObjectInput& in = B.inputs[object];
  if (in.kind != OBJ_MESH) return "object " + std::to_string(object) + " is a sphere, not a mesh added by srt_pt_add_mesh";
  if (in.source >= 0)
    return "object " + std::to_string(object) + " is an instance: update its source, object " + std::to_string(in.source) + ", and every instance follows";
  if (in.is_light && !B.dynamic_lights)
    return "object " + std::to_string(object) + " is an area light: its light-list copy and light tables depend on its vertices, commit the scene again";
  if ((size_t)nverts * 3 != in.mesh.pos.size())
    return "object " + std::to_string(object) + " was added with " + std::to_string(in.mesh.pos.size() / 3) + " vertices, not " + std::to_string(nverts);
  return "";
}

std::string prepare_mesh_update(const BuiltScene& B, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                                HostBVH* prebuilt, MeshUpdate* out, bool* bad_argument) {
  *bad_argument = true;
  const std::string refused = check_mesh_update(B, object, nverts);
  if (!refused.empty()) return refused;
  *bad_argument = false;
  const bool use_bvh = B.flat.use_bvh;
  const uint32_t nobj = (uint32_t)B.inputs.size();
  MeshUpdate& U = *out;
  U = MeshUpdate();
  U.object = object;
  U.pos.assign(pos, pos + 3 * (size_t)nverts);
  U.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  MeshInput m;                                     // the mesh as a fresh commit would be given it (the arrays are moved back out below)
  m.pos.swap(U.pos); m.nrm.swap(U.nrm);
  m.idx = B.inputs[object].mesh.idx;
  const uint32_t ntri = (uint32_t)m.idx.size() / 3;

  // Tri_Mesh::build (leaf size 4) or List<Triangle>, and the object-space box, as build_scene has them
  Box ob;
  if (use_bvh && prebuilt) {
    U.blas.nodes.swap(prebuilt->nodes);
    U.blas.prim.swap(prebuilt->prim);
  } else {
    std::vector<Box> tb(ntri);
    for (uint32_t t = 0; t < ntri; t++)
      tb[t] = triangle_box(&m.pos[3 * m.idx[3 * t]], &m.pos[3 * m.idx[3 * t + 1]], &m.pos[3 * m.idx[3 * t + 2]]);
    if (use_bvh) {
      if (!build_bvh(tb, 4, &U.blas))
        return "BVH<Triangle> build of object " + std::to_string(object) +
               " does not terminate (coincident centroids); the reference loops forever on this mesh";
    } else {
      for (const Box& b : tb) ob.enclose(b);  // List<Triangle>::bbox
    }
  }
  if (use_bvh) {
    const HostNode& root = U.blas.nodes[0];
    for (int a = 0; a < 3; a++) { ob.mn[a] = root.mn[a]; ob.mx[a] = root.mx[a]; }
    append_nodes(U.blas, &U.nodes);
    append_records(U.blas, blas_leaf_code, &U.recs);
    append_triangles(m, &U.blas.prim, &U.tris, &U.tri_nrm, &U.tri_packed);
  } else {
    append_triangles(m, nullptr, &U.tris, &U.tri_nrm, &U.tri_packed);
  }
  m.pos.swap(U.pos); m.nrm.swap(U.nrm);

  // the mesh and its instances take the new box and the new range lengths; what is stored behind the mesh moves by the difference
  // (a mesh has at least one node, so node_off orders the stored meshes)
  U.local_boxes = B.local_boxes;
  U.store = B.store;
  const MeshStore old = B.store[object];
  const int64_t dn = (int64_t)U.nodes.size() - (int64_t)old.nnodes, dr = (int64_t)U.recs.size() - (int64_t)old.nrec;
  U.max_blas_depth = interior_depth(U.blas);
  for (uint32_t i = 0; i < nobj; i++) {
    const ObjectInput& in = B.inputs[i];
    if (in.kind != OBJ_MESH) continue;
    if (i == object || in.source == (int32_t)object) {
      for (int a = 0; a < 3; a++) { U.local_boxes[6 * (size_t)i + a] = ob.mn[a]; U.local_boxes[6 * (size_t)i + 3 + a] = ob.mx[a]; }
      U.store[i].nnodes = (uint32_t)U.nodes.size();
      U.store[i].nrec = (uint32_t)U.recs.size();
    } else if (use_bvh && U.store[i].node_off > old.node_off) {
      U.store[i].node_off = (uint32_t)((int64_t)U.store[i].node_off + dn);
      U.store[i].rec_base = (uint32_t)((int64_t)U.store[i].rec_base + dr);
    }
    if (i != object && in.source < 0) U.max_blas_depth = std::max(U.max_blas_depth, interior_depth(B.blas[i]));
  }

  std::vector<Mat4> trans(nobj);
  for (uint32_t i = 0; i < nobj; i++) trans[i] = B.inputs[i].trans;
  Top T;
  if (!build_top(trans, U.local_boxes, use_bvh, &T)) return "BVH<Object> build does not terminate (coincident object centroids)";
  ReposedTop& R = U.top;
  make_objects(B.inputs, trans, T, U.store, (uint32_t)T.nodes.size(), use_bvh, &R.objects, &R.lazy_objects);
  make_wave_lazy(T.wave, R.objects, &R.wave_lazy);
  R.tlas.nodes.swap(T.tlas.nodes);
  R.tlas.prim.swap(T.tlas.prim);
  R.tlas_nodes.swap(T.nodes);
  R.wave_tlas.swap(T.wave);
  R.max_tlas_depth = T.depth;
  return "";
}

void apply_mesh_update(BuiltScene* built, MeshUpdate* update) {
  BuiltScene& B = *built;
  FlatScene& F = B.flat;
  MeshUpdate& U = *update;
  const MeshStore old = B.store[U.object];
  B.inputs[U.object].mesh.pos.swap(U.pos);
  B.inputs[U.object].mesh.nrm.swap(U.nrm);
  B.blas[U.object].nodes.swap(U.blas.nodes);
  B.blas[U.object].prim.swap(U.blas.prim);
  B.local_boxes.swap(U.local_boxes);
  B.store.swap(U.store);
  // the triangle range stays where it is
  std::copy(U.tris.begin(), U.tris.end(), F.tris.begin() + old.tri_base);
  std::copy(U.tri_nrm.begin(), U.tri_nrm.end(), F.tri_nrm.begin() + old.tri_base);
  std::copy(U.tri_packed.begin(), U.tri_packed.end(), F.tri_packed.begin() + 9 * (size_t)old.tri_base);
  if (F.use_bvh) {
    // records: [ .. the mesh's .. what lies behind ]
    std::vector<WaveInterior> recs(F.blas_recs.begin(), F.blas_recs.begin() + old.rec_base);
    recs.insert(recs.end(), U.recs.begin(), U.recs.end());
    recs.insert(recs.end(), F.blas_recs.begin() + old.rec_base + old.nrec, F.blas_recs.end());
    F.blas_recs.swap(recs);
    // nodes: [ new BVH<Object> | BVH<Triangle>s in front | the mesh's | those behind ]
    const size_t at = (size_t)F.tlas_nodes + old.node_off;
    std::vector<Node> nodes(U.top.tlas_nodes);
    nodes.insert(nodes.end(), F.nodes.begin() + F.tlas_nodes, F.nodes.begin() + at);
    nodes.insert(nodes.end(), U.nodes.begin(), U.nodes.end());
    nodes.insert(nodes.end(), F.nodes.begin() + at + old.nnodes, F.nodes.end());
    F.nodes.swap(nodes);
  }
  F.tlas_nodes = (uint32_t)U.top.tlas_nodes.size();
  F.max_tlas_depth = U.top.max_tlas_depth;
  F.max_blas_depth = U.max_blas_depth;
  F.wave_tlas.swap(U.top.wave_tlas);
  F.wave_lazy.swap(U.top.wave_lazy);
  F.lazy_objects.swap(U.top.lazy_objects);
  F.objects.swap(U.top.objects);
  B.tlas.nodes.swap(U.top.tlas.nodes);
  B.tlas.prim.swap(U.top.tlas.prim);
  const int32_t li = light_of(B, U.object);          // an emissive mesh (BuiltScene::dynamic_lights): its light-list copy and LightTri records
  if (li >= 0) write_light_mesh(built, (uint32_t)li, U.object);
  if (any_inactive(B)) mask_top(built);
}

void refit_boxes(const HostBVH& tree, const float* pos, const std::vector<uint32_t>& idx, std::vector<float>* boxes6) {
  const size_t nn = tree.nodes.size();
  std::vector<Box> nb(nn);
  for (size_t n = nn; n-- > 0;) {
    const HostNode& nd = tree.nodes[n];
    Box b;
    if (nd.l == nd.r) {
      for (uint32_t k = nd.start; k < nd.start + nd.size; k++) {
        const uint32_t t = tree.prim[k];
        b.enclose(triangle_box(&pos[3 * (size_t)idx[3 * (size_t)t]], &pos[3 * (size_t)idx[3 * (size_t)t + 1]], &pos[3 * (size_t)idx[3 * (size_t)t + 2]]));
      }
    } else {
      b.enclose(nb[nd.l]);
      b.enclose(nb[nd.r]);
    }
    nb[n] = b;
  }
  boxes6->resize(6 * nn);
  for (size_t n = 0; n < nn; n++)
    for (int a = 0; a < 3; a++) { (*boxes6)[6 * n + a] = nb[n].mn[a]; (*boxes6)[6 * n + 3 + a] = nb[n].mx[a]; }
}

// What both refits of a mesh start with: the refusals, then the new arrays, the node boxes and every object's object-space box.
static std::string mesh_refit_head(const BuiltScene& B, uint32_t object, const float* pos, const float* nrm, uint32_t nverts, const float* node_boxes,
                                   bool refuse_non_finite, MeshRefit* out) {
  const std::string refused = check_mesh_update(B, object, nverts);
  if (!refused.empty()) return refused;
  if (!B.flat.use_bvh) return "the scene was committed without BVHs: there is no tree to refit";
  if (refuse_non_finite)
    for (size_t k = 0; k < 3 * (size_t)nverts; k++)
      if (!std::isfinite(pos[k]))
        return "vertex " + std::to_string(k / 3) + " of the new positions has a non-finite coordinate";
  const uint32_t nobj = (uint32_t)B.inputs.size();
  MeshRefit& R = *out;
  R = MeshRefit();
  R.object = object;
  R.pos.assign(pos, pos + 3 * (size_t)nverts);
  R.nrm.assign(nrm, nrm + 3 * (size_t)nverts);
  const HostBVH& tree = B.blas[object];
  if (node_boxes) R.boxes.assign(node_boxes, node_boxes + 6 * tree.nodes.size());
  else refit_boxes(tree, pos, B.inputs[object].mesh.idx, &R.boxes);
  // the mesh and its instances take the new root box; storage does not move
  R.local_boxes = B.local_boxes;
  for (uint32_t i = 0; i < nobj; i++)
    if (i == object || (B.inputs[i].kind == OBJ_MESH && B.inputs[i].source == (int32_t)object))
      for (int a = 0; a < 6; a++) R.local_boxes[6 * (size_t)i + a] = R.boxes[a];
  return "";
}

std::string prepare_mesh_refit(const BuiltScene& B, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                               const float* node_boxes, MeshRefit* out, bool* bad_argument) {
  *bad_argument = true;
  const std::string refused = mesh_refit_head(B, object, pos, nrm, nverts, node_boxes, true, out);
  if (!refused.empty()) return refused;
  *bad_argument = false;
  const uint32_t nobj = (uint32_t)B.inputs.size();
  MeshRefit& R = *out;
  std::vector<Mat4> trans(nobj);
  for (uint32_t i = 0; i < nobj; i++) trans[i] = B.inputs[i].trans;
  Top T;
  if (!build_top(trans, R.local_boxes, true, &T)) return "BVH<Object> build does not terminate (coincident object centroids)";
  ReposedTop& P = R.top;
  make_objects(B.inputs, trans, T, B.store, (uint32_t)T.nodes.size(), true, &P.objects, &P.lazy_objects);
  make_wave_lazy(T.wave, P.objects, &P.wave_lazy);
  P.tlas.nodes.swap(T.tlas.nodes);
  P.tlas.prim.swap(T.tlas.prim);
  P.tlas_nodes.swap(T.nodes);
  P.wave_tlas.swap(T.wave);
  P.max_tlas_depth = T.depth;
  return "";
}

// The mesh's own half of a refit, in place: the vertex arrays, the object-space boxes, the BVH<Triangle>'s boxes on both sides, the
// interior records, the triangle records in the kept order and the light-list copy.  (A rebuilt BVH<Object> is in by now: the
// BVH<Triangle> nodes are written behind it.)
static void write_mesh_refit(BuiltScene* built, MeshRefit* refit) {
  BuiltScene& B = *built;
  FlatScene& F = B.flat;
  MeshRefit& R = *refit;
  const MeshStore m = B.store[R.object];
  MeshInput& mesh = B.inputs[R.object].mesh;
  HostBVH& tree = B.blas[R.object];
  for (size_t n = 0; n < tree.nodes.size(); n++) {
    HostNode& h = tree.nodes[n];
    Node& f = F.nodes[(size_t)F.tlas_nodes + m.node_off + n];
    for (int a = 0; a < 3; a++) { h.mn[a] = f.mn[a] = R.boxes[6 * n + a]; h.mx[a] = f.mx[a] = R.boxes[6 * n + 3 + a]; }
  }
  // interior records in node order, as append_records numbers them: both child boxes, nothing else
  size_t q = m.rec_base;
  for (const HostNode& h : tree.nodes) {
    if (h.l == h.r) continue;
    WaveInterior& wi = F.blas_recs[q++];
    for (int a = 0; a < 6; a++) { wi.boxl[a] = R.boxes[6 * (size_t)h.l + a]; wi.boxr[a] = R.boxes[6 * (size_t)h.r + a]; }
  }
  // triangle records in the kept primitive order
  std::vector<Tri> tris;
  std::vector<TriNrm> tri_nrm;
  std::vector<float> packed;
  append_triangles(mesh, &tree.prim, &tris, &tri_nrm, &packed);
  std::copy(tris.begin(), tris.end(), F.tris.begin() + m.tri_base);
  std::copy(tri_nrm.begin(), tri_nrm.end(), F.tri_nrm.begin() + m.tri_base);
  std::copy(packed.begin(), packed.end(), F.tri_packed.begin() + 9 * (size_t)m.tri_base);
  const int32_t li = light_of(B, R.object);          // an emissive mesh (BuiltScene::dynamic_lights): its light-list copy and LightTri records
  if (li >= 0) write_light_mesh(built, (uint32_t)li, R.object);
}

void apply_mesh_refit(BuiltScene* built, MeshRefit* refit) {
  MeshRefit& R = *refit;
  MeshInput& mesh = built->inputs[R.object].mesh;
  mesh.pos.swap(R.pos);
  mesh.nrm.swap(R.nrm);
  built->local_boxes.swap(R.local_boxes);
  apply_repose(built, &R.top);                     // the BVH<Object> and the tables of object order; the BVH<Triangle> nodes stay behind it
  write_mesh_refit(built, refit);
}

std::string prepare_mesh_refit_inplace(const BuiltScene& B, uint32_t object, const float* pos, const float* nrm, uint32_t nverts,
                                       const float* node_boxes, bool refuse_non_finite, MeshRefit* out) {
  const std::string refused = mesh_refit_head(B, object, pos, nrm, nverts, node_boxes, refuse_non_finite, out);
  if (!refused.empty()) return refused;
  // Object::bbox of every object from its unchanged transform and its object-space box, masked by the active table, folded
  // through the kept tree
  const size_t nobj = B.inputs.size();
  std::vector<float> posed(6 * nobj);
  for (size_t i = 0; i < nobj; i++) {
    Mat4 itrans;
    uint32_t has_trans;
    posed_values(B.inputs[i].trans, &out->local_boxes[6 * i], &itrans, &has_trans, &posed[6 * i]);
  }
  effective_boxes(B, &posed);
  top_refit_boxes(B.tlas, posed.data(), &out->top_boxes);
  return "";
}

void apply_mesh_refit_inplace(BuiltScene* built, MeshRefit* refit) {
  MeshRefit& R = *refit;
  MeshInput& mesh = built->inputs[R.object].mesh;
  mesh.pos.swap(R.pos);
  mesh.nrm.swap(R.nrm);
  built->local_boxes.swap(R.local_boxes);
  write_mesh_refit(built, refit);
  write_top_boxes(built, R.top_boxes);
  if (any_inactive(*built)) write_top_counts(built);
}

void top_refit_boxes(const HostBVH& tree, const float* posed, std::vector<float>* boxes6) {
  const size_t nn = tree.nodes.size();
  std::vector<Box> nb(nn);
  for (size_t n = nn; n-- > 0;) {                    // children lie behind their parent: one backward pass
    const HostNode& nd = tree.nodes[n];
    Box b;
    if (nd.l == nd.r) {
      for (uint32_t k = nd.start; k < nd.start + nd.size; k++) {
        Box ob;
        for (int a = 0; a < 3; a++) { ob.mn[a] = posed[6 * (size_t)tree.prim[k] + a]; ob.mx[a] = posed[6 * (size_t)tree.prim[k] + 3 + a]; }
        b.enclose(ob);
      }
    } else {
      b.enclose(nb[nd.l]);
      b.enclose(nb[nd.r]);
    }
    nb[n] = b;
  }
  boxes6->resize(6 * nn);
  for (size_t n = 0; n < nn; n++)
    for (int a = 0; a < 3; a++) { (*boxes6)[6 * n + a] = nb[n].mn[a]; (*boxes6)[6 * n + 3 + a] = nb[n].mx[a]; }
}

std::string prepare_top_refit(const BuiltScene& B, const uint32_t* objects, const Mat4* new_trans, uint32_t n, TopRefit* out) {
  const std::string refused = check_repose_list(B, objects, n);
  if (!refused.empty()) return refused;
  const uint32_t nobj = (uint32_t)B.inputs.size();
  TopRefit& R = *out;
  R = TopRefit();
  R.listed.assign(objects, objects + n);
  R.trans.assign(new_trans, new_trans + n);
  R.itrans.resize(n);
  R.has_trans.resize(n);
  // Object::bbox of every object: the listed ones under their new transforms, the others under the committed ones
  std::vector<float> posed(6 * (size_t)nobj);
  std::vector<bool> listed(nobj, false);
  for (uint32_t k = 0; k < n; k++) {
    listed[objects[k]] = true;
    posed_values(new_trans[k], &B.local_boxes[6 * (size_t)objects[k]], &R.itrans[k], &R.has_trans[k], &posed[6 * (size_t)objects[k]]);
  }
  if (!B.flat.use_bvh) return "";
  for (uint32_t i = 0; i < nobj; i++) {
    if (listed[i]) continue;
    Mat4 itrans;
    uint32_t has_trans;
    posed_values(B.inputs[i].trans, &B.local_boxes[6 * (size_t)i], &itrans, &has_trans, &posed[6 * (size_t)i]);
  }
  effective_boxes(B, &posed);
  top_refit_boxes(B.tlas, posed.data(), &R.boxes);
  return "";
}

void apply_top_refit(BuiltScene* built, TopRefit* refit) {
  BuiltScene& B = *built;
  FlatScene& F = B.flat;
  TopRefit& R = *refit;
  std::vector<uint32_t> slot_of(B.tlas.prim.size());
  for (size_t s = 0; s < B.tlas.prim.size(); s++) slot_of[B.tlas.prim[s]] = (uint32_t)s;
  for (size_t k = 0; k < R.listed.size(); k++) {
    const uint32_t i = R.listed[k];
    B.inputs[i].trans = R.trans[k];
    Object& o = F.objects[slot_of[i]];
    o.trans = R.trans[k];
    o.itrans = R.itrans[k];
    o.has_trans = R.has_trans[k];
    // a listed area light (BuiltScene::dynamic_lights): its record and area terms, as apply_repose gives them
    const int32_t li = B.inputs[i].is_light ? light_of(B, i) : -1;
    if (li < 0) continue;
    Light& L = F.lights[(size_t)li];
    light_record(o.trans, o.itrans, o.has_trans != 0u, &L);
    for (uint32_t t = 0; t < L.ntri; t++) {
      LightTri& lt = F.light_tris[(size_t)(L.tri_base - F.light_tri_first) + t];
      lt.area_term = light_area_term(L.pdfT, lt.v0, lt.v1, lt.v2);
    }
  }
  if (F.use_bvh) write_top_boxes(built, R.boxes);
}

void write_top_boxes(BuiltScene* built, const std::vector<float>& boxes6) {
  FlatScene& F = built->flat;
  HostBVH& tree = built->tlas;
  for (size_t n = 0; n < tree.nodes.size(); n++) {
    HostNode& h = tree.nodes[n];
    Node& f = F.nodes[n];
    for (int a = 0; a < 3; a++) { h.mn[a] = f.mn[a] = boxes6[6 * n + a]; h.mx[a] = f.mx[a] = boxes6[6 * n + 3 + a]; }
  }
  // sweep records in node order, as append_records numbers them: both child boxes, nothing else
  size_t q = 0;
  for (const HostNode& h : tree.nodes) {
    if (h.l == h.r) continue;
    WaveInterior& wi = F.wave_tlas[q++];
    for (int a = 0; a < 6; a++) { wi.boxl[a] = boxes6[6 * (size_t)h.l + a]; wi.boxr[a] = boxes6[6 * (size_t)h.r + a]; }
  }
}

bool any_inactive(const BuiltScene& B) {
  return std::find(B.active.begin(), B.active.end(), (uint8_t)0) != B.active.end();
}

void effective_boxes(const BuiltScene& B, std::vector<float>* posed6) {
  const Box empty;
  for (size_t i = 0; i < B.active.size(); i++)
    if (!B.active[i])
      for (int a = 0; a < 3; a++) { (*posed6)[6 * i + a] = empty.mn[a]; (*posed6)[6 * i + 3 + a] = empty.mx[a]; }
}

void posed_boxes(const BuiltScene& B, std::vector<float>* posed6) {
  const size_t nobj = B.inputs.size();
  posed6->resize(6 * nobj);
  for (size_t i = 0; i < nobj; i++) {
    Mat4 itrans;
    uint32_t has_trans;
    posed_values(B.inputs[i].trans, &B.local_boxes[6 * i], &itrans, &has_trans, &(*posed6)[6 * i]);
  }
}

void write_top_counts(BuiltScene* built) {
  FlatScene& F = built->flat;
  if (!F.use_bvh) return;
  const HostBVH& tree = built->tlas;
  // what a leaf holds for the walks: its primitives, or nothing while every one of them is inactive (the BVH<Object>'s leaves hold 0 or 1)
  auto held = [&](const HostNode& h) {
    for (uint32_t k = h.start; k < h.start + h.size; k++)
      if (built->active[tree.prim[k]]) return h.size;
    return 0u;
  };
  size_t q = 0;
  for (size_t n = 0; n < tree.nodes.size(); n++) {
    const HostNode& h = tree.nodes[n];
    if (h.l == h.r) { F.nodes[n].count = LEAF_BIT | held(h); continue; }
    WaveInterior& wi = F.wave_tlas[q++];               // (numbered in node order, as append_records numbers them)
    const HostNode &a = tree.nodes[h.l], &c = tree.nodes[h.r];
    if (a.l == a.r) wi.l_cnt = held(a);
    if (c.l == c.r) wi.r_cnt = held(c);
  }
}

void mask_top(BuiltScene* built) {
  if (!built->flat.use_bvh) return;
  std::vector<float> posed, boxes;
  posed_boxes(*built, &posed);
  effective_boxes(*built, &posed);
  top_refit_boxes(built->tlas, posed.data(), &boxes);
  write_top_boxes(built, boxes);
  write_top_counts(built);
}

std::string check_active_list(const BuiltScene& B, const uint32_t* objects, uint32_t n, bool* unsupported) {
  *unsupported = true;
  if (!B.flat.use_bvh) return "the scene was committed without BVHs: there are no boxes to hide an object behind";
  if (B.tlas.nodes.size() < 2) return "the root of the BVH<Object> is a leaf, and the root's box is never tested: an object alone in its scene cannot be hidden";
  *unsupported = false;
  const uint32_t nobj = (uint32_t)B.inputs.size();
  std::vector<bool> seen(nobj, false);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t i = objects[k];
    if (i >= nobj) return "object " + std::to_string(i) + " is out of range (the scene has " + std::to_string(nobj) + " objects)";
    if (seen[i]) return "object " + std::to_string(i) + " is listed twice";
    if (B.inputs[i].is_light) return "object " + std::to_string(i) + " is an area light: the light list would go on sampling it";
    seen[i] = true;
  }
  return "";
}

bool apply_set_active(BuiltScene* built, const uint32_t* objects, const uint8_t* active, uint32_t n) {
  bool changed = false;
  for (uint32_t k = 0; k < n; k++) {
    const uint8_t a = active[k] ? 1 : 0;
    if (built->active[objects[k]] != a) { built->active[objects[k]] = a; changed = true; }
  }
  if (changed) mask_top(built);
  return changed;
}

double tree_cost(const HostBVH& tree) {
  if (tree.nodes.empty()) return 0.0;
  auto empty = [](const HostNode& h) { return h.mn[0] > h.mx[0] || h.mn[1] > h.mx[1] || h.mn[2] > h.mx[2]; };   // (nothing active below)
  auto area = [&](const HostNode& h) {
    if (empty(h)) return 0.0;
    const double x = (double)h.mx[0] - (double)h.mn[0], y = (double)h.mx[1] - (double)h.mn[1], z = (double)h.mx[2] - (double)h.mn[2];
    return 2.0 * (x * y + y * z + z * x);
  };
  if (empty(tree.nodes[0])) return 0.0;
  const double root = area(tree.nodes[0]);
  double cost = 0.0;
  for (const HostNode& h : tree.nodes) cost += (h.l == h.r ? (double)h.size : 1.0) * (area(h) / root);
  return cost;
}

}  // namespace srt
