// What the stand-alone sanitizer programs over the scene layer (tests/host_emu/*_sanitized_main.cpp) share: the EXPECT count, the
// small scenes they commit, the scene-file loader and the byte comparisons.  Each program keeps its own check_* functions and main.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_scene.h"

using namespace srt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static inline Mat4 pose(float s, float x, float y, float z) {
  Mat4 m = mat_identity();
  m.c[0][0] = m.c[1][1] = m.c[2][2] = s;
  m.c[3][0] = x; m.c[3][1] = y; m.c[3][2] = z;
  return m;
}

// n x n quads over [0,1]^2 lifted by amp * a ripple of `waves` periods: 2 n^2 triangles whose tree depends on amp and waves
// (amp == 0: a flat sheet, every triangle box widened by +1).
static inline MeshInput sheet(int n, float amp, float waves) {
  MeshInput m;
  for (int j = 0; j <= n; j++)
    for (int i = 0; i <= n; i++) {
      const float x = (float)i / n, z = (float)j / n;
      const float p[3] = {x, amp * std::sin(6.2831853f * waves * x) * std::cos(6.2831853f * waves * z), z};
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

// 0: an area light; 1: sheet A; 2: sheet B; 3, 4: instances of A; 5: an instance of B; 6: a sphere
static inline std::vector<ObjectInput> scene(const MeshInput& A, const MeshInput& B) {
  std::vector<ObjectInput> in;
  ObjectInput light;
  light.trans = pose(0.5f, 0.0f, 2.0f, 0.0f);
  light.material = 1; light.is_light = true; light.mesh = sheet(1, 0.0f, 1.0f);
  in.push_back(light);
  ObjectInput a; a.trans = mat_identity(); a.mesh = A; in.push_back(a);
  ObjectInput b; b.trans = pose(0.7f, 1.5f, 0.2f, -0.4f); b.mesh = B; in.push_back(b);
  ObjectInput i1; i1.trans = pose(0.3f, -1.0f, 0.5f, 0.8f); i1.source = 1; in.push_back(i1);
  ObjectInput i2; i2.trans = pose(0.6f, 0.2f, -1.1f, 1.9f); i2.source = 1; in.push_back(i2);
  ObjectInput i3; i3.trans = pose(0.4f, -2.0f, 0.1f, -1.2f); i3.source = 2; in.push_back(i3);
  ObjectInput s; s.kind = OBJ_SPHERE; s.radius = 0.2f; s.trans = pose(1.0f, -1.0f, 1.5f, 0.3f); in.push_back(s);
  return in;
}

// 0: a grey Lambertian; 1: an emitter
static inline std::vector<Material> two_materials() {
  std::vector<Material> mats(2);
  std::memset(mats.data(), 0, 2 * sizeof(Material));
  mats[0].a[0] = mats[0].a[1] = mats[0].a[2] = 0.5f;
  mats[1].type = 3; mats[1].a[0] = mats[1].a[1] = mats[1].a[2] = 5.0f;
  return mats;
}

template <class V>
static inline bool same_bytes(const V& a, const V& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

static inline bool same_tree(const HostBVH& a, const HostBVH& b) { return same_bytes(a.nodes, b.nodes) && a.prim == b.prim; }

// Everything a kernel reads that does not depend on where a mesh is stored: the ranges may lie elsewhere, their contents may not differ.
static inline bool same_contents(const FlatScene& a, const FlatScene& b) {
  if (a.tlas_nodes != b.tlas_nodes || a.objects.size() != b.objects.size() || a.wave_tlas.size() != b.wave_tlas.size() ||
      a.wave_lazy != b.wave_lazy || a.lazy_objects != b.lazy_objects || a.max_tlas_depth != b.max_tlas_depth)
    return false;
  if (a.tlas_nodes && std::memcmp(a.nodes.data(), b.nodes.data(), a.tlas_nodes * sizeof(Node)) != 0) return false;
  if (!a.wave_tlas.empty() && std::memcmp(a.wave_tlas.data(), b.wave_tlas.data(), a.wave_tlas.size() * sizeof(WaveInterior)) != 0) return false;
  for (size_t k = 0; k < a.objects.size(); k++) {
    const Object &x = a.objects[k], &y = b.objects[k];
    if (x.kind != y.kind || x.has_trans != y.has_trans || x.material != y.material || x.use_bvh != y.use_bvh || x.id != y.id ||
        x.ntri != y.ntri || x.nnodes != y.nnodes || x.nrec != y.nrec || std::memcmp(&x.trans, &y.trans, 2 * sizeof(Mat4)) != 0)
      return false;
    for (uint32_t t = 0; t < x.ntri; t++)
      if (std::memcmp(&a.tris[x.tri_base + t], &b.tris[y.tri_base + t], sizeof(Tri)) != 0 ||
          std::memcmp(&a.tri_nrm[x.tri_base + t], &b.tri_nrm[y.tri_base + t], sizeof(TriNrm)) != 0 ||
          std::memcmp(&a.tri_packed[9 * (size_t)(x.tri_base + t)], &b.tri_packed[9 * (size_t)(y.tri_base + t)], 9 * sizeof(float)) != 0)
        return false;
    for (uint32_t r = 0; r < x.nrec; r++)
      if (std::memcmp(&a.blas_recs[x.rec_base + r], &b.blas_recs[y.rec_base + r], sizeof(WaveInterior)) != 0) return false;
    for (uint32_t n = 0; n < x.nnodes; n++)
      if (std::memcmp(&a.nodes[x.node_base + n], &b.nodes[y.node_base + n], sizeof(Node)) != 0) return false;
  }
  return true;
}

// What a pose or the active table decides, byte for byte: every object's transform, the BVH<Object> on both sides, the tables of
// object order, the light tables and the active table.
static inline bool same_posed_scene(const BuiltScene& a, const BuiltScene& b) {
  if (a.inputs.size() != b.inputs.size()) return false;
  for (size_t i = 0; i < a.inputs.size(); i++)
    if (std::memcmp(&a.inputs[i].trans, &b.inputs[i].trans, sizeof(Mat4)) != 0) return false;
  return same_bytes(a.flat.nodes, b.flat.nodes) && same_bytes(a.flat.objects, b.flat.objects) && same_bytes(a.flat.wave_tlas, b.flat.wave_tlas) &&
         a.flat.wave_lazy == b.flat.wave_lazy && a.flat.lazy_objects == b.flat.lazy_objects && same_tree(a.tlas, b.tlas) &&
         a.flat.tlas_nodes == b.flat.tlas_nodes && a.flat.max_tlas_depth == b.flat.max_tlas_depth && same_bytes(a.flat.lights, b.flat.lights) &&
         same_bytes(a.flat.light_tris, b.flat.light_tris) && a.active == b.active;
}

// Byte for byte: host trees, inputs, the active table and every flattened array.
static inline bool identical(const BuiltScene& A, const BuiltScene& B) {
  const FlatScene &a = A.flat, &b = B.flat;
  if (!same_bytes(a.nodes, b.nodes) || !same_bytes(a.tris, b.tris) || !same_bytes(a.tri_nrm, b.tri_nrm) || a.tri_packed != b.tri_packed ||
      !same_bytes(a.objects, b.objects) || !same_bytes(a.wave_tlas, b.wave_tlas) || !same_bytes(a.blas_recs, b.blas_recs) || a.wave_lazy != b.wave_lazy ||
      a.lazy_objects != b.lazy_objects || a.tlas_nodes != b.tlas_nodes || a.max_tlas_depth != b.max_tlas_depth || a.max_blas_depth != b.max_blas_depth)
    return false;
  if (A.local_boxes != B.local_boxes || !same_tree(A.tlas, B.tlas) || A.blas.size() != B.blas.size() || A.active != B.active) return false;
  for (size_t i = 0; i < A.blas.size(); i++)
    if (!same_tree(A.blas[i], B.blas[i]) || A.inputs[i].mesh.pos != B.inputs[i].mesh.pos || A.inputs[i].mesh.nrm != B.inputs[i].mesh.nrm)
      return false;
  return true;
}

struct Reader {
  std::vector<unsigned char> bytes;
  size_t at = 0;
  bool ok = true;
  void read(void* dst, size_t n) {
    if (at + n > bytes.size()) { ok = false; std::memset(dst, 0, n); return; }
    std::memcpy(dst, bytes.data() + at, n);
    at += n;
  }
  uint32_t u32() { uint32_t v; read(&v, 4); return v; }
  float f32() { float v; read(&v, 4); return v; }
  template <class T> void array(std::vector<T>* v, size_t n) {
    if (at + n * sizeof(T) > bytes.size()) { ok = false; return; }
    v->resize(n);
    if (n) read(v->data(), n * sizeof(T));
  }
};

// A scene and a repose list from a file (tests/_repose_device_cases.py:write_scene_file), little endian, 32-bit words: nmat, then
// per material {type, a[3], b[3], ior}; nobj, then per object {kind (0 mesh, 1 sphere, 2 instance), is_light, material, source,
// radius, T[16], nverts, nidx, pos[3 nverts], nrm[3 nverts], idx[nidx]}; n, then n insertion indices and n transforms of 16 floats.
// False unless the whole file was read and was all of it.
static inline bool load_scene_file(const char* path, std::vector<Material>* mats, std::vector<ObjectInput>* inputs, std::vector<uint32_t>* listed,
                                   std::vector<Mat4>* moved) {
  Reader R;
  if (FILE* f = std::fopen(path, "rb")) {
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) R.bytes.insert(R.bytes.end(), buf, buf + got);
    std::fclose(f);
  }
  mats->resize(R.u32());
  for (Material& m : *mats) {
    std::memset(&m, 0, sizeof m);
    m.type = R.u32();
    for (float& v : m.a) v = R.f32();
    for (float& v : m.b) v = R.f32();
    m.ior = R.f32();
  }
  inputs->resize(R.ok ? R.u32() : 0);
  for (ObjectInput& o : *inputs) {
    const uint32_t kind = R.u32();
    o.kind = kind == 1u ? OBJ_SPHERE : OBJ_MESH;
    o.is_light = R.u32() != 0u;
    o.material = R.u32();
    const uint32_t source = R.u32();
    o.source = kind == 2u ? (int32_t)source : -1;
    o.radius = R.f32();
    R.read(&o.trans, sizeof(Mat4));
    const uint32_t nverts = R.u32(), nidx = R.u32();
    R.array(&o.mesh.pos, 3 * (size_t)nverts);
    R.array(&o.mesh.nrm, 3 * (size_t)nverts);
    R.array(&o.mesh.idx, nidx);
    if (!R.ok) break;
  }
  const uint32_t n = R.ok ? R.u32() : 0;
  R.array(listed, n);
  R.array(moved, n);
  return R.ok && R.at == R.bytes.size();
}
