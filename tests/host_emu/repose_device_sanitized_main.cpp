// Stand-alone check of srt_pt_repose_device's scene layer (pt_scene.cpp alone; tests/test_pt_repose_device_host.py builds it
// with -fsanitize=address,undefined and runs it once): prepare_repose_supplied - the per-object values supplied by the caller
// instead of computed - against prepare_repose on the scene and the list of the file given as argv[1], with the posed boxes and
// with a tree built beforehand, in a scene with BVHs and in a list scene; and refused lists, which leave the scene alone.
//
// File (little endian, 32-bit words): nmat, then per material {type, a[3], b[3], ior}; nobj, then per object {kind (0 mesh,
// 1 sphere, 2 instance), is_light, material, source, radius, T[16], nverts, nidx, pos[3 nverts], nrm[3 nverts], idx[nidx]};
// n, then n insertion indices and n transforms of 16 floats.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_scene.h"

using namespace srt;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

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

template <class V>
static bool same_bytes(const V& a, const V& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

static bool same_top(const ReposedTop& a, const ReposedTop& b) {
  return a.listed == b.listed && same_bytes(a.trans, b.trans) && same_bytes(a.tlas.nodes, b.tlas.nodes) && a.tlas.prim == b.tlas.prim &&
         same_bytes(a.tlas_nodes, b.tlas_nodes) && a.max_tlas_depth == b.max_tlas_depth && same_bytes(a.wave_tlas, b.wave_tlas) &&
         a.wave_lazy == b.wave_lazy && a.lazy_objects == b.lazy_objects && same_bytes(a.objects, b.objects);
}

static bool same_scene(const BuiltScene& a, const BuiltScene& b) {
  if (a.inputs.size() != b.inputs.size()) return false;
  for (size_t i = 0; i < a.inputs.size(); i++)
    if (std::memcmp(&a.inputs[i].trans, &b.inputs[i].trans, sizeof(Mat4)) != 0) return false;
  return same_bytes(a.flat.nodes, b.flat.nodes) && same_bytes(a.flat.objects, b.flat.objects) && same_bytes(a.flat.wave_tlas, b.flat.wave_tlas) &&
         a.flat.wave_lazy == b.flat.wave_lazy && a.flat.lazy_objects == b.flat.lazy_objects && same_bytes(a.tlas.nodes, b.tlas.nodes) &&
         a.tlas.prim == b.tlas.prim && a.flat.tlas_nodes == b.flat.tlas_nodes && a.flat.max_tlas_depth == b.flat.max_tlas_depth;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s scene-file\n", argv[0]); return 2; }
  Reader R;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) R.bytes.insert(R.bytes.end(), buf, buf + got);
    std::fclose(f);
  }
  std::vector<Material> mats(R.u32());
  for (Material& m : mats) {
    std::memset(&m, 0, sizeof m);
    m.type = R.u32();
    for (float& v : m.a) v = R.f32();
    for (float& v : m.b) v = R.f32();
    m.ior = R.f32();
  }
  std::vector<ObjectInput> inputs(R.ok ? R.u32() : 0);
  for (ObjectInput& o : inputs) {
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
  std::vector<uint32_t> listed;
  std::vector<Mat4> moved;
  R.array(&listed, n);
  R.array(&moved, n);
  if (!R.ok || R.at != R.bytes.size() || inputs.empty() || !n) { std::printf("cannot read %s\n", argv[1]); return 2; }
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
    EXPECT(same_scene(S, first));                        // preparing leaves the scene alone
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
    EXPECT(same_scene(S, first));
    // applied: the scene of a fresh build on the new poses, and of srt_pt_repose's path
    BuiltScene H = S, fresh;
    apply_repose(&S, &from_boxes);
    apply_repose(&H, &want);
    std::vector<ObjectInput> posed_inputs = inputs;
    for (uint32_t i = 0; i < nobj; i++) posed_inputs[i].trans = all[i];
    EXPECT(build_scene(posed_inputs, mats, use_bvh != 0, &fresh).empty());
    EXPECT(same_scene(S, H) && same_scene(S, fresh));
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
    EXPECT(same_scene(S, first));
  }
  if (failures) return 1;
  std::printf("repose_device_sanitized: ok (%u objects, %u listed)\n", nobj, n);
  return 0;
}
