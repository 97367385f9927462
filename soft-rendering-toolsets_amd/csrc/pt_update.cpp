// The path tracer's host side after srt_pt_scene_commit: what the units that change or query a committed scene share (pt_update.h) -
// the device writes more than one of them makes, settle() and what goes with it, where the BVH builds go - and srt_pt_scene_counts.
// The jobs themselves: pt_update_mesh.cpp (new vertices), pt_update_skin.cpp (skins and rigs), pt_update_pose.cpp (poses, object
// timelines) and pt_update_shading.cpp (materials, delta lights, shading timelines).  Host code only, as all of them are.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pt_light_update.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

namespace srt {

// Nothing is in flight any more: epochs the caller enqueued on streams of its own read the arrays that are about to change.
hipError_t quiesce(srt_pt* pt) {
  hipError_t e;
  if ((e = hipSetDevice(pt->device)) != hipSuccess || (e = hipStreamSynchronize(pt->stream)) != hipSuccess) return e;
  return hipDeviceSynchronize();
}

// The index buffer of mesh `object` on the device.  Every mesh that can be updated has its own from the commit on; an emissive
// mesh has it from the commit only when srt_pt_set_dynamic_lights was on by then - otherwise it is appended here, at the light's
// first update, refit or skin.  Nothing a render kernel reads; the caller has waited for whatever reads d_idx.
int ensure_mesh_idx(srt_pt* pt, uint32_t object) {
  if (pt->mesh.idx_off[object] != SIZE_MAX) return SRT_OK;
  const std::vector<uint32_t>& idx = pt->built.inputs[object].mesh.idx;
  DeviceBuffer<uint32_t> fresh;
  int st;
  if ((st = fresh.ensure(pt->mesh.idx_words + idx.size()))) return st;
  if ((pt->mesh.idx_words && hipMemcpy(fresh, pt->mesh.d_idx, pt->mesh.idx_words * sizeof(uint32_t), hipMemcpyDeviceToDevice) != hipSuccess) ||
      hipMemcpy(fresh + pt->mesh.idx_words, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    return srt::fail(SRT_ERR_HIP, "index buffer of object %u: device copy failed", object);
  pt->mesh.d_idx = std::move(fresh);                      // (frees the old array)
  pt->mesh.idx_off[object] = pt->mesh.idx_words;
  pt->mesh.idx_words += idx.size();
  pt->mesh.idx_uncounted += idx.size() * sizeof(uint32_t);
  return SRT_OK;
}

// Host forms of the dynamic-light calls (srt_pt_repose, srt_pt_update_mesh, srt_pt_refit_mesh): the light's record and its
// LightTri records from the host mirror, and - after new vertices - its light-list triangle copies.  The device forms run the
// kernels of pt_light_update.hip instead and upload none of this.
int upload_light(srt_pt* pt, uint32_t li, bool triangles) {
  const FlatScene& F = pt->built.flat;
  const Light& L = F.lights[li];
  const size_t lt = (size_t)(L.tri_base - F.light_tri_first), n = L.ntri;
  SRT_HIP(hipMemcpy(pt->d_lights + li, &L, sizeof(Light), hipMemcpyHostToDevice));
  if (n) SRT_HIP(hipMemcpy(pt->d_ltris + lt, &F.light_tris[lt], n * sizeof(LightTri), hipMemcpyHostToDevice));
  pt->bytes_uploaded += sizeof(Light) + n * sizeof(LightTri);
  if (triangles && n) {
    SRT_HIP(hipMemcpy(pt->d_tris + L.tri_base, &F.tris[L.tri_base], n * sizeof(Tri), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->d_nrm + L.tri_base, &F.tri_nrm[L.tri_base], n * sizeof(TriNrm), hipMemcpyHostToDevice));
    SRT_HIP(hipMemcpy(pt->d_tri_packed + 9 * (size_t)L.tri_base, &F.tri_packed[9 * (size_t)L.tri_base], 9 * n * sizeof(float), hipMemcpyHostToDevice));
    const uint64_t bytes = n * (sizeof(Tri) + sizeof(TriNrm) + 9 * sizeof(float));
    pt->bytes_uploaded += bytes;
    pt->tri_bytes_uploaded += bytes;
  }
  return SRT_OK;
}

// The BVH<Object>'s nodes after the scene layer replaced them.  With their count unchanged the BVH<Triangle> nodes behind them have
// not moved: the first tlas_nodes nodes are copied in place, enqueued on `s`.  Otherwise all of d_nodes goes up anew, once what
// `s` holds is done with the old array.
int write_top_level(srt_pt* pt, hipStream_t s, size_t old_tlas_nodes) {
  const FlatScene& F = pt->built.flat;
  if (F.tlas_nodes != old_tlas_nodes) {
    SRT_HIP(hipStreamSynchronize(s));
    return upload(pt, &pt->d_nodes, F.nodes);
  }
  if (F.tlas_nodes) SRT_HIP(hipMemcpyAsync(pt->d_nodes, F.nodes.data(), (size_t)F.tlas_nodes * sizeof(Node), hipMemcpyHostToDevice, s));
  pt->bytes_uploaded += (uint64_t)F.tlas_nodes * sizeof(Node);
  return SRT_OK;
}

// The tables in object order after the scene layer replaced them: the sweep records, which of their children hold a real
// BVH<Triangle> and - unless a kernel has gathered them in place - the object records.  Nothing may be reading the old ones.
int upload_object_tables(srt_pt* pt, bool records) {
  const FlatScene& F = pt->built.flat;
  int st;
  if ((records && (st = upload(pt, &pt->d_objects, F.objects))) || (st = upload(pt, &pt->d_wave, F.wave_tlas))) return st;
  return upload(pt, &pt->d_wave_lazy, F.wave_lazy);
}

ListedLights listed_lights(const BuiltScene& built, const uint32_t* objects, uint32_t n) {
  ListedLights L;
  for (uint32_t k = 0; k < n; k++) {
    const int32_t li = built.inputs[objects[k]].is_light ? light_of(built, objects[k]) : -1;   // (light_of counts the lights in front)
    if (li < 0) continue;
    L.pairs.push_back(k);
    L.pairs.push_back((uint32_t)li);
    L.max_ntri = std::max(L.max_ntri, built.flat.lights[(size_t)li].ntri);
  }
  return L;
}

// Host forms: the listed lights' records as the host mirror has them now.
int upload_listed_lights(srt_pt* pt, const uint32_t* objects, uint32_t n) {
  const ListedLights L = listed_lights(pt->built, objects, n);
  int st = SRT_OK;
  for (size_t q = 1; q < L.pairs.size() && st == SRT_OK; q += 2) st = upload_light(pt, L.pairs[q], false);
  return st;
}

// Device forms: the records of the `nl` lights in pose.d_light_list from the pose kernel's output where it lies (pose.d_out, `n` poses),
// then their area terms under the new pdfT.  No upload.
void launch_listed_lights(srt_pt* pt, hipStream_t s, uint32_t nl, uint32_t max_ntri, uint32_t n) {
  const FlatScene& F = pt->built.flat;
  launch_light_records(s, pt->pose.d_light_list, nl, pt->pose.d_out, n, pt->d_lights, (uint32_t)F.lights.size());
  launch_light_area_terms(s, pt->pose.d_light_list, nl, max_ntri, pt->d_lights, (uint32_t)F.lights.size(), F.light_tri_first, pt->d_ltris, (uint32_t)F.light_tris.size());
}

void drop_update_tables(srt_pt* pt, uint32_t object) { pt->mesh.drop_refit_tables(object); pt->pose.drop(); pt->top.drop_tables(); }

// The laggards catch up (settle_top of pt_update_pose.cpp, which begins with settle_mesh of pt_update_mesh.cpp - the top half reads
// the boxes its calls left behind the mesh's -, and settle_shading of pt_update_shading.cpp); with nothing pending it does nothing.
int settle(srt_pt* pt) {
  if (!pt) return SRT_OK;
  const int st = settle_top(pt);
  return st != SRT_OK ? st : settle_shading(pt);
}

// srt_pt_scene_begin, srt_pt_scene_commit, srt_pt_destroy: wait for what is pending and forget it.
void discard_pending(srt_pt* pt) {
  if (pt->shade.pending_mats || pt->shade.pending_lights) {
    if (hipSetDevice(pt->device) == hipSuccess) (void)hipEventSynchronize(pt->shade.event);
    pt->shade.pending_mats = pt->shade.pending_lights = false;
  }
  if (!pt->top.pending) return;
  if (hipSetDevice(pt->device) == hipSuccess) (void)hipEventSynchronize(pt->top.event);
  pt->top.refits += pt->top.pending - pt->top.pending_active - pt->mesh.pending;   // (they ran; only their read-back is not worth making any more)
  pt->mesh.refits += pt->mesh.pending;
  pt->mesh.forget_pending();
  pt->top.forget_pending();
}

int not_committed(const char* what) { return srt::fail(SRT_ERR_STATE, "%s before srt_pt_scene_commit", what); }
int need_committed(srt_pt* pt, const char* what) {
  const int settled = settle(pt);
  return settled != SRT_OK ? settled : pt->committed ? SRT_OK : not_committed(what);
}

bool device_builds(const srt_pt* pt) {
  const char* be = getenv("SRT_BVH_BUILDER");
  return pt->device >= 0 && (be ? strcmp(be, "host") != 0 : pt->bvh_builder != 0);
}

DeviceBuilderScope::DeviceBuilderScope(const srt_pt* pt, bool on) {
  if (on) set_device_bvh_builder(build_bvh_device, pt->bvh_device_min);
  else set_device_bvh_builder(nullptr, 0);
}
DeviceBuilderScope::~DeviceBuilderScope() { set_device_bvh_builder(nullptr, 0); }

// (Calls that replace only the BVH<Object> pass the committed BVH<Triangle> depth, which is within the limit.)
int check_depth(uint32_t tlas_depth, uint32_t blas_depth) {
  if ((int)tlas_depth <= kMaxTlasDepth && (int)blas_depth <= kMaxBlasDepth) return SRT_OK;
  return srt::fail(SRT_ERR_UNSUPPORTED, "BVH too deep for the traversal stacks (TLAS %u > %d or BLAS %u > %d)", tlas_depth, kMaxTlasDepth, blas_depth, kMaxBlasDepth);
}

}  // namespace srt

extern "C" {

int srt_pt_scene_counts(srt_pt* pt, uint64_t out[8]) {
  if (!pt || !out) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_counts: NULL argument");
  { const int settled = settle(pt); if (settled != SRT_OK) return settled; }
  const FlatScene& F = pt->built.flat;
  const bool have = pt->committed;
  out[0] = have ? F.objects.size() : 0;
  out[1] = have ? F.tris.size() : 0;
  out[2] = have ? F.nodes.size() - F.tlas_nodes : 0;
  out[3] = have ? F.blas_recs.size() : 0;
  out[4] = pt->blas_builds;
  out[5] = 0;
  if (have && pt->device >= 0)
    out[5] = F.nodes.size() * sizeof(Node) + F.tris.size() * sizeof(Tri) + F.tri_nrm.size() * sizeof(TriNrm) + F.tri_packed.size() * sizeof(float) +
             F.objects.size() * sizeof(Object) + F.lights.size() * sizeof(Light) + F.light_tris.size() * sizeof(LightTri) +
             F.materials.size() * sizeof(Material) + F.wave_tlas.size() * sizeof(WaveInterior) + F.blas_recs.size() * sizeof(WaveInterior) +
             F.wave_lazy.size() * sizeof(uint32_t) + F.delta_lights.size() * sizeof(DeltaLight) + pt->env_map.size() * sizeof(float) +
             pt->mesh.idx_words * sizeof(uint32_t);
  out[6] = pt->bytes_uploaded;
  out[7] = pt->tri_bytes_uploaded;
  return SRT_OK;
}

}  // extern "C"
