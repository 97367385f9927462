// The path tracer's lifecycle and scene description: create / destroy, scene begin / add / commit, and the settings a render reads
// (camera, image size, tiling, kernel mode, switches).  Host code only - no kernel is defined or launched here; the context is
// pt_context.h's.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_context.h"
#include "pt_env_image.h"
#include "pt_trace.h"
#include "srt_pt_debug.h"

using namespace srt;

namespace {

void update_tiling(srt_pt* pt) {
  TileMap& T = pt->tiles;
  if (!pt->w || !pt->h) { T.tiles_x = T.tiles_y = T.local_tiles = 0; pt->tiles_per_rank = 0; return; }
  T.tiles_x = (pt->w + T.tile_w - 1) / T.tile_w;
  T.tiles_y = (pt->h + T.tile_h - 1) / T.tile_h;
  const uint32_t ntiles = T.tiles_x * T.tiles_y;
  pt->tiles_per_rank = (ntiles + T.world - 1) / T.world;
  T.local_tiles = (ntiles > T.rank) ? (ntiles - T.rank + T.world - 1) / T.world : 0;
}

// The image sampler's tables describe a map that goes (launches that read the device copies may still be in flight on any stream).
void drop_env_image(srt_pt* pt) {
  if (pt->env_image.d_tables || pt->env_image.d_trig) {
    (void)hipSetDevice(pt->device);
    (void)hipDeviceSynchronize();
  }
  pt->env_image.drop();
}

}  // namespace

namespace srt {
int need_device(srt_pt* pt, const char* what) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "%s: NULL context", what);
  if (pt->device < 0) return srt::fail(SRT_ERR_NO_DEVICE, "%s needs a HIP device; this context is host-only and there is no CPU fallback", what);
  SRT_HIP(hipSetDevice(pt->device));
  return SRT_OK;
}

int need_ready(srt_pt* pt, const char* what) {
  int st = need_device(pt, what);
  if (st != SRT_OK) return st;
  if (!pt->committed) return not_committed(what);
  if (!pt->have_cam) return srt::fail(SRT_ERR_STATE, "%s before srt_pt_set_camera", what);
  if (!pt->w || !pt->h) return srt::fail(SRT_ERR_STATE, "%s before srt_pt_set_params", what);
  return SRT_OK;
}

int env_image_host_tables(srt_pt* pt, const char* what) {
  if (pt->env_type != SRT_ENV_MAP)
    return srt::fail(SRT_ERR_INVALID, "%s: image sampling (srt_pt_set_env_sampling) needs an environment map (srt_pt_set_env_map); the scene has %s",
                     what, pt->env_type == SRT_ENV_NONE ? "no environment light" : pt->env_type == SRT_ENV_SPHERE ? "a uniform sphere" : "a uniform hemisphere");
  if (pt->env_image.cdf_pdf.empty()) {
    EnvImageTables T;
    build_env_image_tables(pt->env_map.data(), pt->env_w, pt->env_h, &T);
    pt->env_image.cdf_pdf = std::move(T.cdf_pdf); pt->env_image.trig = std::move(T.trig); pt->env_image.total = T.total;
  }
  return SRT_OK;
}

int env_image_ready(srt_pt* pt, const char* what) {
  if (pt->env_sampling != SRT_ENV_SAMPLING_IMAGE || pt->normal_colors) return SRT_OK;
  return env_image_upload(pt, what);
}

int env_image_upload(srt_pt* pt, const char* what) {
  int st = env_image_host_tables(pt, what);
  if (st != SRT_OK || pt->env_image.valid) return st;
  if ((st = upload(pt, &pt->env_image.d_tables, pt->env_image.cdf_pdf)) || (st = upload(pt, &pt->env_image.d_trig, pt->env_image.trig))) return st;
  pt->env_image.valid = true;
  return SRT_OK;
}
}  // namespace srt

extern "C" {

int srt_pt_create(int device, srt_pt** out) {
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_create: out is NULL");
  *out = nullptr;
  srt_pt* pt = new (std::nothrow) srt_pt();
  if (!pt) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  if (device >= 0) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
      delete pt;
      return srt::fail(SRT_ERR_NO_DEVICE, "no HIP device available (%s); this path has no CPU fallback",
                       e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    }
    if (device >= count) { delete pt; return srt::fail(SRT_ERR_INVALID, "device %d out of range [0,%d)", device, count); }
    if (hipSetDevice(device) != hipSuccess || pt->stream.create(hipStreamNonBlocking) != SRT_OK ||
        pt->d_totals.ensure(C_COUNT + 4) != SRT_OK || pt->h_fault.ensure(1, hipHostMallocMapped) != SRT_OK ||
        pt->h_cancel.ensure(1, hipHostMallocMapped) != SRT_OK ||
        hipMemset(pt->d_totals, 0, (C_COUNT + 4) * sizeof(unsigned long long)) != hipSuccess) {
      delete pt;
      return srt::fail(SRT_ERR_HIP, "HIP context setup failed on device %d", device);
    }
    *pt->h_fault = 0u;
    *pt->h_cancel = 0u;
    (void)hipDeviceSynchronize();                         // (the null-stream memset above: done before any non-blocking stream's first kernel)
    pt->device = device;
  }
  *out = pt;
  return SRT_OK;
}

int srt_pt_destroy(srt_pt* pt) {
  if (!pt) return SRT_OK;
  if (pt->device >= 0) {
    (void)hipSetDevice(pt->device);
    discard_pending(pt);
    (void)hipStreamSynchronize(pt->stream);
    report_cast_stats(pt);
    pt->stream.reset();                                   // (the stream goes first, what its kernels used after it)
  }
  delete pt;
  return SRT_OK;
}

int srt_pt_scene_begin(srt_pt* pt) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_begin: NULL context");
  discard_pending(pt);
  pt->inputs.clear();
  pt->materials.clear();
  pt->delta_lights.clear();
  pt->env_type = 0;
  pt->env_map.clear(); pt->env_w = pt->env_h = 0;
  drop_env_image(pt);
  pt->committed = false;
  pt->scene_generation++;
  return SRT_OK;
}

int srt_pt_add_material(srt_pt* pt, const srt_pt_material* m, uint32_t* index_out) {
  if (!pt || !m) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_material: NULL argument");
  if (m->type > SRT_MAT_REFRACT) return srt::fail(SRT_ERR_INVALID, "unknown material type %u", m->type);
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  Material mm;
  mm.type = m->type;
  for (int i = 0; i < 3; i++) { mm.a[i] = m->a[i]; mm.b[i] = m->b[i]; }
  mm.ior = m->ior;
  pt->materials.push_back(mm);
  if (index_out) *index_out = (uint32_t)pt->materials.size() - 1;
  return SRT_OK;
}

int srt_pt_add_mesh(srt_pt* pt, const float* positions, const float* normals, uint32_t nverts, const uint32_t* indices,
                    uint32_t nindices, const float trans[16], uint32_t material, int is_area_light) {
  if (!pt || !positions || !normals || !indices || !trans) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_mesh: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (nverts == 0 || nindices == 0 || nindices % 3) return srt::fail(SRT_ERR_INVALID, "mesh needs >= 1 triangle (nindices %u)", nindices);
  if (material >= pt->materials.size()) return srt::fail(SRT_ERR_INVALID, "material %u not defined", material);
  for (uint32_t i = 0; i < nindices; i++)
    if (indices[i] >= nverts) return srt::fail(SRT_ERR_INVALID, "index %u (= %u) out of range (nverts %u)", i, indices[i], nverts);
  ObjectInput o;
  o.kind = OBJ_MESH;
  std::memcpy(&o.trans, trans, sizeof(Mat4));
  o.material = material;
  o.is_light = is_area_light != 0;
  o.mesh.pos.assign(positions, positions + 3 * (size_t)nverts);
  o.mesh.nrm.assign(normals, normals + 3 * (size_t)nverts);
  o.mesh.idx.assign(indices, indices + nindices);
  pt->inputs.push_back(std::move(o));
  return SRT_OK;
}

int srt_pt_add_instance(srt_pt* pt, uint32_t source_object, const float trans[16], uint32_t material) {
  if (!pt || !trans) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_instance: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (source_object >= pt->inputs.size()) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_instance: object %u is not added yet (%zu objects so far)", source_object, pt->inputs.size());
  const ObjectInput& src = pt->inputs[source_object];
  if (src.kind != OBJ_MESH || src.source >= 0)
    return srt::fail(SRT_ERR_INVALID, "srt_pt_add_instance: object %u is %s, not a mesh added by srt_pt_add_mesh", source_object,
                     src.kind != OBJ_MESH ? "a sphere" : "an instance");
  if (material >= pt->materials.size()) return srt::fail(SRT_ERR_INVALID, "material %u not defined", material);
  if (pt->materials[material].type == SRT_MAT_DIFFUSE_LIGHT)
    return srt::fail(SRT_ERR_INVALID, "srt_pt_add_instance: an emissive object needs triangles of its own in the area-light list; add it with srt_pt_add_mesh");
  ObjectInput o;
  o.kind = OBJ_MESH;
  std::memcpy(&o.trans, trans, sizeof(Mat4));
  o.material = material;
  o.source = (int32_t)source_object;
  pt->inputs.push_back(std::move(o));
  return SRT_OK;
}

int srt_pt_add_sphere(srt_pt* pt, float radius, const float trans[16], uint32_t material) {
  if (!pt || !trans) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_sphere: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (material >= pt->materials.size()) return srt::fail(SRT_ERR_INVALID, "material %u not defined", material);
  ObjectInput o;
  o.kind = OBJ_SPHERE;
  std::memcpy(&o.trans, trans, sizeof(Mat4));
  o.material = material;
  o.radius = radius;
  pt->inputs.push_back(std::move(o));
  return SRT_OK;
}

int srt_pt_add_sphere_light(srt_pt* pt, float radius, const float trans[16], uint32_t material, const float* positions,
                            const float* normals, uint32_t nverts, const uint32_t* indices, uint32_t nindices) {
  if (!pt || !trans || !positions || !normals || !indices) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_sphere_light: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (material >= pt->materials.size()) return srt::fail(SRT_ERR_INVALID, "material %u not defined", material);
  if (!nverts || !nindices || nindices % 3) return srt::fail(SRT_ERR_INVALID, "the light mesh needs triangles (%u vertices, %u indices)", nverts, nindices);
  ObjectInput o;
  o.kind = OBJ_SPHERE;
  std::memcpy(&o.trans, trans, sizeof(Mat4));
  o.material = material;
  o.radius = radius;
  o.is_light = true;
  o.mesh.pos.assign(positions, positions + 3 * (size_t)nverts);
  o.mesh.nrm.assign(normals, normals + 3 * (size_t)nverts);
  o.mesh.idx.assign(indices, indices + nindices);
  pt->inputs.push_back(std::move(o));
  return SRT_OK;
}

int srt_pt_add_light(srt_pt* pt, uint32_t type, const float radiance[3], const float angle_bounds[2], const float trans[16]) {
  if (!pt || !radiance || !trans) return srt::fail(SRT_ERR_INVALID, "srt_pt_add_light: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (type > SRT_LIGHT_SPOT) return srt::fail(SRT_ERR_INVALID, "unknown light type %u", type);
  if (type == SRT_LIGHT_SPOT && !angle_bounds) return srt::fail(SRT_ERR_INVALID, "a spot light needs angle_bounds");
  Mat4 T;
  std::memcpy(&T, trans, sizeof(Mat4));
  pt->delta_lights.push_back(make_delta_light(type, radiance, angle_bounds, T));
  return SRT_OK;
}

int srt_pt_set_env_light(srt_pt* pt, uint32_t type, const float radiance[3]) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_env_light: NULL context");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (type > SRT_ENV_HEMISPHERE) return srt::fail(SRT_ERR_INVALID, "unknown environment light type %u (image maps: srt_pt_set_env_map)", type);
  if (type != SRT_ENV_NONE && !radiance) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_env_light: radiance is NULL");
  pt->env_type = type;
  for (int i = 0; i < 3; i++) pt->env_radiance[i] = (type != SRT_ENV_NONE) ? radiance[i] : 0.0f;
  return SRT_OK;
}

int srt_pt_set_env_map(srt_pt* pt, uint32_t width, uint32_t height, const float* rgb) {
  if (!pt || !rgb) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_env_map: NULL argument");
  if (pt->committed) return srt::fail(SRT_ERR_STATE, "scene already committed; call srt_pt_scene_begin first");
  if (!width || !height || (uint64_t)width * height > (1ull << 28)) return srt::fail(SRT_ERR_INVALID, "environment map size %ux%u", width, height);
  pt->env_type = SRT_ENV_MAP;
  pt->env_w = width; pt->env_h = height;
  pt->env_map.assign(rgb, rgb + 3 * (size_t)width * height);
  drop_env_image(pt);                                     // the sampler's tables describe the map that goes
  return SRT_OK;
}

int srt_pt_scene_commit(srt_pt* pt, int use_bvh) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_scene_commit: NULL context");
  discard_pending(pt);
  if (pt->device >= 0) { SRT_HIP(hipSetDevice(pt->device)); drop_update_tables(pt, UINT32_MAX); }   // they describe trees and records that are about to go
  pt->committed = false;    // build_scene replaces the host's record, the uploads below the device's: no scene until the last has gone through
  // BVH<Triangle> builds of big meshes run on the device (pt_bvh_device.hip: identical arrays); srt_pt_set_bvh_builder
  const DeviceBuilderScope builder(pt, device_builds(pt));
  const std::string err = build_scene(pt->inputs, pt->materials, use_bvh != 0, &pt->built);
  pt->blas_builds += pt->built.blas_builds;
  if (!err.empty()) return srt::fail(SRT_ERR_UNSUPPORTED, "%s", err.c_str());
  pt->built.flat.delta_lights = pt->delta_lights;
  const FlatScene& F = pt->built.flat;
  int st;
  if ((st = check_depth(F.max_tlas_depth, F.max_blas_depth))) return st;
  if (pt->device >= 0) {
    SRT_HIP(hipSetDevice(pt->device));
    SRT_HIP(hipStreamSynchronize(pt->stream));
    if ((st = upload(pt, &pt->d_nodes, F.nodes)) || (st = upload(pt, &pt->d_tris, F.tris, true)) || (st = upload(pt, &pt->d_nrm, F.tri_nrm, true)) ||
        (st = upload(pt, &pt->d_tri_packed, F.tri_packed, true)) ||
        (st = upload(pt, &pt->d_objects, F.objects)) || (st = upload(pt, &pt->d_lights, F.lights)) ||
        (st = upload(pt, &pt->d_ltris, F.light_tris)) || (st = upload(pt, &pt->d_mats, F.materials)) ||
        (st = upload(pt, &pt->d_wave, F.wave_tlas)) || (st = upload(pt, &pt->d_blas, F.blas_recs, true)) || (st = upload(pt, &pt->d_wave_lazy, F.wave_lazy)) ||
        (st = upload(pt, &pt->d_dlights, F.delta_lights)) || (st = upload(pt, &pt->d_env_map, pt->env_map)))
      return st;
    // the index buffers the kernels of pt_mesh_update.hip read (12 B per triangle)
    std::vector<uint32_t> idx;
    pt->mesh.idx_off.assign(pt->built.inputs.size(), SIZE_MAX);
    for (size_t i = 0; i < pt->built.inputs.size(); i++) {
      const ObjectInput& in = pt->built.inputs[i];
      if (in.kind != OBJ_MESH || in.source >= 0 || (in.is_light && !pt->built.dynamic_lights)) continue;   // (a light's goes up later when the switch is set later: ensure_mesh_idx)
      pt->mesh.idx_off[i] = idx.size();
      idx.insert(idx.end(), in.mesh.idx.begin(), in.mesh.idx.end());
    }
    pt->mesh.idx_words = idx.size();
    pt->mesh.idx_uncounted = 0;
    if ((st = upload(pt, &pt->mesh.d_idx, idx))) return st;
  }
  pt->committed = true;
  pt->scene_generation++;
  pt->drop_cast_shapes();
  return SRT_OK;
}

int srt_pt_set_stream_slots(srt_pt* pt, uint32_t slots) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_stream_slots: NULL context");
  if (slots > kMaxStreamSlots) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_stream_slots: at most %u path slots (got %u)", kMaxStreamSlots, slots);
  pt->stream_slots = slots;
  return SRT_OK;
}

int srt_pt_set_bvh_builder(srt_pt* pt, int device, uint32_t min_primitives) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_bvh_builder: NULL context");
  pt->bvh_builder = device ? 1 : 0;
  pt->bvh_device_min = min_primitives;
  return SRT_OK;
}

int srt_pt_set_camera(srt_pt* pt, const float iview[16], float vert_fov_deg, float aspect_ratio) {
  if (!pt || !iview) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_camera: NULL argument");
  pt->cam = make_camera(iview, vert_fov_deg, aspect_ratio);
  pt->have_cam = true;
  return SRT_OK;
}

int srt_pt_set_params(srt_pt* pt, uint32_t width, uint32_t height, uint32_t max_depth) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_params: NULL context");
  if (!width || !height) return srt::fail(SRT_ERR_INVALID, "image must be at least 1x1 (got %ux%u)", width, height);
  if ((uint64_t)width * height > 0x7fffffffull) return srt::fail(SRT_ERR_UNSUPPORTED, "image larger than 2^31 pixels");
  if (width > 65535u || height > 65535u) return srt::fail(SRT_ERR_UNSUPPORTED, "image sides above 65535 are not supported (got %ux%u)", width, height);
  if (max_depth > (uint32_t)kMaxPathDepth) return srt::fail(SRT_ERR_UNSUPPORTED, "max_depth %u > %d is not supported", max_depth, kMaxPathDepth);
  pt->w = width; pt->h = height; pt->max_depth = max_depth;
  update_tiling(pt);
  return SRT_OK;
}

int srt_pt_set_tiling(srt_pt* pt, uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t world) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_tiling: NULL context");
  if (!tile_w || !tile_h || tile_w % 8 || tile_h % 8) return srt::fail(SRT_ERR_INVALID, "tile size must be a positive multiple of 8 (got %ux%u)", tile_w, tile_h);
  if (!world || rank >= world) return srt::fail(SRT_ERR_INVALID, "rank %u / world %u is not a valid shard", rank, world);
  pt->tiles.tile_w = tile_w; pt->tiles.tile_h = tile_h; pt->tiles.rank = rank; pt->tiles.world = world;
  update_tiling(pt);
  return SRT_OK;
}

int srt_pt_tile_info(srt_pt* pt, uint32_t* local_tiles, uint32_t* tiles_per_rank, uint32_t* floats_per_tile) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_tile_info: NULL context");
  if (!pt->w) return srt::fail(SRT_ERR_STATE, "srt_pt_tile_info before srt_pt_set_params");
  if (local_tiles) *local_tiles = pt->tiles.local_tiles;
  if (tiles_per_rank) *tiles_per_rank = pt->tiles_per_rank;
  if (floats_per_tile) *floats_per_tile = pt->tiles.tile_w * pt->tiles.tile_h * 3;
  return SRT_OK;
}

int srt_pt_set_kernel(srt_pt* pt, int mode) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_kernel: NULL context");
  if (mode < 0 || mode > 7)
    return srt::fail(SRT_ERR_INVALID, "kernel mode must be 0 (auto), 1 (per-lane, lane per pixel), 2 (wave-uniform), 3 (wave-uniform, stamped), 4 (per-lane, lane per sample), 5 (persistent waves, flattened per-lane walk), 6 (streamed: logic + ray-cast kernels) or 7 (streamed sweeps: BVH<Triangle> walks queued)");
  pt->kernel_mode = mode;
  return SRT_OK;
}

int srt_pt_set_elision(srt_pt* pt, int on) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_elision: NULL context");
  pt->elide = on ? 1 : 0;
  pt->wave_blocks = 0;                                    // the launch configuration is re-derived for the other build
  return SRT_OK;
}

int srt_pt_set_dynamic_lights(srt_pt* pt, int on) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_dynamic_lights: NULL context");
  pt->built.dynamic_lights = on != 0;
  return SRT_OK;
}

int srt_pt_set_env_sampling(srt_pt* pt, uint32_t mode) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_env_sampling: NULL context");
  if (mode > SRT_ENV_SAMPLING_IMAGE)
    return srt::fail(SRT_ERR_INVALID, "srt_pt_set_env_sampling: unknown mode %u (0 uniform, 1 image)", mode);
  pt->env_sampling = mode;                                // the tables follow at the first launch that needs them (env_image_ready)
  return SRT_OK;
}

int srt_pt_env_sampling(srt_pt* pt, uint32_t* mode) {
  if (!pt || !mode) return srt::fail(SRT_ERR_INVALID, "srt_pt_env_sampling: NULL argument");
  *mode = pt->env_sampling;
  return SRT_OK;
}

int srt_pt_set_normal_colors(srt_pt* pt, int on) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_normal_colors: NULL context");
  pt->normal_colors = on ? 1 : 0;
  return SRT_OK;
}

// ---- Pathtracer::log_ray: the switch (the rings and their readers: pt.hip) ---------------------------------------------
int srt_pt_set_ray_log(srt_pt* pt, uint32_t capacity) {
  if (!pt) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_ray_log: NULL context");
  if (capacity > (1u << 26)) return srt::fail(SRT_ERR_INVALID, "srt_pt_set_ray_log: at most 2^26 rays per read (got %u)", capacity);
  pt->ray_log_cap = capacity;                             // the rings follow at the next epoch on each stream (stream_buffers)
  return SRT_OK;
}

int srt_pt_live_resources(uint64_t out[4]) {
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_live_resources: NULL argument");
  for (int k = 0; k < OWNED_KINDS; k++) out[k] = owned_live((OwnedKind)k).load(std::memory_order_relaxed);
  return SRT_OK;
}

}  // extern "C"
