// New shading values for a committed scene: srt_pt_update_materials / _lights / _env_light from the caller's values, the shading
// timelines from keys - their device form only enqueues, and settle_shading reads the tables back later - and srt_pt_dump_shading.
// Host code only: the kernel is in pt_anim.hip, the key arithmetic both sides share in pt_anim.h.
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_anim.h"
#include "pt_update.h"
#include "srt_pt_debug.h"

using namespace srt;

// ---- srt_pt_shading_timeline: Anim_Material::at(t) / Scene_Light::set_time(t) of listed materials and delta lights (pt_anim.h, pt_anim.hip) ----
struct srt_pt_shading_timeline : SceneHandle {
  std::vector<uint32_t> materials, lights, track_offsets;   // 6 tracks per material, then 6 per light, then 2 of the environment (env), CSR
  bool env = false;
  std::vector<float> knot_times, knot_values;
  DeviceBuffer<uint32_t> d_track_offsets, d_materials, d_lights;
  DeviceBuffer<float> d_knot_times, d_knot_values;
};

namespace {

const char* material_type_name(uint32_t type) {
  static const char* names[] = {"Lambertian", "Mirror", "Glass", "Diffuse Light", "Refract"};
  return type <= SRT_MAT_REFRACT ? names[type] : "unknown";
}

// What the calls refuse about a list of indices into a table of `size` records, as a message (empty: nothing).
std::string check_index_list(const uint32_t* list, uint32_t n, size_t size, const char* item) {
  std::vector<uint8_t> seen(size, 0);
  for (uint32_t k = 0; k < n; k++) {
    if (list[k] >= size) return std::string(item) + " " + std::to_string(list[k]) + " (entry " + std::to_string(k) + ") is out of range: the scene has " + std::to_string(size);
    if (seen[list[k]]) return std::string(item) + " " + std::to_string(list[k]) + " is listed twice";
    seen[list[k]] = 1;
  }
  return std::string();
}

// The record the kernels read, from a material as srt_pt_add_material takes it: what build_scene makes of it at a commit.
Material material_record(const srt_pt_material& m) {
  Material r;
  r.type = m.type;
  for (int i = 0; i < 3; i++) { r.a[i] = m.a[i]; r.b[i] = m.b[i]; }
  r.ior = m.ior;
  anim_material_store(&r);
  return r;
}

// The verdict is in and nothing of the context is in flight: the listed records into the host's record and, one copy per record, onto the device.
template <typename T>
int write_records(srt_pt* pt, std::vector<T>* host, T* d_table, const uint32_t* list, const std::vector<T>& fresh) {
  for (size_t k = 0; k < fresh.size(); k++) (*host)[list[k]] = fresh[k];
  if (pt->device < 0) return SRT_OK;
  for (size_t k = 0; k < fresh.size(); k++) SRT_HIP(hipMemcpy(d_table + list[k], &fresh[k], sizeof(T), hipMemcpyHostToDevice));
  pt->bytes_uploaded += fresh.size() * sizeof(T);
  return SRT_OK;
}

int update_materials(srt_pt* pt, const char* what, const uint32_t* materials, const srt_pt_material* m, uint32_t n) {
  if (!pt || (n && (!materials || !m))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  FlatScene& F = pt->built.flat;
  const std::string refused = check_index_list(materials, n, F.materials.size(), "material");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<Material> fresh(n);
  for (uint32_t k = 0; k < n; k++) {
    if (m[k].type != F.materials[materials[k]].type)
      return srt::fail(SRT_ERR_INVALID, "%s: material %u was committed as %s (type %u) and cannot become %s (type %u): the type decides the light list, the instancing rules and the elision proof - commit again",
                       what, materials[k], material_type_name(F.materials[materials[k]].type), F.materials[materials[k]].type, material_type_name(m[k].type), m[k].type);
    fresh[k] = material_record(m[k]);
  }
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  return written(pt, write_records(pt, &F.materials, pt->d_mats.get(), materials, fresh));
}

int update_lights(srt_pt* pt, const char* what, const uint32_t* lights, const float* radiance, const float* angle_bounds, const float* trans, uint32_t n) {
  if (!pt || (n && (!lights || !radiance || !trans))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  FlatScene& F = pt->built.flat;
  const std::string refused = check_index_list(lights, n, F.delta_lights.size(), "light");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  std::vector<DeltaLight> fresh(n);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t type = F.delta_lights[lights[k]].type;
    if (type == DL_SPOT && !angle_bounds) return srt::fail(SRT_ERR_INVALID, "%s: light %u is a spot light and needs angle_bounds", what, lights[k]);
    Mat4 T;
    std::memcpy(&T, trans + 16 * (size_t)k, sizeof(Mat4));
    fresh[k] = make_delta_light(type, radiance + 3 * (size_t)k, angle_bounds ? angle_bounds + 2 * (size_t)k : nullptr, T);
  }
  if (pt->device >= 0) SRT_HIP(quiesce(pt));
  return written(pt, write_records(pt, &F.delta_lights, pt->d_dlights.get(), lights, fresh));
}

int update_env_light(srt_pt* pt, const char* what, const float radiance[3]) {
  if (!pt || !radiance) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  if (pt->env_type != SRT_ENV_SPHERE && pt->env_type != SRT_ENV_HEMISPHERE)
    return srt::fail(SRT_ERR_INVALID, "%s: the scene was committed %s; a radiance is what a sphere or hemisphere environment light has", what,
                     pt->env_type == SRT_ENV_MAP ? "with an environment map" : "without an environment light");
  for (int i = 0; i < 3; i++) pt->env_radiance[i] = radiance[i];
  return SRT_OK;
}

int shading_usable(const srt_pt_shading_timeline* tl, const char* what) {
  if (!tl) return srt::fail(SRT_ERR_INVALID, "%s: NULL timeline", what);
  if (tl->stale())
    return srt::fail(SRT_ERR_STATE, "%s: the timeline is stale - its context's scene was begun or committed again after srt_pt_shading_timeline_create", what);
  return SRT_OK;
}

// The host form: every listed item at time t from the host's record of the scene (the committed types; the values a light's triple
// without a key keeps).  lights21: radiance3, angle_bounds2, trans16 per light.
void shading_values(const srt_pt_shading_timeline* tl, float t, srt_pt_material* materials, float* lights21, float env[3]) {
  const FlatScene& F = tl->pt->built.flat;
  const uint32_t nm = (uint32_t)tl->materials.size(), nl = (uint32_t)tl->lights.size();
  const uint32_t* off = tl->track_offsets.data();
  for (uint32_t k = 0; k < nm; k++) {
    Material m;
    m.type = F.materials[tl->materials[k]].type;
    anim_material_item(off, tl->knot_times.data(), tl->knot_values.data(), k, t, &m);
    materials[k].type = m.type;
    for (int i = 0; i < 3; i++) { materials[k].a[i] = m.a[i]; materials[k].b[i] = m.b[i]; }
    materials[k].ior = m.ior;
  }
  for (uint32_t j = 0; j < nl; j++) {
    const DeltaLight& L = F.delta_lights[tl->lights[j]];
    AnimLightOut out;
    anim_light_item(off + 6 * (size_t)nm + 6 * (size_t)j, tl->knot_times.data(), tl->knot_values.data(), t, &out);
    float* o = lights21 + 21 * (size_t)j;
    for (int i = 0; i < 3; i++) o[i] = out.options ? out.radiance[i] : L.radiance[i];
    for (int i = 0; i < 2; i++) o[3 + i] = out.options ? out.angle_bounds[i] : L.angle_bounds[i];
    if (out.pose) std::memcpy(o + 5, out.trans, 16 * sizeof(float));
    else std::memcpy(o + 5, &L.trans, 16 * sizeof(float));
  }
  if (tl->env) anim_env_item(off + 6 * (size_t)nm + 6 * (size_t)nl, tl->knot_times.data(), tl->knot_values.data(), t, env);
}

}  // namespace

namespace srt {

// The host's record catches up with the device after srt_pt_shading_timeline_apply calls: one wait for the event behind the last of them, d_mats and / or d_dlights read back
// once (32 B per material, 160 B per light) into the host's record.
int settle_shading(srt_pt* pt) {
  if (!pt->shade.pending_mats && !pt->shade.pending_lights) return SRT_OK;
  const bool mats = pt->shade.pending_mats, lights = pt->shade.pending_lights;
  pt->shade.pending_mats = pt->shade.pending_lights = false;
  if (!pt->committed) return SRT_OK;                      // (a failure took the scene away: there is no record to bring up to date)
  FlatScene& F = pt->built.flat;
  if (hipSetDevice(pt->device) != hipSuccess || hipEventSynchronize(pt->shade.event) != hipSuccess ||
      (mats && !F.materials.empty() && hipMemcpy(F.materials.data(), pt->d_mats, F.materials.size() * sizeof(Material), hipMemcpyDeviceToHost) != hipSuccess) ||
      (lights && !F.delta_lights.empty() &&
       hipMemcpy(F.delta_lights.data(), pt->d_dlights, F.delta_lights.size() * sizeof(DeltaLight), hipMemcpyDeviceToHost) != hipSuccess)) {
    pt->committed = false;
    return srt::fail(SRT_ERR_HIP, "settling srt_pt_shading_timeline_apply: %s; the scene has to be committed again", hipGetErrorString(hipGetLastError()));
  }
  return SRT_OK;
}

}  // namespace srt

extern "C" {

int srt_pt_update_materials(srt_pt* pt, const uint32_t* materials, const srt_pt_material* m, uint32_t n) {
  return update_materials(pt, "srt_pt_update_materials", materials, m, n);
}

int srt_pt_update_lights(srt_pt* pt, const uint32_t* lights, const float* radiance, const float* angle_bounds, const float* trans, uint32_t n) {
  return update_lights(pt, "srt_pt_update_lights", lights, radiance, angle_bounds, trans, n);
}

int srt_pt_update_env_light(srt_pt* pt, const float radiance[3]) { return update_env_light(pt, "srt_pt_update_env_light", radiance); }

int srt_pt_shading_timeline_create(srt_pt* pt, const uint32_t* materials, uint32_t nmaterials, const uint32_t* lights, uint32_t nlights, int env,
                                   const uint32_t* track_offsets, const float* knot_times, const float* knot_values, srt_pt_shading_timeline** out) {
  const char* what = "srt_pt_shading_timeline_create";
  if (out) *out = nullptr;
  if (!pt || (nmaterials && !materials) || (nlights && !lights) || !track_offsets || !knot_times || !knot_values || !out)
    return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  int st;
  if ((st = need_committed(pt, what))) return st;
  const FlatScene& F = pt->built.flat;
  if (!nmaterials && !nlights && !env) return srt::fail(SRT_ERR_INVALID, "%s: nothing is listed", what);
  if ((uint64_t)nmaterials + nlights > (1u << 28)) return srt::fail(SRT_ERR_INVALID, "%s: %u materials and %u lights", what, nmaterials, nlights);
  std::string refused = check_index_list(materials, nmaterials, F.materials.size(), "material");
  if (refused.empty()) refused = check_index_list(lights, nlights, F.delta_lights.size(), "light");
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  if (env && pt->env_type != SRT_ENV_SPHERE && pt->env_type != SRT_ENV_HEMISPHERE)
    return srt::fail(SRT_ERR_INVALID, "%s: environment keys need a sphere or hemisphere environment light (the scene has %s)", what,
                     pt->env_type == SRT_ENV_MAP ? "an environment map" : "none");
  const uint32_t ntracks = 6u * nmaterials + 6u * nlights + (env ? 2u : 0u);
  refused = anim_check_tracks(track_offsets, ntracks, 1, knot_times, false, "track");
  const uint32_t* lo = track_offsets + 6 * (size_t)nmaterials;
  const char* const no_key = "has no key on any track (Splines::any() is false: the reference would not change it)";
  for (uint32_t k = 0; k < nmaterials && refused.empty(); k++)
    if (track_offsets[6 * (size_t)k] == track_offsets[6 * (size_t)k + 6]) refused = "material " + std::to_string(k) + " of the list " + no_key;
  for (uint32_t j = 0; j < nlights && refused.empty(); j++)
    if (lo[6 * (size_t)j] == lo[6 * (size_t)j + 6]) refused = "light " + std::to_string(j) + " of the list " + no_key;
  if (env && refused.empty() && lo[6 * (size_t)nlights] == lo[6 * (size_t)nlights + 2]) refused = std::string("the environment light ") + no_key;
  if (!refused.empty()) return srt::fail(SRT_ERR_INVALID, "%s: %s", what, refused.c_str());
  srt_pt_shading_timeline* tl = new (std::nothrow) srt_pt_shading_timeline;
  if (!tl) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  const size_t nk = track_offsets[ntracks];
  tl->pt = pt; tl->generation = pt->scene_generation; tl->env = env != 0;
  if (nmaterials) tl->materials.assign(materials, materials + nmaterials);
  if (nlights) tl->lights.assign(lights, lights + nlights);
  tl->track_offsets.assign(track_offsets, track_offsets + ntracks + 1);
  tl->knot_times.assign(knot_times, knot_times + nk);
  tl->knot_values.assign(knot_values, knot_values + 4 * nk);
  return handle_publish(tl, out, [&]() -> int {
    SRT_HIP(hipSetDevice(pt->device));
    int w;
    if ((w = tl->d_track_offsets.upload(tl->track_offsets)) || (w = tl->d_materials.upload(tl->materials)) || (w = tl->d_lights.upload(tl->lights)) ||
        (w = tl->d_knot_times.upload(tl->knot_times)) || (w = tl->d_knot_values.upload(tl->knot_values)))
      return w;
    pt->bytes_uploaded += (tl->track_offsets.size() + tl->materials.size() + tl->lights.size()) * sizeof(uint32_t) + 5 * nk * sizeof(float);
    return SRT_OK;
  });
}

int srt_pt_shading_timeline_destroy(srt_pt_shading_timeline* timeline) { return handle_destroy(timeline); }

int srt_pt_shading_timeline_values(srt_pt_shading_timeline* timeline, float t, srt_pt_material* materials_out, float* lights_out, float env_out[3]) {
  const char* what = "srt_pt_shading_timeline_values";
  int st = shading_usable(timeline, what);
  if (st != SRT_OK) return st;
  if ((!timeline->materials.empty() && !materials_out) || (!timeline->lights.empty() && !lights_out) || (timeline->env && !env_out))
    return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  if ((st = settle(timeline->pt)) != SRT_OK) return st;   // (a light's triple without a key keeps the record's values)
  shading_values(timeline, t, materials_out, lights_out, env_out);
  return SRT_OK;
}

int srt_pt_shading_timeline_update(srt_pt_shading_timeline* timeline, float t) {
  const char* what = "srt_pt_shading_timeline_update";
  int st = shading_usable(timeline, what);
  if (st != SRT_OK) return st;
  srt_pt* pt = timeline->pt;
  if ((st = settle(pt)) != SRT_OK) return st;
  const uint32_t nm = (uint32_t)timeline->materials.size(), nl = (uint32_t)timeline->lights.size();
  std::vector<srt_pt_material> mats(nm);
  std::vector<float> lights(21 * (size_t)nl), radiance(3 * (size_t)nl), bounds(2 * (size_t)nl), trans(16 * (size_t)nl);
  float env[3] = {0.0f, 0.0f, 0.0f};
  shading_values(timeline, t, mats.data(), lights.data(), env);
  for (uint32_t j = 0; j < nl; j++) {
    std::memcpy(&radiance[3 * (size_t)j], &lights[21 * (size_t)j], 3 * sizeof(float));
    std::memcpy(&bounds[2 * (size_t)j], &lights[21 * (size_t)j + 3], 2 * sizeof(float));
    std::memcpy(&trans[16 * (size_t)j], &lights[21 * (size_t)j + 5], 16 * sizeof(float));
  }
  if (nm && (st = update_materials(pt, what, timeline->materials.data(), mats.data(), nm))) return st;
  if (nl && (st = update_lights(pt, what, timeline->lights.data(), radiance.data(), bounds.data(), trans.data(), nl))) return st;
  if (timeline->env && (st = update_env_light(pt, what, env))) return st;
  return SRT_OK;
}

int srt_pt_shading_timeline_apply(srt_pt_shading_timeline* timeline, void* stream, float t) {
  const char* what = "srt_pt_shading_timeline_apply";
  const int usable = shading_usable(timeline, what);       // (no settle(): this call only adds to what is pending)
  if (usable != SRT_OK) return usable;
  srt_pt* pt = timeline->pt;
  if (pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: the kernel runs on the device only; this context is host-only (srt_pt_shading_timeline_update is the host form)", what);
  SRT_HIP(hipSetDevice(pt->device));
  const uint32_t nm = (uint32_t)timeline->materials.size(), nl = (uint32_t)timeline->lights.size();
  if (nm + nl) {
    { const int made = pt->shade.event.create(hipEventDisableTiming); if (made != SRT_OK) return made; }
    launch_anim_shading(stream, timeline->d_track_offsets, timeline->d_knot_times, timeline->d_knot_values, timeline->d_materials, nm, timeline->d_lights, nl, t,
                        pt->d_mats, pt->d_dlights);
    // the host's record is behind from here until settle(); a HIP failure leaves a record nobody can vouch for: commit again
    pt->shade.pending_mats = pt->shade.pending_mats || nm != 0;
    pt->shade.pending_lights = pt->shade.pending_lights || nl != 0;
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipEventRecord(pt->shade.event, (hipStream_t)stream);
    if (he != hipSuccess) {
      pt->committed = false;
      pt->shade.pending_mats = pt->shade.pending_lights = false;
      return srt::fail(SRT_ERR_HIP, "%s: the launch failed (%s); the scene has to be committed again", what, hipGetErrorString(he));
    }
  }
  // the environment's radiance is a launch parameter: one item, evaluated here by the function of pt_anim.h, in effect from the next launch
  if (timeline->env)
    anim_env_item(timeline->track_offsets.data() + 6 * (size_t)nm + 6 * (size_t)nl, timeline->knot_times.data(), timeline->knot_values.data(), t, pt->env_radiance);
  return SRT_OK;
}

int srt_pt_dump_shading(srt_pt* pt, int from_device, uint32_t counts[2], srt_pt_material* materials, size_t cap_materials, uint32_t* light_heads,
                        float* light_values, size_t cap_lights, uint32_t* env_type, float env_radiance[3]) {
  const char* what = "srt_pt_dump_shading";
  if (!pt || !counts || (cap_materials && !materials) || (cap_lights && (!light_heads || !light_values))) return srt::fail(SRT_ERR_INVALID, "%s: NULL argument", what);
  { const int ready = need_committed(pt, what); if (ready != SRT_OK) return ready; }
  if (from_device && pt->device < 0)
    return srt::fail(SRT_ERR_UNSUPPORTED, "%s: this context is host-only, there are no device arrays to read (from_device = 0 reads the host's)", what);
  const FlatScene& F = pt->built.flat;
  std::vector<Material> mats(F.materials);
  std::vector<DeltaLight> lights(F.delta_lights);
  if (from_device) {
    SRT_HIP(hipSetDevice(pt->device));
    SRT_HIP(hipDeviceSynchronize());
    if (!mats.empty()) SRT_HIP(hipMemcpy(mats.data(), pt->d_mats, mats.size() * sizeof(Material), hipMemcpyDeviceToHost));
    if (!lights.empty()) SRT_HIP(hipMemcpy(lights.data(), pt->d_dlights, lights.size() * sizeof(DeltaLight), hipMemcpyDeviceToHost));
  }
  counts[0] = (uint32_t)mats.size(); counts[1] = (uint32_t)lights.size();
  for (size_t k = 0; k < mats.size() && k < cap_materials; k++) {
    materials[k].type = mats[k].type;
    for (int i = 0; i < 3; i++) { materials[k].a[i] = mats[k].a[i]; materials[k].b[i] = mats[k].b[i]; }
    materials[k].ior = mats[k].ior;
  }
  for (size_t j = 0; j < lights.size() && j < cap_lights; j++) {
    const DeltaLight& L = lights[j];
    light_heads[2 * j] = L.type; light_heads[2 * j + 1] = L.has_trans;
    float* o = light_values + 37 * j;
    for (int i = 0; i < 3; i++) o[i] = L.radiance[i];
    o[3] = L.angle_bounds[0]; o[4] = L.angle_bounds[1];
    std::memcpy(o + 5, &L.trans, 16 * sizeof(float));
    std::memcpy(o + 21, &L.itrans, 16 * sizeof(float));
  }
  if (env_type) *env_type = pt->env_type;
  if (env_radiance)
    for (int i = 0; i < 3; i++) env_radiance[i] = pt->env_radiance[i];
  return SRT_OK;
}

}  // extern "C"
