// anim_shading_ref.cpp - the reference's own material and light keys (Material::Anim_Material::at, Spectrum::to_linear,
// Material::emissive, Scene_Light::set_time, Scene_Light::radiance, Pose::transform) run on keys the caller describes, for
// tests/golden/make_shading_golden.py to record (tests/golden/anim_shading.npz: data only).
//
// INTEGRATION HARNESS, part of integration/_build/libdropin_pt_full.so, where scene/material.cpp, scene/light.cpp and scene/pose.cpp
// are compiled where they lie.  Nothing of the product runs here.  The library is built with -fno-access-control, so the knots go
// straight into the splines' maps, as in anim_ref.cpp.
#include <cstdint>

#include "scene/light.h"
#include "scene/material.h"
#include "scene/pose.h"

namespace {

Spectrum spectrum_at(const float* values, uint32_t k) { return Spectrum(values[4 * k], values[4 * k + 1], values[4 * k + 2]); }

}  // namespace

extern "C" {

// One Material with the reference's default options.  offsets[7]: the knots of the albedo, reflectance, transmittance, emissive,
// intensity and ior tracks are [offsets[i], offsets[i + 1]) of times / values (4 floats per knot: xyz_ or x___).  Out, per
// requested time, 20 floats: the six options after Scene_Object::set_time's material step (albedo3, reflectance3, transmittance3,
// emissive3, intensity, ior), then albedo.to_linear() and Material::emissive().
__attribute__((visibility("default")))
void dropin_anim_material_reference(const uint32_t* offsets, const float* times, const float* values, const float* ts, uint32_t nt, float* out20) {
  Material mat;
  auto& s = mat.anim.splines;
  for (uint32_t k = offsets[0]; k < offsets[1]; k++) s.head.control_points[times[k]] = spectrum_at(values, k);
  for (uint32_t k = offsets[1]; k < offsets[2]; k++) s.tail.head.control_points[times[k]] = spectrum_at(values, k);
  for (uint32_t k = offsets[2]; k < offsets[3]; k++) s.tail.tail.head.control_points[times[k]] = spectrum_at(values, k);
  for (uint32_t k = offsets[3]; k < offsets[4]; k++) s.tail.tail.tail.head.control_points[times[k]] = spectrum_at(values, k);
  for (uint32_t k = offsets[4]; k < offsets[5]; k++) s.tail.tail.tail.tail.head.control_points[times[k]] = values[4 * k];
  for (uint32_t k = offsets[5]; k < offsets[6]; k++) s.tail.tail.tail.tail.tail.head.control_points[times[k]] = values[4 * k];
  for (uint32_t i = 0; i < nt; i++) {
    if (mat.anim.splines.any()) mat.anim.at(ts[i], mat.opt);   // (scene/object.cpp:71)
    const Material::Options& o = mat.opt;
    const Spectrum lin = o.albedo.to_linear(), em = mat.emissive();
    const float row[20] = {o.albedo.r, o.albedo.g, o.albedo.b, o.reflectance.r, o.reflectance.g, o.reflectance.b, o.transmittance.r, o.transmittance.g,
                           o.transmittance.b, o.emissive.r, o.emissive.g, o.emissive.b, o.intensity, o.ior, lin.r, lin.g, lin.b, em.r, em.g, em.b};
    for (int a = 0; a < 20; a++) out20[20 * i + a] = row[a];
  }
}

// One Scene_Light of the given Light_Type with the options (spectrum3, intensity, angle_bounds2) and pose (pos3, euler3, scale3) it
// starts from.  offsets[7]: the spectrum, intensity and angle_bounds tracks of Anim_Light, then the position, rotation (xyzw) and
// scale tracks of Anim_Pose.  Out, per requested time, 25 floats after Scene_Light::set_time(t): spectrum3, intensity, angle_bounds2,
// Scene_Light::radiance(), pose.transform() in Mat4::data order.
__attribute__((visibility("default")))
void dropin_anim_light_reference(int light_type, const float* options6, const float* pose9, const uint32_t* offsets, const float* times, const float* values,
                                 const float* ts, uint32_t nt, float* out25) {
  Scene_Light light((Light_Type)light_type, 1, Pose{Vec3(pose9[0], pose9[1], pose9[2]), Vec3(pose9[3], pose9[4], pose9[5]), Vec3(pose9[6], pose9[7], pose9[8])});
  light.opt.spectrum = Spectrum(options6[0], options6[1], options6[2]);
  light.opt.intensity = options6[3];
  light.opt.angle_bounds = Vec2(options6[4], options6[5]);
  auto& s = light.lanim.splines;
  for (uint32_t k = offsets[0]; k < offsets[1]; k++) s.head.control_points[times[k]] = spectrum_at(values, k);
  for (uint32_t k = offsets[1]; k < offsets[2]; k++) s.tail.head.control_points[times[k]] = values[4 * k];
  for (uint32_t k = offsets[2]; k < offsets[3]; k++) s.tail.tail.head.control_points[times[k]] = Vec2(values[4 * k], values[4 * k + 1]);
  auto& p = light.anim.splines;
  for (uint32_t k = offsets[3]; k < offsets[4]; k++) p.head.control_points[times[k]] = Vec3(values[4 * k], values[4 * k + 1], values[4 * k + 2]);
  for (uint32_t k = offsets[4]; k < offsets[5]; k++) p.tail.head.values[times[k]] = Quat(values[4 * k], values[4 * k + 1], values[4 * k + 2], values[4 * k + 3]);
  for (uint32_t k = offsets[5]; k < offsets[6]; k++) p.tail.tail.head.control_points[times[k]] = Vec3(values[4 * k], values[4 * k + 1], values[4 * k + 2]);
  for (uint32_t i = 0; i < nt; i++) {
    light.set_time(ts[i]);
    const Spectrum r = light.radiance();
    const Mat4 m = light.pose.transform();
    float* o = out25 + 25 * i;
    o[0] = light.opt.spectrum.r; o[1] = light.opt.spectrum.g; o[2] = light.opt.spectrum.b; o[3] = light.opt.intensity;
    o[4] = light.opt.angle_bounds.x; o[5] = light.opt.angle_bounds.y;
    o[6] = r.r; o[7] = r.g; o[8] = r.b;
    for (int a = 0; a < 16; a++) o[9 + a] = m.data[a];
  }
}

}  // extern "C"
