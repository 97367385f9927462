// Host module of the shading-timeline tests (tests/_shading_cases.py builds it with g++ -ffp-contract=off): the item functions of
// pt_anim.h - anim_material_options / anim_material_values / anim_material_store, anim_light_item, anim_env_item - one item at a
// time on the CPU, for comparison with what the reference recorded (tests/golden/anim_shading.npz).  With -DSHADING_HOST_MAIN the
// same file is a stand-alone program (built with -fsanitize=address,undefined and run as its own process) that evaluates a flat
// file of keys, compares with the recorded numbers in it and then runs the table check and the evaluation over hostile inputs.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_anim.h"

using namespace srt;

extern "C" {

// options14: albedo3 reflectance3 transmittance3 emissive3 intensity ior; values7: a3 b3 ior as srt_pt_update_materials takes them;
// stored3: `a` of the record the kernels read.
void shading_emu_materials(const uint32_t* offsets, const float* times, const float* values, const uint32_t* types, uint32_t n, float t, float* options14,
                           float* values7, float* stored3) {
  for (uint32_t k = 0; k < n; k++) {
    const AnimMaterialOptions p = anim_material_options(offsets + 6 * (size_t)k, times, values, t);
    const float o[14] = {p.albedo.x, p.albedo.y, p.albedo.z, p.reflectance.x, p.reflectance.y, p.reflectance.z, p.transmittance.x, p.transmittance.y,
                         p.transmittance.z, p.emissive.x, p.emissive.y, p.emissive.z, p.intensity, p.ior};
    std::memcpy(options14 + 14 * (size_t)k, o, sizeof o);
    Material m;
    m.type = types[k];
    anim_material_item(offsets, times, values, k, t, &m);
    float* v = values7 + 7 * (size_t)k;
    for (int i = 0; i < 3; i++) { v[i] = m.a[i]; v[3 + i] = m.b[i]; }
    v[6] = m.ior;
    anim_material_store(&m);
    for (int i = 0; i < 3; i++) stored3[3 * (size_t)k + i] = m.a[i];
  }
}

// flags2: {option triple keyed, pose triple keyed}; out21: radiance3 angle_bounds2 trans16, entries of a triple without a key left alone.
void shading_emu_lights(const uint32_t* offsets, const float* times, const float* values, uint32_t n, float t, uint32_t* flags2, float* out21) {
  for (uint32_t j = 0; j < n; j++) {
    AnimLightOut out;
    anim_light_item(offsets + 6 * (size_t)j, times, values, t, &out);
    flags2[2 * (size_t)j] = out.options; flags2[2 * (size_t)j + 1] = out.pose;
    float* o = out21 + 21 * (size_t)j;
    if (out.options) { std::memcpy(o, out.radiance, sizeof out.radiance); std::memcpy(o + 3, out.angle_bounds, sizeof out.angle_bounds); }
    if (out.pose) std::memcpy(o + 5, out.trans, sizeof out.trans);
  }
}

void shading_emu_env(const uint32_t* offsets3, const float* times, const float* values, float t, float* radiance3) { anim_env_item(offsets3, times, values, t, radiance3); }

float shading_emu_to_linear(float f) { return anim_to_linear(f); }

}  // extern "C"

#ifdef SHADING_HOST_MAIN
namespace {

bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }

template <typename T>
bool read(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || fread(v->data(), sizeof(T), n, f) == n;
}

}  // namespace

// File: {nm, nl, env, nt, nk} uint32; types[nm]; offsets[6 nm + 6 nl + 2 env + 1]; times[nk]; values[4 nk]; ts[nt]; then per time the
// expected values7[nm], stored3[nm], flags2[nl] (uint32), lights21[nl] and env3.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t head[5];
  if (fread(head, 4, 5, f) != 5) return 2;
  const uint32_t nm = head[0], nl = head[1], env = head[2], nt = head[3], nk = head[4];
  const size_t ntracks = 6 * (size_t)nm + 6 * (size_t)nl + 2 * (size_t)env;
  std::vector<uint32_t> types, offsets, flags;
  std::vector<float> times, values, ts, want7, want3, want21, wantenv;
  if (!read(f, &types, nm) || !read(f, &offsets, ntracks + 1) || !read(f, &times, nk) || !read(f, &values, 4 * (size_t)nk) || !read(f, &ts, nt)) return 2;
  const std::string refused = anim_check_tracks(offsets.data(), (uint32_t)ntracks, 1, times.data(), false, "track");
  if (!refused.empty()) { printf("the recorded tables are refused: %s\n", refused.c_str()); return 1; }
  size_t bad = 0;
  std::vector<float> o14(14 * (size_t)nm), v7(7 * (size_t)nm), s3(3 * (size_t)nm), l21(21 * (size_t)nl);
  std::vector<uint32_t> fl(2 * (size_t)nl);
  for (uint32_t i = 0; i < nt; i++) {
    if (!read(f, &want7, 7 * (size_t)nm) || !read(f, &want3, 3 * (size_t)nm) || !read(f, &flags, 2 * (size_t)nl) || !read(f, &want21, 21 * (size_t)nl) || !read(f, &wantenv, 3)) return 2;
    shading_emu_materials(offsets.data(), times.data(), values.data(), types.data(), nm, ts[i], o14.data(), v7.data(), s3.data());
    std::fill(l21.begin(), l21.end(), 0.0f);
    shading_emu_lights(offsets.data() + 6 * (size_t)nm, times.data(), values.data(), nl, ts[i], fl.data(), l21.data());
    for (size_t q = 0; q < v7.size(); q++) bad += !same(v7[q], want7[q]);
    for (size_t q = 0; q < s3.size(); q++) bad += !same(s3[q], want3[q]);
    for (size_t j = 0; j < nl; j++) {
      bad += fl[2 * j] != flags[2 * j] || fl[2 * j + 1] != flags[2 * j + 1];
      for (int a = 0; a < 21; a++)
        if (a < 5 ? flags[2 * j] : flags[2 * j + 1]) bad += !same(l21[21 * j + a], want21[21 * j + a]);
    }
    if (env) {
      float e[3];
      shading_emu_env(offsets.data() + 6 * (size_t)nm + 6 * (size_t)nl, times.data(), values.data(), ts[i], e);
      for (int a = 0; a < 3; a++) bad += !same(e[a], wantenv[a]);
    }
  }
  fclose(f);
  if (bad) { printf("%zu values differ from the recorded ones\n", bad); return 1; }
  // hostile inputs: query times no track holds, and tables the check has to refuse (an ACCEPTED line is a failure)
  const float odd[] = {NAN, INFINITY, -INFINITY, 3.4e38f, -3.4e38f, 1e-45f};
  for (float t : odd) {
    shading_emu_materials(offsets.data(), times.data(), values.data(), types.data(), nm, t, o14.data(), v7.data(), s3.data());
    shading_emu_lights(offsets.data() + 6 * (size_t)nm, times.data(), values.data(), nl, t, fl.data(), l21.data());
  }
  const float channels[] = {NAN, INFINITY, -INFINITY, 3.4e38f, -3.4e38f, 0.04045f, 0.040450003f, 0.0f, -0.0f, 1e-45f};
  for (float c : channels) (void)shading_emu_to_linear(c);
  if (!(shading_emu_to_linear(INFINITY) == INFINITY) || !(shading_emu_to_linear(-INFINITY) == -INFINITY) || shading_emu_to_linear(NAN) == shading_emu_to_linear(NAN)) {
    printf("to_linear of a non-finite channel\n");
    return 1;
  }
  if (nk >= 2 && ntracks >= 1) {
    auto refuses = [&](const std::vector<uint32_t>& off, const std::vector<float>& tm, const char* name) {
      if (anim_check_tracks(off.data(), (uint32_t)ntracks, 1, tm.data(), false, "track").empty()) printf("ACCEPTED: %s\n", name);
    };
    size_t long_track = 0;
    while (long_track < ntracks && offsets[long_track + 1] - offsets[long_track] < 2) long_track++;
    if (long_track == ntracks) { printf("no track with two knots\n"); return 1; }
    std::vector<uint32_t> off = offsets;
    off[0] = 1; refuses(off, times, "offsets that start at 1");
    off = offsets; off[long_track + 1] = off[long_track] - (off[long_track] ? 1u : 0u) - (off[long_track] ? 0u : 0u);
    if (off[long_track]) refuses(off, times, "offsets that descend");
    for (float v : {NAN, INFINITY, times[offsets[long_track]]}) {
      std::vector<float> tm = times;
      tm[offsets[long_track] + 1] = v;
      refuses(offsets, tm, "a time that is not finite or does not ascend");
    }
  }
  printf("shading_sanitized: ok (%u materials, %u lights, %u times)\n", nm, nl, nt);
  return 0;
}
#endif
