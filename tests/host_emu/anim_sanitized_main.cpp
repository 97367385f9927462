// TEST-ONLY stand-alone program, built by test_pt_anim_host.py with g++ -fsanitize=address,undefined and run as its own process:
// the table check, the table packing and the host evaluation of soft-rendering-toolsets_amd/csrc/pt_anim.h over the recorded
// fixtures (tests/golden/anim_*.npz, flattened to one binary file by the test) and over malformed offset arrays.
//   anim_sanitized <file>
// file: u32 nobjects, ntimes, nknots; track_offsets[3 nobjects + 1]; knot_times[nknots]; knot_values[4 nknots]; ts[ntimes];
// trans[ntimes][nobjects][16]; u32 nrigs; per rig: u32 njoints, nknots; parent[njoints]; extent[3 njoints]; base[3];
// rest_pose[3 njoints]; knot_offsets[njoints + 1]; knot_times[nknots]; knot_quats[4 nknots]; posed[ntimes][njoints][16].
// Every table is packed the way srt_pt_timeline_create and srt_pt_skin_set_rig pack theirs - exactly offsets[last] knots, in heap
// vectors of exactly that size - so that an index outside a track is an error the sanitizer reports.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pt_anim.h"

namespace {

template <typename T>
bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  v.shrink_to_fit();
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

size_t mismatches(const float* a, const float* b, size_t n) {
  size_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    if (a[i] != a[i] && b[i] != b[i]) continue;
    if (memcmp(a + i, b + i, 4) != 0) bad++;
  }
  return bad;
}

// the packing: exactly what the offsets name
struct Packed { std::vector<uint32_t> offsets; std::vector<float> times, values; };
Packed pack(const uint32_t* offsets, size_t noffsets, const float* times, const float* values) {
  Packed p;
  p.offsets.assign(offsets, offsets + noffsets);
  const size_t nk = offsets[noffsets - 1];
  p.times.assign(times, times + nk);
  p.values.assign(values, values + 4 * nk);
  p.offsets.shrink_to_fit(); p.times.shrink_to_fit(); p.values.shrink_to_fit();
  return p;
}

int expect_refused(const char* what, const std::vector<uint32_t>& offsets, uint32_t nitems, uint32_t per_item, const std::vector<float>& times, bool refuse_empty) {
  const std::string r = srt::anim_check_tracks(offsets.data(), nitems, per_item, times.data(), refuse_empty, "object");
  printf("%-28s %s\n", what, r.empty() ? "ACCEPTED" : r.c_str());
  return r.empty() ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: anim_sanitized <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t h[3];
  if (fread(h, 4, 3, f) != 3) return 2;
  const uint32_t nobj = h[0], nt = h[1], nk = h[2];
  std::vector<uint32_t> offsets;
  std::vector<float> times, values, ts, want;
  if (!read(f, offsets, 3 * (size_t)nobj + 1) || !read(f, times, nk) || !read(f, values, 4 * (size_t)nk) || !read(f, ts, nt) ||
      !read(f, want, (size_t)nt * nobj * 16))
    return 2;
  size_t bad = 0;
  // ---- the recorded objects: check, pack, evaluate ----
  const std::string refused = srt::anim_check_tracks(offsets.data(), nobj, 3, times.data(), true, "object");
  if (!refused.empty()) { printf("the fixture's tables are refused: %s\n", refused.c_str()); bad++; }
  const Packed P = pack(offsets.data(), offsets.size(), times.data(), values.data());
  std::vector<float> got(16 * (size_t)nobj), pose(9 * (size_t)nobj);
  const float specials[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), -0.0f, 1e30f};
  for (uint32_t i = 0; i < nt + 5; i++) {
    const float t = i < nt ? ts[i] : specials[i - nt];              // (a NaN or infinite time reads no knot outside its track either)
    for (uint32_t k = 0; k < nobj; k++) srt::anim_object_transform(P.offsets.data(), P.times.data(), P.values.data(), k, t, &pose[9 * (size_t)k], &got[16 * (size_t)k]);
    if (i < nt) {
      const size_t b = mismatches(got.data(), &want[(size_t)i * nobj * 16], got.size());
      printf("objects, t = %g: %zu mismatches\n", (double)t, b);
      bad += b;
    }
  }
  // ---- malformed offset arrays: each is refused, and refusing it reads nothing outside the arrays ----
  {
    const std::vector<float> t4 = {0.0f, 1.0f, 2.0f, 3.0f};
    std::vector<float> t_nan = t4, t_inf = t4, t_same = t4, t_desc = t4;
    t_nan[1] = std::numeric_limits<float>::quiet_NaN(); t_inf[3] = std::numeric_limits<float>::infinity(); t_same[2] = t_same[1]; t_desc[1] = -1.0f;
    bad += expect_refused("offsets start at 1", {1, 2, 3, 4}, 1, 3, t4, true);
    bad += expect_refused("offsets descend", {0, 3, 2, 4}, 1, 3, t4, true);
    bad += expect_refused("offsets descend to 0", {0, 4, 4, 0}, 1, 3, t4, true);
    bad += expect_refused("all tracks empty", {0, 2, 3, 4, 4, 4, 4}, 2, 3, t4, true);
    bad += expect_refused("first object empty", {0, 0, 0, 0, 1, 2, 4}, 2, 3, t4, true);
    bad += expect_refused("NaN time", {0, 2, 3, 4}, 1, 3, t_nan, true);
    bad += expect_refused("infinite time", {0, 2, 3, 4}, 1, 3, t_inf, true);
    bad += expect_refused("equal times", {0, 4, 4, 4}, 1, 3, t_same, true);
    bad += expect_refused("descending times", {0, 4, 4, 4}, 1, 3, t_desc, true);
    // accepted: equal times in DIFFERENT tracks, an empty joint of a rig, no object at all
    if (!srt::anim_check_tracks(std::vector<uint32_t>{0, 2, 3, 4}.data(), 1, 3, std::vector<float>{0.0f, 1.0f, 1.0f, 1.0f}.data(), true, "object").empty()) bad++;
    if (!srt::anim_check_tracks(std::vector<uint32_t>{0, 0, 2}.data(), 2, 1, std::vector<float>{0.0f, 1.0f}.data(), false, "joint").empty()) bad++;
    if (!srt::anim_check_tracks(std::vector<uint32_t>{0}.data(), 0, 3, std::vector<float>{0.0f}.data(), true, "object").empty()) bad++;
  }
  // ---- the recorded rigs ----
  uint32_t nrigs = 0;
  if (fread(&nrigs, 4, 1, f) != 1) return 2;
  for (uint32_t r = 0; r < nrigs; r++) {
    uint32_t g[2];
    if (fread(g, 4, 2, f) != 2) return 2;
    const uint32_t nj = g[0], rk = g[1];
    std::vector<int32_t> parent;
    std::vector<uint32_t> koff;
    std::vector<float> extent, base, rest, ktimes, kquats, posed_want;
    if (!read(f, parent, nj) || !read(f, extent, 3 * (size_t)nj) || !read(f, base, 3) || !read(f, rest, 3 * (size_t)nj) || !read(f, koff, (size_t)nj + 1) ||
        !read(f, ktimes, rk) || !read(f, kquats, 4 * (size_t)rk) || !read(f, posed_want, (size_t)nt * nj * 16))
      return 2;
    if (!srt::anim_check_tracks(koff.data(), nj, 1, ktimes.data(), false, "joint").empty()) bad++;
    const Packed K = pack(koff.data(), koff.size(), ktimes.data(), kquats.data());
    std::vector<float> cap(4 * (size_t)nj, 0.0f), local(16 * (size_t)nj), posed(16 * (size_t)nj), euler(3 * (size_t)nj);
    for (uint32_t j = 0; j < nj; j++) memcpy(&cap[4 * (size_t)j], &extent[3 * (size_t)j], 12);
    for (uint32_t i = 0; i < nt; i++) {
      srt::anim_rig_posed_host(parent.data(), cap.data(), base.data(), rest.data(), K.offsets.data(), K.times.data(), K.values.data(), nj, ts[i], euler.data(),
                               local.data(), posed.data());
      const size_t b = mismatches(posed.data(), &posed_want[(size_t)i * nj * 16], posed.size());
      printf("rig %u, t = %g: %zu mismatches\n", r, (double)ts[i], b);
      bad += b;
    }
    // a hierarchy that does not end (validation refuses it; the walk is bounded all the same)
    std::vector<int32_t> loop(parent);
    if (nj >= 2) { loop[0] = 1; loop[1] = 0; }
    srt::anim_rig_posed_host(loop.data(), cap.data(), base.data(), rest.data(), K.offsets.data(), K.times.data(), K.values.data(), nj, 0.5f, euler.data(), local.data(),
                             posed.data());
  }
  fclose(f);
  if (bad) { printf("anim_sanitized: FAILED (%zu)\n", bad); return 1; }
  printf("anim_sanitized: ok\n");
  return 0;
}
