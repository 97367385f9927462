// TEST-ONLY stand-alone program, built by test_pt_ik_host.py with g++ -fsanitize=address,undefined and run as its own process: the
// handle-table check, the CSR construction and the host solve of soft-rendering-toolsets_amd/csrc/pt_ik.h over the recorded
// fixtures (tests/golden/ik_*.npz, flattened to one binary file by the test), a handle on every joint, the maximum handle count
// and one past it, and handle lists that name joints out of range.
//   ik_sanitized <file>
// file: u32 nrigs; per rig: u32 njoints, nhandles, ncalls; parent[njoints]; extent[3 njoints]; handle_joints[nhandles];
// targets[ncalls][nhandles][3]; enabled[ncalls][nhandles] (bytes); pose_before[ncalls][njoints][3]; pose_after[ncalls][njoints][3].
// Every array lives in a heap vector of exactly its size, so that an index outside a table is an error the sanitizer reports.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_ik.h"

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

struct Rig { uint32_t nj; std::vector<int32_t> parent; std::vector<float> cap; };

// What srt_pt_rig_step_ik_host does behind its checks: 0 solved, 1 unsupported, 2 invalid.
int solve(const Rig& R, const std::vector<uint32_t>& hj, const std::vector<float>& targets, const uint8_t* enabled, std::vector<float>& pose) {
  const uint32_t nh = (uint32_t)hj.size();
  if (!srt::ik_supported(R.nj, nh)) return 1;
  if (!srt::ik_check_handles(hj.data(), nh, R.nj).empty()) return 2;
  std::vector<uint32_t> off, list;
  srt::ik_build_csr(R.parent.data(), R.nj, hj.data(), nh, off, list);
  off.shrink_to_fit(); list.shrink_to_fit();
  // the lists ascend and name handles whose chain holds the joint
  for (uint32_t j = 0; j < R.nj; j++)
    for (uint32_t k = off[j]; k < off[j + 1]; k++) {
      if (k > off[j] && list[k - 1] >= list[k]) return 3;
      bool holds = false;
      for (int32_t c = (int32_t)hj[list[k]]; c >= 0; c = R.parent[c]) holds = holds || (uint32_t)c == j;
      if (!holds) return 3;
    }
  std::vector<float> scratch((size_t)srt::kIkJointFloats * R.nj);
  srt::ik_step_host(R.parent.data(), R.cap.data(), R.nj, hj.data(), off.data(), list.data(), targets.data(), enabled, scratch.data(), pose.data());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: ik_sanitized <file>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t nrigs = 0;
  if (fread(&nrigs, 4, 1, f) != 1) return 2;
  size_t bad = 0;
  for (uint32_t r = 0; r < nrigs; r++) {
    uint32_t h[3];
    if (fread(h, 4, 3, f) != 3) return 2;
    const uint32_t nj = h[0], nh = h[1], K = h[2];
    Rig R;
    R.nj = nj;
    std::vector<float> extent, targets, before, after;
    std::vector<uint32_t> hj;
    std::vector<uint8_t> enabled;
    if (!read(f, R.parent, nj) || !read(f, extent, 3 * (size_t)nj) || !read(f, hj, nh) || !read(f, targets, (size_t)K * nh * 3) || !read(f, enabled, (size_t)K * nh) ||
        !read(f, before, (size_t)K * nj * 3) || !read(f, after, (size_t)K * nj * 3))
      return 2;
    R.cap.assign(4 * (size_t)nj, 0.0f);
    R.cap.shrink_to_fit();
    for (uint32_t j = 0; j < nj; j++) memcpy(&R.cap[4 * (size_t)j], &extent[3 * (size_t)j], 12);
    // ---- the recorded calls ----
    for (uint32_t c = 0; c < K; c++) {
      std::vector<float> pose(before.begin() + (size_t)c * nj * 3, before.begin() + (size_t)(c + 1) * nj * 3);
      const std::vector<float> t(targets.begin() + (size_t)c * nh * 3, targets.begin() + (size_t)(c + 1) * nh * 3);
      const std::vector<uint8_t> e(enabled.begin() + (size_t)c * nh, enabled.begin() + (size_t)(c + 1) * nh);
      pose.shrink_to_fit();
      const int st = solve(R, hj, t, e.data(), pose);
      const size_t b = st ? 1 : mismatches(pose.data(), &after[(size_t)c * nj * 3], pose.size());
      printf("rig %u, call %u: status %d, %zu mismatches\n", r, c, st, b);
      bad += b;
    }
    const std::vector<float> first(before.begin(), before.begin() + (size_t)nj * 3);
    // ---- no handle at all; a handle on every joint; the maximum count; one past it; joints out of range ----
    {
      std::vector<float> pose(first);
      if (solve(R, {}, {}, nullptr, pose) != 0 || mismatches(pose.data(), first.data(), pose.size())) { printf("rig %u: no handles changed the pose\n", r); bad++; }
    }
    for (uint32_t n : {nj, srt::kIkMaxHandles, srt::kIkMaxHandles + 1u}) {
      std::vector<uint32_t> every(n);
      std::vector<float> t(3 * (size_t)n);
      for (uint32_t i = 0; i < n; i++) { every[i] = i % nj; t[3 * (size_t)i] = 1.0f + 0.001f * i; t[3 * (size_t)i + 1] = 2.0f; t[3 * (size_t)i + 2] = -1.5f; }
      every.shrink_to_fit(); t.shrink_to_fit();
      std::vector<float> pose(first);
      const int want = n > srt::kIkMaxHandles ? 1 : 0;         // one past the limit is refused before anything is built
      const int st = solve(R, every, t, nullptr, pose);
      printf("rig %u, %u handles: status %d\n", r, n, st);
      if (st != want || (want && mismatches(pose.data(), first.data(), pose.size()))) bad++;
    }
    for (uint32_t wrong : {nj, nj + 1u, 0xffffffffu}) {
      std::vector<uint32_t> list(hj);
      list.push_back(wrong);
      list.shrink_to_fit();
      std::vector<float> t(3 * list.size(), 0.5f), pose(first);
      const int st = solve(R, list, t, nullptr, pose);
      if (st != 2 || mismatches(pose.data(), first.data(), pose.size())) { printf("rig %u: joint %u was not refused (status %d)\n", r, wrong, st); bad++; }
    }
  }
  fclose(f);
  if (bad) { printf("ik_sanitized: FAILED (%zu)\n", bad); return 1; }
  printf("ik_sanitized: ok\n");
  return 0;
}
