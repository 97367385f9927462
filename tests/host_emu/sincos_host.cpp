// TEST-ONLY: the branch-free srt_sincosf / srt_sincosf2 (pt_device.h) compiled for the host next to the _plain forms they restate.
// Built by tests/test_pt_sincos_host.py with g++ -ffp-contract=off as a library; with -DSINCOS_HOST_MAIN and
// -fsanitize=undefined as a program of its own over the arguments whose double -> int32 conversion the functions must keep defined.
#include "pt_device.h"

#include <cstdio>
#include <thread>
#include <vector>

using namespace srt;

namespace {

// new and plain forms on one argument: 0 when all four values agree bit for bit
inline int differs(float y) {
  float c, s, pc, ps;
  srt_sincosf2(y, c, s);
  srt_sincosf2_plain(y, pc, ps);
  const float c1 = srt_sincosf(y, 1), s1 = srt_sincosf(y, 0);
  const float pc1 = srt_sincosf_plain(y, 1), ps1 = srt_sincosf_plain(y, 0);
  return (f2u(c) != f2u(pc)) | (f2u(s) != f2u(ps)) | (f2u(c1) != f2u(pc1)) | (f2u(s1) != f2u(ps1));
}

}  // namespace

// Every float whose magnitude bits lie in [lo, hi), in both signs, on `threads` threads (1..16).  Returns the number of arguments
// on which a new form differs from its plain form; first_bad takes the bits of the smallest-magnitude one (0xffffffff without).
extern "C" uint64_t sincos_sweep(uint32_t lo, uint32_t hi, int threads, uint32_t* first_bad) {
  if (threads < 1) threads = 1;
  if (threads > 16) threads = 16;
  std::vector<uint64_t> bad(threads, 0);
  std::vector<uint32_t> first(threads, 0xffffffffu);
  std::vector<std::thread> pool;
  const uint64_t span = (uint64_t)hi - lo, chunk = (span + threads - 1) / threads;
  for (int t = 0; t < threads; t++)
    pool.emplace_back([&, t] {
      const uint64_t a = lo + chunk * t, b = (a + chunk < hi) ? a + chunk : hi;
      for (uint64_t u = a; u < b; u++)
        for (uint32_t sign = 0; sign < 2; sign++) {
          const uint32_t bits = (uint32_t)u | (sign << 31);
          if (differs(u2f(bits))) {
            bad[t]++;
            if (first[t] == 0xffffffffu) first[t] = bits;
          }
        }
    });
  for (auto& th : pool) th.join();
  uint64_t total = 0;
  uint32_t f = 0xffffffffu;
  for (int t = 0; t < threads; t++) {
    total += bad[t];
    if (first[t] != 0xffffffffu && (f == 0xffffffffu || (first[t] & 0x7fffffffu) < (f & 0x7fffffffu))) f = first[t];
  }
  if (first_bad) *first_bad = f;
  return total;
}

// The new forms on n arguments: srt_sincosf2 into c2 / s2, srt_sincosf(., 1) and (., 0) into c1 / s1.
extern "C" void sincos_eval(const float* x, size_t n, float* c2, float* s2, float* c1, float* s1) {
  for (size_t i = 0; i < n; i++) {
    srt_sincosf2(x[i], c2[i], s2[i]);
    c1[i] = srt_sincosf(x[i], 1);
    s1[i] = srt_sincosf(x[i], 0);
  }
}

#ifdef SINCOS_HOST_MAIN
int main() {
  const uint32_t args[] = {
      0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7fffffffu,           // NaNs
      0x7f800000u, 0xff800000u,                                     // infinities
      0x00000000u, 0x80000000u,                                     // zeros
      0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu,           // denormals
      0x00800000u, 0x39800000u, 0x397fffffu,                        // smallest normal, 2^-12 and its neighbour
      0x42efffffu, 0x42f00000u, 0xc2f00000u, 0x42f00001u,           // around 120
      0x43000000u, 0x4f000000u, 0xcf000000u, 0x4f000001u,           // 128, +-2^31 and above
      0x5f000000u, 0x7f7fffffu, 0xff7fffffu};                       // 2^63, +-FLT_MAX
  int failed = 0;
  for (uint32_t bits : args) {
    const float y = u2f(bits);
    float c, s;
    srt_sincosf2(y, c, s);
    const float c1 = srt_sincosf(y, 1), s1 = srt_sincosf(y, 0);
    const int d = differs(y);
    std::printf("%08x -> cos %08x sin %08x | %08x %08x%s\n", bits, f2u(c), f2u(s), f2u(c1), f2u(s1), d ? "  DIFFERS" : "");
    failed |= d;
  }
  // one exponent step on both sides of 120, every 997th pattern, both signs
  for (uint32_t u = 0x42000000u; u < 0x43800000u; u += 997u) failed |= differs(u2f(u)) | differs(u2f(u | 0x80000000u));
  if (failed) { std::printf("sincos_sanitized: FAILED\n"); return 1; }
  std::printf("sincos_sanitized: ok (%zu arguments)\n", sizeof(args) / sizeof(args[0]));
  return 0;
}
#endif
