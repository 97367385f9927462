// TEST-ONLY, stand-alone: the top-down step's box tests from per-axis min / max (box_hit_minmax, topdown_step<true>, pt_trace.h)
// against the form they stand in for (box_hit_inv, topdown_step<false>) on inputs that pass the guard, and the guard's predicates
// on inputs that must fail them.  Built and run by tests/test_pt_box_minmax_host.py with g++ -ffp-contract=off.
//   Hit flags, the four flag bits (child order among them): equal.  times, cur_far_t.x and the children's times: equal as values,
//   bit-equal wherever the value is not a zero; zeros of the other sign are counted and reported, not failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "pt_trace.h"

using namespace srt;

namespace {

struct Set { float bl[6], br[6]; V3 org, inv; float tx, ty, rb0, rb1; };

unsigned long long g_sets = 0, g_zero_signs = 0, g_fail = 0, g_skipped = 0;
unsigned long long g_flags[16] = {0};

// 0 = the same bits, 1 = zeros of different sign, 2 = different
int cmp(float a, float b) {
  const uint32_t x = __float_as_uint(a), y = __float_as_uint(b);
  if (x == y) return 0;
  if (a == 0.0f && b == 0.0f) return 1;
  return 2;
}

bool guard(const Set& s) { return minmax_box_ok(s.bl) && minmax_box_ok(s.br) && minmax_origin_ok(s.org) && minmax_inv_ok(s.inv); }

void check(const Set& s, const char* what) {
  if (!guard(s)) { g_skipped++; return; }                // (constructed sets may leave the guard's domain: those are not claims)
  g_sets++;
  int worst = 0;
  auto both = [&](float a, float b) { const int c = cmp(a, b); if (c == 1) g_zero_signs++; if (c > worst) worst = c; };
  // one box
  float ax = s.tx, ay = s.ty, bx = s.tx, by = s.ty;
  const bool ha = box_hit_inv(s.bl, s.org, s.inv, ax, ay);
  const bool hb = box_hit_minmax(s.bl, s.org, s.inv, bx, by);
  both(ax, bx); both(ay, by);
  // the step
  WaveInterior W;
  for (int j = 0; j < 6; j++) { W.boxl[j] = s.bl[j]; W.boxr[j] = s.br[j]; }
  W.l_ref = 1; W.r_ref = 2; W.l_cnt = W.r_cnt = 0u;
  float f0, l0x, l0y, r0x, r0y, f1, l1x, l1y, r1x, r1y;
  const uint32_t fa = topdown_step<false>(W, s.org, s.inv, s.tx, s.ty, s.rb0, s.rb1, f0, l0x, l0y, r0x, r0y);
  const uint32_t fb = topdown_step<true>(W, s.org, s.inv, s.tx, s.ty, s.rb0, s.rb1, f1, l1x, l1y, r1x, r1y);
  both(f0, f1); both(l0x, l1x); both(l0y, l1y); both(r0x, r1x); both(r0y, r1y);
  g_flags[fa & 15u]++;
  if (ha != hb || fa != fb || worst == 2) {
    if (g_fail++ < 8)
      std::printf("FAIL (%s): hit %d %d flags %u %u  times %a %a | %a %a  farx %a %a  l %a %a | %a %a  r %a %a | %a %a\n", what, ha, hb, fa, fb,
                  ax, ay, bx, by, f0, f1, l0x, l0y, l1x, l1y, r0x, r0y, r1x, r1y);
  }
}

std::mt19937 rng(20240607u);
float uni(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }

Set random_set() {
  Set s;
  for (int a = 0; a < 3; a++) {
    float p = uni(-1, 1), q = uni(-1, 1);
    s.bl[a] = std::fmin(p, q); s.bl[3 + a] = std::fmax(p, q);
    p = uni(-1, 1); q = uni(-1, 1);
    s.br[a] = std::fmin(p, q); s.br[3 + a] = std::fmax(p, q);
  }
  if (rng() % 10u == 0u) for (int j = 0; j < 6; j++) s.br[j] = s.bl[j];   // the same box twice: equal entry times
  s.org = v3(uni(-2, 2), uni(-2, 2), uni(-2, 2));
  V3 d = v3(uni(-0.7f, 0.7f) - s.org.x, uni(-0.7f, 0.7f) - s.org.y, uni(-0.7f, 0.7f) - s.org.z);
  if (d.x == 0.0f) d.x = 0.125f;
  if (d.y == 0.0f) d.y = 0.125f;
  if (d.z == 0.0f) d.z = 0.125f;
  const float n = std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
  s.inv = v3(1.0f / (d.x / n), 1.0f / (d.y / n), 1.0f / (d.z / n));
  const bool cam = (rng() & 1u) != 0u;
  s.rb0 = cam ? 0.0f : 0.001f; s.rb1 = cam ? INFINITY : std::numeric_limits<float>::max();
  s.tx = s.rb0; s.ty = s.rb1;
  return s;
}

// the `times` a step can be handed: dist_bounds, NaN, inverted, infinite, a window that cuts the box
void all_times(Set s, const char* what) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float t[][2] = {{s.rb0, s.rb1}, {nan, INFINITY}, {0.0f, nan}, {nan, nan}, {3.0f, 1.0f}, {1.0f, 2.5f}, {-INFINITY, INFINITY},
                        {INFINITY, INFINITY}, {-INFINITY, -INFINITY}, {INFINITY, -INFINITY}, {0.0f, 0.0f}, {-0.0f, 0.0f}, {0.0f, -0.0f}};
  for (const auto& p : t) { s.tx = p[0]; s.ty = p[1]; check(s, what); }
}

Set scaled(Set s, float k) {
  for (int j = 0; j < 6; j++) { s.bl[j] *= k; s.br[j] *= k; }
  s.org = s.org * k;
  s.inv = v3(s.inv.x / k, s.inv.y / k, s.inv.z / k);    // (t scales with the geometry: dist_bounds and times with it)
  s.tx *= k; s.ty *= k; s.rb0 *= k; s.rb1 *= k;
  return s;
}

void constructed() {
  const float big[] = {0x1p100f, -0x1p100f, 0x1p127f, -0x1p127f, std::numeric_limits<float>::max()};
  const float tiny[] = {0x1p-149f, -0x1p-149f, 0x1p-130f, -0x1p-127f, 0x1p-126f};
  for (int i = 0; i < 512; i++) {
    const Set b = random_set();
    // flat boxes: lo == hi on one, two or three axes, left, right or both
    for (int m = 1; m < 8; m++)
      for (int side = 1; side < 4; side++) {
        Set s = b;
        for (int a = 0; a < 3; a++)
          if (m >> a & 1) { if (side & 1) s.bl[3 + a] = s.bl[a]; if (side & 2) s.br[3 + a] = s.br[a]; }
        all_times(s, "flat box");
        // ... seen from a point in its plane
        for (int a = 0; a < 3; a++) if (m >> a & 1) { if (a == 0) s.org.x = s.bl[0]; if (a == 1) s.org.y = s.bl[1]; if (a == 2) s.org.z = s.bl[2]; }
        all_times(s, "flat box, origin in its plane");
      }
    // origins on a face, an edge or a corner of the left box (lo or hi per axis), and inside it otherwise
    for (int m = 1; m < 8; m++)
      for (int hi = 0; hi < 8; hi++) {
        Set s = b;
        float o[3] = {0.5f * (s.bl[0] + s.bl[3]), 0.5f * (s.bl[1] + s.bl[4]), 0.5f * (s.bl[2] + s.bl[5])};
        for (int a = 0; a < 3; a++) if (m >> a & 1) o[a] = s.bl[(hi >> a & 1) ? 3 + a : a];
        s.org = v3(o[0], o[1], o[2]);
        all_times(s, "origin on the box");
      }
    // reciprocals so small that both products of an axis round to the same number (l == h), and so large that they overflow
    for (int a = 0; a < 3; a++) {
      for (float v : tiny) { Set s = b; if (a == 0) s.inv.x = v; if (a == 1) s.inv.y = v; if (a == 2) s.inv.z = v; all_times(s, "l == h"); }
      for (float v : big) { Set s = b; if (a == 0) s.inv.x = v; if (a == 1) s.inv.y = v; if (a == 2) s.inv.z = v; all_times(s, "overflow"); }
    }
    for (float v : big) { Set s = b; s.inv = v3(v, -v, v); all_times(s, "overflow on every axis"); }
    for (float v : tiny) { Set s = b; s.inv = v3(v, v, -v); all_times(s, "l == h on every axis"); }
    { Set s = b; s.org = v3(0x1p127f, -0x1p127f, 0x1p127f); for (int j = 0; j < 6; j++) { s.bl[j] *= 0x1p127f; s.br[j] *= 0x1p127f; } all_times(s, "b - o overflows"); }
    // the set scaled by 2^+-40
    all_times(scaled(b, 0x1p40f), "scaled up");
    all_times(scaled(b, 0x1p-40f), "scaled down");
  }
}

int g_guard_fail = 0;
void expect(bool got, bool want, const char* what) {
  if (got != want) { g_guard_fail++; std::printf("GUARD: %s: got %d, want %d\n", what, got, want); }
}

void guard_predicates() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = INFINITY;
  const float good_box[6] = {-1, -2, -3, 1, 2, 3}, flat_box[6] = {-1, 2, -3, 1, 2, 3};
  expect(minmax_box_ok(good_box), true, "a finite ordered box");
  expect(minmax_box_ok(flat_box), true, "a flat box");
  expect(minmax_origin_ok(v3(0.0f, -0.0f, 0x1p-149f)), true, "zeros and a denormal in the origin");
  expect(minmax_inv_ok(v3(0x1p-149f, -0x1p127f, 1.0f)), true, "a denormal and a huge reciprocal");
  const float bad[] = {0.0f, -0.0f, inf, -inf, nan, -nan};
  for (float v : bad)
    for (int a = 0; a < 3; a++) {
      const V3 i = v3(a == 0 ? v : 1.0f, a == 1 ? v : -2.0f, a == 2 ? v : 0.5f);
      expect(minmax_inv_ok(i), false, "a zero, infinite or NaN reciprocal");
    }
  const float bad_o[] = {inf, -inf, nan, -nan};
  for (float v : bad_o)
    for (int a = 0; a < 3; a++) {
      const V3 o = v3(a == 0 ? v : 1.0f, a == 1 ? v : -2.0f, a == 2 ? v : 0.5f);
      expect(minmax_origin_ok(o), false, "a non-finite origin");
    }
  for (float v : bad_o)
    for (int j = 0; j < 6; j++) {
      float bx[6];
      for (int k = 0; k < 6; k++) bx[k] = good_box[k];
      bx[j] = v;
      expect(minmax_box_ok(bx), false, "a non-finite bound");
    }
  for (int a = 0; a < 3; a++) {
    float bx[6];
    for (int k = 0; k < 6; k++) bx[k] = good_box[k];
    bx[a] = good_box[3 + a]; bx[3 + a] = good_box[a];
    expect(minmax_box_ok(bx), false, "an inverted box");
  }
  const float fmax = std::numeric_limits<float>::max();
  const float empty[6] = {fmax, fmax, fmax, -fmax, -fmax, -fmax};
  expect(minmax_box_ok(empty), false, "the empty box");
}

}  // namespace

int main() {
  for (int i = 0; i < (1 << 18); i++) {
    Set s = random_set();
    switch (rng() % 8u) {                                // most keep dist_bounds as their times
      case 1: s.tx = std::numeric_limits<float>::quiet_NaN(); s.ty = INFINITY; break;
      case 2: s.tx = 3.0f; s.ty = 1.0f; break;
      case 3: s.tx = 0.0f; s.ty = std::numeric_limits<float>::quiet_NaN(); break;
      case 4: s.tx = 1.0f; s.ty = 2.5f; break;
      default: break;
    }
    check(s, "random");
  }
  const unsigned long long n_random = g_sets;
  constructed();
  guard_predicates();
  std::printf("sets: %llu random, %llu constructed (%llu more outside the guard), zeros of the other sign: %llu, failures: %llu, guard failures: %d\n",
              n_random, g_sets - n_random, g_skipped, g_zero_signs, g_fail, g_guard_fail);
  std::printf("flag nibbles:");
  for (int f = 0; f < 16; f++) std::printf(" %llu", g_flags[f]);
  std::printf("\n");
  if (n_random != (1ull << 18) || g_fail != 0 || g_guard_fail != 0) return 1;
  std::printf("box_minmax: ok\n");
  return 0;
}
