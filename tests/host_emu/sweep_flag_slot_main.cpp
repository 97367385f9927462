// TEST-ONLY, stand-alone: the sweeps' flag nibbles through the slot word that is dead between the two sweeps (pt_wave.h: top-down step
// q stores its four flag bits in SLOT(q, r, 1) once tin.y has been read; need_of and the combine read them back, the combine before it
// writes ret.id there; the root keeps its bits in a register) against the 64-bit word of four bits per node that they replace.
// The model below goes through the slots in the kernel's order of reads and writes, with the kernel's index arithmetic, on trees of 2
// to 16 leaves (1 to 15 interior nodes, parents before children), and puts each of the sixteen nibbles on every node in turn.  Every
// value a step reads - tin, the flags, cur_far_t.x, a child's result - must be the one its writer meant.
// Built and run by tests/test_pt_box_minmax_host.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

namespace {

constexpr int NR = 3, LANES = 2;
struct Node { int l_ref, r_ref; };                       // >= 0: interior node, < 0: a leaf

std::vector<float> wl;
int g_lane = 0;
#define SLOT(q, r, f) wl[(size_t)(((((q) - 1) * NR + (r)) * 2 + (f)) * LANES + g_lane)]

float u2f(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// what the writers mean
float tin_x(int q, int r) { return 1000.0f * q + r + 0.25f; }
float tin_y(int q, int r) { return 1000.0f * q + r + 0.5f; }
float farx_of(int q, int r) { return -(float)(q * 8 + r + 1); }
float ret_dist(int q, int r) { return 5000.0f + q * 8 + r; }
uint32_t ret_id(int q, int r) { return 0xABC00000u | (uint32_t)q << 4 | (uint32_t)r; }

unsigned long long g_checks = 0, g_fail = 0;
void same(uint32_t got, uint32_t want, const char* what, int q, int r) {
  g_checks++;
  if (got != want && g_fail++ < 8) std::printf("FAIL: %s at node %d ray %d: got %08x, want %08x\n", what, q, r, got, want);
}

void run(const std::vector<Node>& T, const std::vector<uint32_t>& nib) {
  const int Q = (int)T.size();
  wl.assign((size_t)(Q > 1 ? Q - 1 : 0) * NR * 2 * LANES + 1, u2f(0xDEADBEEFu));
  for (g_lane = 0; g_lane < LANES; g_lane++) {
    unsigned long long fl[NR];
    uint32_t fl0[NR];
    float farx0[NR];
    for (int r = 0; r < NR; r++) { fl[r] = 0ull; fl0[r] = 0u; farx0[r] = 0.0f; }
    // top-down
    for (int q = 0; q < Q; q++) {
      const Node& W = T[q];
      for (int r = 0; r < NR; r++) {
        if (q != 0) {
          const float tx = SLOT(q, r, 0), ty = SLOT(q, r, 1);
          same(f2u(tx), f2u(tin_x(q, r)), "tin.x", q, r);
          same(f2u(ty), f2u(tin_y(q, r)), "tin.y", q, r);
        }
        const uint32_t f = (nib[q] + (uint32_t)r + (uint32_t)g_lane) & 15u;
        fl[r] |= (unsigned long long)f << (4 * q);
        if (q != 0) { SLOT(q, r, 0) = farx_of(q, r); SLOT(q, r, 1) = u2f(f); } else { farx0[r] = farx_of(q, r); fl0[r] = f; }
        if (W.l_ref >= 0) { SLOT(W.l_ref, r, 0) = tin_x(W.l_ref, r); SLOT(W.l_ref, r, 1) = tin_y(W.l_ref, r); }
        if (W.r_ref >= 0) { SLOT(W.r_ref, r, 0) = tin_x(W.r_ref, r); SLOT(W.r_ref, r, 1) = tin_y(W.r_ref, r); }
      }
    }
    // bottom-up
    for (int q = Q - 1; q >= 0; q--) {
      const Node& W = T[q];
      for (int side = 0; side < 2; side++) {             // eval_child
        const int ref = side ? W.r_ref : W.l_ref;
        if (ref >= 0)
          for (int r = 0; r < NR; r++) {
            same(f2u(SLOT(ref, r, 0)), f2u(ret_dist(ref, r)), "child's ret.dist", q, r);
            same(f2u(SLOT(ref, r, 1)), ret_id(ref, r), "child's ret.id", q, r);
          }
      }
      for (int r = 0; r < NR; r++) {                     // need_of
        const uint32_t f = (q != 0) ? f2u(SLOT(q, r, 1)) : fl0[r];
        same(f, (uint32_t)(fl[r] >> (4 * q)) & 15u, "flags in need_of", q, r);
        const float farx = (q != 0) ? SLOT(q, r, 0) : farx0[r];
        same(f2u(farx), f2u(farx_of(q, r)), "cur_far_t.x in need_of", q, r);
      }
      for (int r = 0; r < NR; r++) {                     // the combine
        const uint32_t f = (q != 0) ? f2u(SLOT(q, r, 1)) : fl0[r];
        same(f, (uint32_t)(fl[r] >> (4 * q)) & 15u, "flags in the combine", q, r);
        const float farx = (q != 0) ? SLOT(q, r, 0) : farx0[r];
        same(f2u(farx), f2u(farx_of(q, r)), "cur_far_t.x in the combine", q, r);
        if (q > 0) { SLOT(q, r, 0) = ret_dist(q, r); SLOT(q, r, 1) = u2f(ret_id(q, r)); }
      }
    }
  }
  same(f2u(wl.back()), 0xDEADBEEFu, "the word behind the slots", Q, 0);
}

std::mt19937 rng(7u);

// a tree of `leaves` leaves; interior nodes numbered in the order they are split off (a parent before its children).  shape: 0 the
// left chain, 1 the right chain, 2 breadth first (balanced), 3 random
std::vector<Node> tree(int leaves, int shape) {
  std::vector<Node> T(1, Node{-1, -1});
  std::vector<std::pair<int, int>> slots = {{0, 0}, {0, 1}};   // (node, side) that still hold a leaf
  for (int n = 2; n < leaves; n++) {
    size_t pick = 0;
    if (shape == 0) { for (size_t i = 0; i < slots.size(); i++) if (slots[i].first == (int)T.size() - 1 && slots[i].second == 0) pick = i; }
    else if (shape == 1) { for (size_t i = 0; i < slots.size(); i++) if (slots[i].first == (int)T.size() - 1 && slots[i].second == 1) pick = i; }
    else if (shape == 2) pick = 0;
    else pick = rng() % slots.size();
    const std::pair<int, int> s = slots[pick];
    slots.erase(slots.begin() + pick);
    const int id = (int)T.size();
    T.push_back(Node{-1, -1});
    if (s.second == 0) T[s.first].l_ref = id; else T[s.first].r_ref = id;
    slots.push_back({id, 0}); slots.push_back({id, 1});
  }
  return T;
}

}  // namespace

int main() {
  unsigned long long runs = 0;
  for (int leaves = 2; leaves <= 16; leaves++)
    for (int shape = 0; shape < 6; shape++) {              // shapes 3, 4, 5: three random trees
      const std::vector<Node> T = tree(leaves, shape < 3 ? shape : 3);
      const int Q = (int)T.size();
      if (Q != leaves - 1) { std::printf("tree of %d leaves has %d interior nodes\n", leaves, Q); return 1; }
      for (int q = 0; q < Q; q++)
        for (uint32_t n = 0; n < 16u; n++) {
          std::vector<uint32_t> nib(Q);
          for (int k = 0; k < Q; k++) nib[k] = rng() & 15u;
          nib[q] = n;                                      // (with the ray and lane offsets every node sees all sixteen)
          run(T, nib);
          runs++;
        }
    }
  std::printf("trees of 2..16 leaves, %llu sweeps, %llu reads checked, failures: %llu\n", runs, g_checks, g_fail);
  if (g_fail) return 1;
  std::printf("sweep_flag_slot: ok\n");
  return 0;
}
