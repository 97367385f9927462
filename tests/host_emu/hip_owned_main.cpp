// TEST-ONLY: the owners of csrc/hip_owned.h (DeviceBuffer, PinnedBuffer, Event, Stream) against the counting stand-in for the HIP runtime
// (tests/host_emu/hip_counting/), as a stand-alone program that tests/test_hip_owned_host.py builds with AddressSanitizer and
// UndefinedBehaviorSanitizer and runs once.  A double free, a use after free or a leak ends the run with the sanitizer's report.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "pt_bvh_device.h"   // RefitTables and BvhWorkspace as the library declares them (includes hip_owned.h)

namespace srt {
static int g_fails = 0;
int fail(int status, const char*, ...) { g_fails++; return status; }
}  // namespace srt
using namespace srt;

#define CHECK(cond) do { if (!(cond)) { std::printf("hip_owned: line %d: %s\n  log \"%s\"\n", __LINE__, #cond, hip_counting().log.c_str()); std::exit(1); } } while (0)

static HipCounting& C = hip_counting();
static std::string take_log() { std::string l; l.swap(C.log); return l; }
static uint64_t live(OwnedKind k) { return owned_live(k).load(); }
static bool all_gone() {
  return C.device_blocks == 0 && C.pinned_blocks == 0 && C.events == 0 && C.streams == 0 && live(OWNED_DEVICE) == 0 && live(OWNED_PINNED) == 0 &&
         live(OWNED_EVENT) == 0 && live(OWNED_STREAM) == 0;
}

// An empty owner makes no call at all: construction, reset(), moves, destruction.
// Shaped like one rank's slot of a group lane (pt_group.cpp: LaneRank).
struct LaneSlot { Stream stream; Event event; DeviceBuffer<float> tiles; };

static void empty_owners() {
  {
    DeviceBuffer<float> a, b(std::move(a)); PinnedBuffer<uint32_t> p, q(std::move(p)); Event e, f(std::move(e));
    Stream s, t(std::move(s));
    DeviceBuffer<void> v;
    a = std::move(b); p = std::move(q); e = std::move(f); s = std::move(t);
    a.reset(); p.reset(); e.reset(); s.reset(); v.reset();
    CHECK(!a && a.capacity() == 0 && !p && p.capacity() == 0 && p.device() == nullptr && (hipEvent_t)e == nullptr && (hipStream_t)s == nullptr);
    LaneSlot L, M(std::move(L));
    L = std::move(M);
    RefitTables T, U(std::move(T));
    T = std::move(U);
    BvhWorkspace W;
  }
  CHECK(take_log().empty() && all_gone());
}

static void device_buffer() {
  {
    DeviceBuffer<float> a;
    CHECK(a.ensure(10) == SRT_OK && a && a.capacity() == 10 && C.last_alloc_bytes == 40 && take_log() == "m" && live(OWNED_DEVICE) == 1);
    float* const first = a;
    CHECK(a.ensure(10) == SRT_OK && a.ensure(3) == SRT_OK && a == first && a.capacity() == 10 && take_log().empty());   // enough: no call
    CHECK(a.ensure(11) == SRT_OK && a.capacity() == 11 && C.last_alloc_bytes == 44 && take_log() == "fm");               // grows: free, then malloc
    a[10] = 1.0f;                                           // (the whole capacity is the caller's)
    // a failed ensure leaves nothing behind
    C.fail_at = 1;
    CHECK(a.ensure(100) == SRT_ERR_HIP && !a && a.capacity() == 0 && take_log() == "fm" && live(OWNED_DEVICE) == 0 && C.device_blocks == 0);
    // upload: frees first, copies the source; an empty source gets one element and no copy
    const std::vector<float> src = {1.0f, 2.0f, 3.0f};
    CHECK(a.upload(src) == SRT_OK && a.capacity() == 3 && C.last_copy_bytes == 12 && take_log() == "mc" && a[2] == 3.0f);
    CHECK(a.upload(src.data(), 2) == SRT_OK && a.capacity() == 2 && take_log() == "fmc");
    CHECK(a.upload(std::vector<float>()) == SRT_OK && a && a.capacity() == 1 && C.last_alloc_bytes == 4 && take_log() == "fm");
    C.fail_at = 1;
    CHECK(a.upload(src) == SRT_ERR_HIP && !a && a.capacity() == 0 && take_log() == "fm" && C.device_blocks == 0);
    // bytes for the arrays a kernel file types
    DeviceBuffer<void> v;
    CHECK(v.ensure(24) == SRT_OK && v.capacity() == 24 && C.last_alloc_bytes == 24 && take_log() == "m");
    // moves: one owner per block
    DeviceBuffer<float> b, c;
    CHECK(b.ensure(4) == SRT_OK && c.ensure(5) == SRT_OK && take_log() == "mm" && live(OWNED_DEVICE) == 3);
    float* const pb = b;
    DeviceBuffer<float> d(std::move(b));                    // construction: no call
    CHECK(!b && b.capacity() == 0 && d == pb && d.capacity() == 4 && take_log().empty());
    c = std::move(d);                                       // onto a full owner: its block goes, once
    CHECK(!d && c == pb && c.capacity() == 4 && take_log() == "f" && live(OWNED_DEVICE) == 2 && C.device_blocks == 2);
    DeviceBuffer<float>& self = c;
    c = std::move(self);                                    // self-move: nothing happens
    CHECK(c == pb && c.capacity() == 4 && take_log().empty());
    c.reset();
    CHECK(!c && take_log() == "f");
    c.reset();
    CHECK(take_log().empty());
  }
  CHECK(take_log() == "f" && all_gone());                   // (v's bytes; everything else went above)
}

static void pinned_buffer() {
  {
    PinnedBuffer<uint32_t> p;
    CHECK(p.ensure(8) == SRT_OK && p && p.capacity() == 8 && p.device() == nullptr && C.last_alloc_bytes == 32 && take_log() == "M" && live(OWNED_PINNED) == 1);
    CHECK(p.ensure(8) == SRT_OK && take_log().empty());
    CHECK(p.ensure(9) == SRT_OK && take_log() == "FM");
    PinnedBuffer<uint32_t> m;
    CHECK(m.ensure(1, hipHostMallocMapped) == SRT_OK && m.device() == m.get() && take_log() == "Mp");
    uint32_t* const pm = m;
    p = std::move(m);
    CHECK(!m && m.device() == nullptr && p == pm && p.device() == pm && take_log() == "F" && live(OWNED_PINNED) == 1);
    PinnedBuffer<uint32_t>& self = p;
    p = std::move(self);
    CHECK(p == pm && take_log().empty());
    C.fail_at = 1;
    CHECK(p.ensure(64) == SRT_ERR_HIP && !p && p.capacity() == 0 && p.device() == nullptr && take_log() == "FM");
  }
  CHECK(take_log().empty() && all_gone());
}

static void events() {
  {
    Event e;
    CHECK(e.create(hipEventDisableTiming) == SRT_OK && (hipEvent_t)e != nullptr && take_log() == "e" && live(OWNED_EVENT) == 1);
    const hipEvent_t raw = e;
    CHECK(e.create() == SRT_OK && (hipEvent_t)e == raw && take_log().empty());   // one that is there stays
    EventPair pair;
    CHECK(pair.first.create() == SRT_OK && pair.second.create() == SRT_OK && take_log() == "ee");
    std::vector<EventPair> pending, spare;                  // the timing brackets' life: pending -> spare -> pending
    pending.push_back(std::move(pair));
    spare.push_back(std::move(pending.back())); pending.pop_back();
    pending.push_back(std::move(spare.back())); spare.pop_back();
    CHECK(take_log().empty() && live(OWNED_EVENT) == 3);
    Event f(std::move(e));
    e = std::move(f);
    Event& self = e;
    e = std::move(self);
    CHECK((hipEvent_t)e == raw && take_log().empty());
    C.fail_at = 1;
    Event g;
    CHECK(g.create() == SRT_ERR_HIP && (hipEvent_t)g == nullptr && take_log() == "e" && live(OWNED_EVENT) == 3);
  }
  CHECK(take_log() == "ddd" && all_gone());
}

static void streams() {
  {
    Stream s;
    CHECK(s.create(hipStreamNonBlocking) == SRT_OK && (hipStream_t)s != nullptr && take_log() == "s" && live(OWNED_STREAM) == 1);
    const hipStream_t raw = s;
    CHECK(s.create(hipStreamNonBlocking) == SRT_OK && (hipStream_t)s == raw && take_log().empty());   // one that is there stays
    Stream t(std::move(s));                                 // construction: no call
    CHECK((hipStream_t)s == nullptr && (hipStream_t)t == raw && take_log().empty());
    s = std::move(t);
    Stream& self = s;
    s = std::move(self);
    CHECK((hipStream_t)s == raw && take_log().empty() && live(OWNED_STREAM) == 1);
    Stream u;
    CHECK(u.create(hipStreamNonBlocking) == SRT_OK && take_log() == "s" && live(OWNED_STREAM) == 2);
    u = std::move(s);                                       // onto a full owner: its stream goes, once
    CHECK((hipStream_t)s == nullptr && (hipStream_t)u == raw && take_log() == "x" && live(OWNED_STREAM) == 1 && C.streams == 1);
    C.fail_at = 1;
    Stream g;
    CHECK(g.create(hipStreamNonBlocking) == SRT_ERR_HIP && (hipStream_t)g == nullptr && take_log() == "s" && live(OWNED_STREAM) == 1);
    u.reset();
    CHECK((hipStream_t)u == nullptr && take_log() == "x");
    u.reset();
    CHECK(take_log().empty());
  }
  CHECK(take_log().empty() && all_gone());
}

// What making one rank's slot of a group lane asks (pt_group.cpp), in its order.
static int fill(LaneSlot* L) {
  int st;
  if ((st = L->stream.create(hipStreamNonBlocking)) || (st = L->event.create(hipEventDisableTiming)) || (st = L->tiles.ensure(64))) return st;
  return SRT_OK;
}

// What making the refit tables of a tree asks of RefitTables, in its order: five tables uploaded, two box arrays allocated.
static int fill(RefitTables* T, bool top) {
  const std::vector<uint32_t> prim(12, 1u), off = {0u, 1u, 3u};
  const std::vector<uint2> leaves(4), list(3), children;    // (an empty table: one element of room)
  int st;
  if ((st = T->d_prim.upload(prim)) || (st = T->d_leaves.upload(leaves)) || (st = T->d_list.upload(list)) || (st = T->d_children.upload(children)) ||
      (st = T->d_level_off.upload(off)) || (!top && (st = T->d_tri_boxes.ensure(12 * 6))) || (st = T->d_node_boxes.ensure(7 * 6)))
    return st;
  T->ntri = 12; T->nnodes = 7;
  return SRT_OK;
}

static int reserve(BvhWorkspace* W, size_t n) {
  int st;
  if ((st = W->d_prim.ensure(n)) || (st = W->d_boxes.ensure(6 * n)) || (st = W->d_nodes.ensure(40 * n)) || (st = W->d_l.ensure(n)) || (st = W->d_r.ensure(n)) ||
      (st = W->d_child.ensure(n)) || (st = W->d_ns.ensure(1)))
    return st;
  W->build_prims = n;
  return SRT_OK;
}

// A struct of owners gives back everything it got when its k-th allocation fails, for every k; and a full one is moved, not copied.
static void structs_of_owners() {
  for (int top = 0; top < 2; top++) {
    int allocations = 0;
    {
      RefitTables T;
      CHECK(fill(&T, top != 0) == SRT_OK);
      for (char c : take_log()) allocations += c == 'm';
      CHECK(allocations == (top ? 6 : 7) && live(OWNED_DEVICE) == (uint64_t)allocations && (top ? !T.d_tri_boxes : (bool)T.d_tri_boxes));
      uint32_t* const prim = T.d_prim;
      RefitTables U(std::move(T));                          // as the context's map and top_tables take them
      CHECK(!T.d_prim && !T.d_node_boxes && U.d_prim == prim && U.ntri == 12 && take_log().empty());
      RefitTables V;
      CHECK(fill(&V, top != 0) == SRT_OK);
      take_log();
      V = std::move(U);                                     // onto a full one: what it held goes, once
      CHECK(V.d_prim == prim && live(OWNED_DEVICE) == (uint64_t)allocations && C.device_blocks == allocations);
      for (char c : take_log()) CHECK(c == 'f');
      V = RefitTables();                                    // how the tables are dropped
      CHECK(!V.d_prim && live(OWNED_DEVICE) == 0 && C.device_blocks == 0);
      take_log();
    }
    CHECK(take_log().empty() && all_gone());
    for (int k = 1; k <= allocations; k++) {
      {
        RefitTables T;
        C.fail_at = k;
        CHECK(fill(&T, top != 0) == SRT_ERR_HIP && C.fail_at == 0);
        CHECK(live(OWNED_DEVICE) == (uint64_t)(k - 1) && C.device_blocks == k - 1);
      }
      CHECK(all_gone());
      take_log();
    }
  }
  {
    LaneSlot L;
    CHECK(fill(&L) == SRT_OK && take_log() == "sem" && live(OWNED_STREAM) == 1 && live(OWNED_EVENT) == 1 && live(OWNED_DEVICE) == 1);
    const hipStream_t raw = L.stream;
    LaneSlot M(std::move(L));                               // as a vector of slots moves them
    CHECK((hipStream_t)L.stream == nullptr && !L.tiles && (hipStream_t)M.stream == raw && M.tiles.capacity() == 64 && take_log().empty());
    M = LaneSlot();                                         // how the group gives a rank's slot back, under that rank's device
    CHECK(take_log() == "xdf" && all_gone());
  }
  CHECK(take_log().empty() && all_gone());
  for (int k = 1; k <= 3; k++) {
    {
      LaneSlot L;
      C.fail_at = k;
      CHECK(fill(&L) == SRT_ERR_HIP && C.fail_at == 0);
      CHECK(live(OWNED_STREAM) + live(OWNED_EVENT) + live(OWNED_DEVICE) == (uint64_t)(k - 1) && C.streams + C.events + C.device_blocks == k - 1);
    }
    CHECK(all_gone());
    take_log();
  }
  for (int k = 1; k <= 7; k++) {
    {
      BvhWorkspace W;
      C.fail_at = k;
      CHECK(reserve(&W, 100) == SRT_ERR_HIP);
      W = BvhWorkspace();                                   // what a failed reservation does
      CHECK(all_gone());
      CHECK(reserve(&W, 100) == SRT_OK && live(OWNED_DEVICE) == 7);
    }
    CHECK(all_gone());
    take_log();
  }
}

int main() {
  empty_owners();
  device_buffer();
  pinned_buffer();
  events();
  streams();
  structs_of_owners();
  CHECK(all_gone() && srt::g_fails > 0);
  std::printf("hip_owned: ok\n");
  return 0;
}
