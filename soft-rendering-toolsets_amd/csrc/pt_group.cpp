// Image-tile sharding of one render over the GPUs of a node inside ONE process: the multi-device form of the path
// tracer's C ABI (include/srt_pt.h, srt_pt_create_multi).
//
// The reference's only parallel axis is the epoch fan-out of Pathtracer::begin_render over a thread pool
// (rays/pathtracer.cpp:250-280); here an epoch is cut into 32 x 32 image tiles dealt round-robin to the devices
// (srt_pt_set_tiling), every device renders its tiles with its own context and stream - the scene is replicated, a few MB -
// and the tile radiance meets on device 0 through ONE RCCL gather per epoch (ncclGather over xGMI, grouped over the
// process's communicators), followed by the un-tiling kernel.  No reduction: the tiles are disjoint.
// RCCL is loaded on first use (dlopen), so single-GPU users never touch it.  Logical ranks that share a device - the way
// the N > 1 path is exercised on a one-GPU box - cannot form an RCCL communicator; their tiles are gathered with
// device-to-device copies instead (also the fallback when librccl is absent; SRT_PT_GATHER=copy|rccl forces one).
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <array>
#include <set>
#include <vector>

#include <hip/hip_runtime.h>

#include "srt_common.h"
#include "srt_pt.h"
#include "pt_internal.h"

namespace {

// the part of <rccl/rccl.h> that is used, bound at run time
typedef struct ncclComm* ncclComm_t;
typedef int ncclResult_t;
constexpr int kNcclFloat = 7;   // ncclFloat32
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Gather)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool load() {
    if (lib) return true;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return false;
    CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
    CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
    GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
    GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
    Gather = (decltype(Gather))dlsym(lib, "ncclGather");
    GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
    return CommInitAll && CommDestroy && GroupStart && GroupEnd && Gather && GetErrorString;
  }
};

}  // namespace

// Every HIP resource below lives in an owner of hip_owned.h, and owners never set the device: whoever calls create / ensure / reset on
// something of rank r has made rank r's device current first (a lane's gather and image, and the timing pairs: rank 0's).

// One rank's slot of a lane: its stream, the event the exchange orders by, and its tiles (tiles_per_rank * floats_per_tile).
struct LaneRank {
  srt::Stream stream; srt::Event event; srt::DeviceBuffer<float> tiles;
  void* handle() const { return (void*)(hipStream_t)stream; }   // the stream as the C ABI passes it
};
// One set of what an epoch in flight needs: a slot per rank, the gathered tiles (n * tile_floats) and the image (w * h * 3) on rank 0.
// Lane 0 always exists; further lanes (srt_pt_group_render_epoch_lane) let epochs overlap.  A lane not created yet has no slots.
struct GroupLane {
  std::vector<LaneRank> ranks;
  srt::DeviceBuffer<float> gather, image;
  size_t tile_floats = 0, image_floats = 0;   // what the buffers were sized for
};
constexpr int kMaxLanes = 4;

// One member: its device, context and communicator, and its part of the accumulator of a render kept on the devices
// (srt_pt_group_fold): its tiles' state, the event behind its last fold and the one behind the last read of it
// (srt_pt_group_accumulator_image, on the display lane).  The events are made by srt_pt_create_multi, the buffer by
// srt_pt_group_set_params: folds and reads only use them.
struct GroupRank {
  int device = 0; srt_pt* ctx = nullptr; ncclComm_t comm = nullptr;
  srt::DeviceBuffer<float> acc;
  srt::Event fold_done, image_done;
  bool fold_recorded = false, image_recorded = false;
};

struct srt_pt_group {
  std::vector<GroupRank> ranks;
  // fixed storage: a lane is created in place, so the render thread creating lane 1 never moves the display lane another thread
  // is using (srt_pt_group_accumulator_image)
  std::array<GroupLane, kMaxLanes> lanes;
  size_t tile_floats = 0, image_floats = 0;   // per rank, and of the image (srt_pt_group_set_params)
  bool use_rccl = false;
  Rccl rccl;
  uint32_t tile_w = 32, tile_h = 32;
  // srt_pt_group_gather_time: event pairs on rank 0's stream around the gather + un-tiling of each epoch
  bool timing = false;
  std::vector<srt::EventPair> timed, spare;
};

namespace {

// What every entry point starts with: a group, and - where the call needs the sizes - one that srt_pt_group_set_params has seen.
int need_group(const srt_pt_group* g, const char* who, bool sized = false) {
  if (!g) return srt::fail(SRT_ERR_INVALID, "%s: NULL group", who);
  if (sized && !g->image_floats) return srt::fail(SRT_ERR_STATE, "%s before srt_pt_group_set_params", who);
  return SRT_OK;
}

// f(context) on every member in rank order; the first status that is not SRT_OK ends it.
template <typename F>
int each_member(srt_pt_group* g, F f) {
  for (GroupRank& R : g->ranks)
    if (const int st = f(R.ctx); st != SRT_OK) return st;
  return SRT_OK;
}

bool lane_exists(const srt_pt_group* g, int lane) { return lane >= 0 && lane < kMaxLanes && !g->lanes[lane].ranks.empty(); }

// A lane's streams and events (once, in place) and its buffers (whenever srt_pt_group_set_params changed the sizes).
int ensure_lane(srt_pt_group* g, int lane) {
  if (lane < 0 || lane >= kMaxLanes) return srt::fail(SRT_ERR_INVALID, "srt_pt_group: lane %d out of range [0, %d)", lane, kMaxLanes);
  const size_t n = g->ranks.size();
  GroupLane& L = g->lanes[lane];
  if (L.ranks.empty()) L.ranks.resize(n);
  int st;
  for (size_t r = 0; r < n; r++) {
    LaneRank& S = L.ranks[r];
    if (S.stream && S.event) continue;
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    if ((st = S.stream.create(hipStreamNonBlocking)) != SRT_OK || (st = S.event.create(hipEventDisableTiming)) != SRT_OK) return st;
  }
  // replaced when the sizes CHANGED, not merely grew: reset() + ensure(), behind the lane's own work
  if (L.tile_floats == g->tile_floats && L.image_floats == g->image_floats && L.image) return SRT_OK;
  for (size_t r = 0; r < n; r++) { SRT_HIP(hipSetDevice(g->ranks[r].device)); SRT_HIP(hipStreamSynchronize(L.ranks[r].stream)); }
  L.tile_floats = L.image_floats = 0;
  const size_t tf = g->tile_floats ? g->tile_floats : 1, imf = g->image_floats ? g->image_floats : 1;   // (a size of 0: one element)
  for (size_t r = 0; r < n; r++) {
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    L.ranks[r].tiles.reset();
    if ((st = L.ranks[r].tiles.ensure(tf)) != SRT_OK) return st;
  }
  SRT_HIP(hipSetDevice(g->ranks[0].device));
  L.gather.reset(); L.image.reset();
  if ((st = L.gather.ensure(tf * n)) != SRT_OK || (st = L.image.ensure(imf)) != SRT_OK) return st;
  L.tile_floats = g->tile_floats; L.image_floats = g->image_floats;
  return SRT_OK;
}

// The exchange step of one epoch on one lane (everything behind the members' launches).
int exchange(srt_pt_group* g, GroupLane& L) {
  const size_t n = g->ranks.size();
  const int device0 = g->ranks[0].device;
  LaneRank& S0 = L.ranks[0];
  const float* gathered = S0.tiles;
  if (g->use_rccl) {                     // ONE collective per epoch: tile radiance -> rank 0
    // (no early return between GroupStart and GroupEnd: a failing rank ends the loop, the group is always closed)
    ncclResult_t rc = g->rccl.GroupStart();
    hipError_t he = hipSuccess;
    for (size_t r = 0; r < n && rc == 0 && he == hipSuccess; r++) {
      he = hipSetDevice(g->ranks[r].device);
      if (he == hipSuccess) rc = g->rccl.Gather(L.ranks[r].tiles, r == 0 ? L.gather.get() : nullptr, g->tile_floats, kNcclFloat, 0, g->ranks[r].comm, L.ranks[r].stream);
    }
    const ncclResult_t rc2 = g->rccl.GroupEnd();
    if (he != hipSuccess) return srt::fail(SRT_ERR_HIP, "hipSetDevice inside the gather group failed: %s", hipGetErrorString(he));
    if (rc != 0 || rc2 != 0) return srt::fail(SRT_ERR_HIP, "ncclGather failed: %s", g->rccl.GetErrorString(rc != 0 ? rc : rc2));
    gathered = L.gather;
  } else if (n > 1) {                    // ranks that share a device (or no RCCL): device-to-device copies behind events
    for (size_t r = 0; r < n; r++) {
      SRT_HIP(hipSetDevice(g->ranks[r].device));
      SRT_HIP(hipEventRecord(L.ranks[r].event, L.ranks[r].stream));
    }
    SRT_HIP(hipSetDevice(device0));
    for (size_t r = 0; r < n; r++) {
      SRT_HIP(hipStreamWaitEvent(S0.stream, L.ranks[r].event, 0));
      if (g->ranks[r].device == device0)
        SRT_HIP(hipMemcpyAsync(L.gather + r * g->tile_floats, L.ranks[r].tiles, g->tile_floats * sizeof(float), hipMemcpyDeviceToDevice, S0.stream));
      else
        SRT_HIP(hipMemcpyPeerAsync(L.gather + r * g->tile_floats, device0, L.ranks[r].tiles, g->ranks[r].device, g->tile_floats * sizeof(float), S0.stream));
    }
    gathered = L.gather;
  }
  SRT_HIP(hipSetDevice(device0));
  return srt_pt_untile_device(g->ranks[0].ctx, S0.handle(), gathered, L.image);
}

// Behind an exchange by copies: rank 0 records its lane event, ranks 1..n-1 wait for it - the next work on this lane must not
// overwrite a rank's tiles before rank 0 has copied them - and device 0 is current again.
int hold_ranks_behind_copies(srt_pt_group* g, GroupLane& L) {
  if (g->ranks.size() < 2 || g->use_rccl) return SRT_OK;
  SRT_HIP(hipEventRecord(L.ranks[0].event, L.ranks[0].stream));
  for (size_t r = 1; r < g->ranks.size(); r++) { SRT_HIP(hipSetDevice(g->ranks[r].device)); SRT_HIP(hipStreamWaitEvent(L.ranks[r].stream, L.ranks[0].event, 0)); }
  SRT_HIP(hipSetDevice(g->ranks[0].device));
  return SRT_OK;
}

constexpr int kDisplayLane = kMaxLanes - 1;   // srt_pt_group_accumulator_image's own streams and exchange buffers

// Every rank's accumulator state, sized for the current image / tiling; replaced and zeroed when the size changed - by
// srt_pt_group_set_params, so that a fold and a read of the accumulator from two threads find it in place.
int ensure_accumulators(srt_pt_group* g) {
  for (GroupRank& R : g->ranks) {
    size_t need = 0;
    int st = srt_pt_accumulator_floats(R.ctx, &need);
    if (st != SRT_OK) return st;
    if (R.acc && R.acc.capacity() == need) continue;
    SRT_HIP(hipSetDevice(R.device));
    SRT_HIP(hipDeviceSynchronize());
    R.acc.reset();
    if ((st = R.acc.ensure(need)) != SRT_OK) return st;
    SRT_HIP(hipMemset(R.acc, 0, need * sizeof(float)));
    SRT_HIP(hipDeviceSynchronize());                     // (null-stream memset: done before a lane's non-blocking stream folds into it)
    R.fold_recorded = R.image_recorded = false;
  }
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_pt_create_multi(const int* devices, int n, srt_pt_group** out) {
  if (!out) return srt::fail(SRT_ERR_INVALID, "srt_pt_create_multi: out is NULL");
  *out = nullptr;
  if (!devices || n < 1 || n > 64) return srt::fail(SRT_ERR_INVALID, "srt_pt_create_multi: need 1..64 devices (got %d)", n);
  srt_pt_group* g = new (std::nothrow) srt_pt_group();
  if (!g) return srt::fail(SRT_ERR_INVALID, "out of host memory");
  g->ranks.resize(n);
  for (int r = 0; r < n; r++) g->ranks[r].device = devices[r];
  int st = SRT_OK;
  for (int r = 0; r < n && st == SRT_OK; r++) {
    GroupRank& R = g->ranks[r];
    st = srt_pt_create(R.device, &R.ctx);
    if (st == SRT_OK) st = srt_pt_set_tiling(R.ctx, g->tile_w, g->tile_h, (uint32_t)r, (uint32_t)n);
    if (st == SRT_OK && hipSetDevice(R.device) != hipSuccess) st = srt::fail(SRT_ERR_HIP, "srt_pt_create_multi: hipSetDevice(%d) failed", R.device);
    if (st == SRT_OK) st = R.fold_done.create(hipEventDisableTiming);
    if (st == SRT_OK) st = R.image_done.create(hipEventDisableTiming);
  }
  if (st == SRT_OK) {
    // one RCCL communicator per rank when every rank has a device of its own; shared devices gather by copies
    const std::set<int> distinct(devices, devices + n);
    const char* mode = getenv("SRT_PT_GATHER");
    const bool want_rccl = mode ? std::strcmp(mode, "rccl") == 0 : (n > 1 && (int)distinct.size() == n);
    if (want_rccl && (int)distinct.size() == n) {
      if (g->rccl.load()) {
        std::vector<ncclComm_t> comms(n, nullptr);
        const ncclResult_t rc = g->rccl.CommInitAll(comms.data(), n, devices);
        if (rc != 0) st = srt::fail(SRT_ERR_HIP, "ncclCommInitAll over %d devices failed: %s", n, g->rccl.GetErrorString(rc));
        else {
          for (int r = 0; r < n; r++) g->ranks[r].comm = comms[r];
          g->use_rccl = true;
        }
      } else if (mode) {
        st = srt::fail(SRT_ERR_UNSUPPORTED, "SRT_PT_GATHER=rccl but librccl could not be loaded: %s", dlerror());
      }
    }
  }
  if (st != SRT_OK) { srt_pt_group_destroy(g); return st; }
  *out = g;
  return SRT_OK;
}

// An explicit routine, not a cascade of destructors: the owners do not set the device, and the group's live on several.  Takes a
// partly built group away too (srt_pt_create_multi on failure).
int srt_pt_group_destroy(srt_pt_group* g) {
  if (!g) return SRT_OK;
  // 1. every lane stream that exists has run dry
  for (GroupLane& L : g->lanes)
    for (size_t r = 0; r < L.ranks.size(); r++)
      if (L.ranks[r].stream) { (void)hipSetDevice(g->ranks[r].device); (void)hipStreamSynchronize(L.ranks[r].stream); }
  // 2. the RCCL communicators
  if (g->use_rccl)
    for (GroupRank& R : g->ranks)
      if (R.comm) (void)g->rccl.CommDestroy(R.comm);
  // 3. per rank, under its device: its lane slots, accumulator and events (a rank without a context never got any), and under
  //    rank 0's what rank 0 holds for all
  for (size_t r = 0; r < g->ranks.size(); r++) {
    GroupRank& R = g->ranks[r];
    if (!R.ctx) continue;
    (void)hipSetDevice(R.device);
    for (GroupLane& L : g->lanes)
      if (r < L.ranks.size()) L.ranks[r] = LaneRank();
    R.acc.reset(); R.fold_done.reset(); R.image_done.reset();
    if (r == 0) {
      for (GroupLane& L : g->lanes) { L.gather.reset(); L.image.reset(); }
      g->timed.clear(); g->spare.clear();
    }
  }
  // 4. the member contexts
  for (GroupRank& R : g->ranks)
    if (R.ctx) { (void)hipSetDevice(R.device); (void)srt_pt_destroy(R.ctx); }
  // 5. nothing is left for a destructor to free under the wrong device
  delete g;
  return SRT_OK;
}

int srt_pt_group_size(srt_pt_group* g) { return g ? (int)g->ranks.size() : 0; }

srt_pt* srt_pt_group_context(srt_pt_group* g, int rank) {
  if (!g || rank < 0 || rank >= (int)g->ranks.size()) { srt::fail(SRT_ERR_INVALID, "srt_pt_group_context: rank %d out of range", rank); return nullptr; }
  return g->ranks[rank].ctx;
}

int srt_pt_group_uses_rccl(srt_pt_group* g) { return g && g->use_rccl ? 1 : 0; }

int srt_pt_group_set_params(srt_pt_group* g, uint32_t width, uint32_t height, uint32_t max_depth) {
  int st = need_group(g, "srt_pt_group_set_params");
  if (st == SRT_OK) st = each_member(g, [&](srt_pt* c) { return srt_pt_set_params(c, width, height, max_depth); });
  uint32_t local = 0, per_rank = 0, fpt = 0;
  if (st != SRT_OK || (st = srt_pt_tile_info(g->ranks[0].ctx, &local, &per_rank, &fpt)) != SRT_OK) return st;
  g->tile_floats = (size_t)per_rank * fpt;
  g->image_floats = (size_t)width * height * 3;
  // lanes 0 and 1 (the render thread's) and the display lane sized now, and the accumulators: later calls - a fold on the render
  // thread, srt_pt_group_accumulator_image on another - only use them
  for (int lane : {0, 1, kDisplayLane})
    if ((st = ensure_lane(g, lane)) != SRT_OK) return st;
  return ensure_accumulators(g);
}

int srt_pt_group_render_epoch_lane(srt_pt_group* g, int lane, uint64_t seed, uint32_t sample_base, uint32_t samples, float** d_image_out, void** stream_out) {
  int st = need_group(g, "srt_pt_group_render_epoch", true);
  if (st != SRT_OK || (st = ensure_lane(g, lane)) != SRT_OK) return st;
  GroupLane& L = g->lanes[lane];
  const size_t n = g->ranks.size();
  for (size_t r = 0; r < n; r++) {       // every rank renders its tiles; the launches only enqueue
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    if ((st = srt_pt_render_epoch_device(g->ranks[r].ctx, L.ranks[r].handle(), seed, sample_base, samples, L.ranks[r].tiles)) != SRT_OK) return st;   // (SRT_CANCELLED included)
  }
  // (the bracket opens once rank 0's own tiles are rendered: what follows is exchange + un-tiling.  A pair is only kept once BOTH
  //  of its events are recorded: whatever fails in between puts it back)
  srt::EventPair ev;
  if (g->timing) {
    SRT_HIP(hipSetDevice(g->ranks[0].device));
    if (!g->spare.empty()) { ev = std::move(g->spare.back()); g->spare.pop_back(); }
    else if ((st = ev.first.create()) != SRT_OK || (st = ev.second.create()) != SRT_OK) return st;
    if (hipEventRecord(ev.first, L.ranks[0].stream) != hipSuccess) { g->spare.push_back(std::move(ev)); return srt::fail(SRT_ERR_HIP, "srt_pt_group: hipEventRecord failed"); }
  }
  st = exchange(g, L);
  if (g->timing) (st == SRT_OK && hipEventRecord(ev.second, L.ranks[0].stream) == hipSuccess ? g->timed : g->spare).push_back(std::move(ev));
  if (st != SRT_OK || (st = hold_ranks_behind_copies(g, L)) != SRT_OK) return st;
  if (d_image_out) *d_image_out = L.image;
  if (stream_out) *stream_out = L.ranks[0].handle();
  return SRT_OK;
}

int srt_pt_group_render_epoch_device(srt_pt_group* g, uint64_t seed, uint32_t sample_base, uint32_t samples, float** d_image_out, void** stream_out) {
  return srt_pt_group_render_epoch_lane(g, 0, seed, sample_base, samples, d_image_out, stream_out);
}

int srt_pt_group_gather_time(srt_pt_group* g, int enable, double* total_ms, uint64_t* epochs) {
  int st = need_group(g, "srt_pt_group_gather_time");
  if (st != SRT_OK) return st;
  SRT_HIP(hipSetDevice(g->ranks[0].device));
  double sum = 0.0;
  uint64_t n = 0;
  for (srt::EventPair& ev : g->timed) {  // (every pair goes back to `spare`, also when one of them cannot be read)
    float ms = 0.f;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { sum += ms; n++; }
    else { (void)hipGetLastError(); st = srt::fail(SRT_ERR_HIP, "srt_pt_group_gather_time: an event pair could not be read"); }
    g->spare.push_back(std::move(ev));
  }
  g->timed.clear();
  g->timing = enable != 0;
  if (total_ms) *total_ms = sum;
  if (epochs) *epochs = n;
  return st;
}

int srt_pt_group_render_epoch(srt_pt_group* g, uint64_t seed, uint32_t sample_base, uint32_t samples, float* rgb_out) {
  if (!rgb_out) return srt::fail(SRT_ERR_INVALID, "srt_pt_group_render_epoch: output is NULL");
  float* d_image = nullptr; void* s = nullptr;
  int st = srt_pt_group_render_epoch_device(g, seed, sample_base, samples, &d_image, &s);
  if (st != SRT_OK) return st;
  SRT_HIP(hipMemcpyAsync(rgb_out, d_image, g->image_floats * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)s));
  SRT_HIP(hipStreamSynchronize((hipStream_t)s));
  // the image is host-visible now: a member whose streamed launch ended with unfinished units, or a cancel, invalidates it
  return each_member(g, [](srt_pt* c) { return srt_pt_cancel_requested(c) ? (int)SRT_CANCELLED : srt::pt_check_fault(c, "srt_pt_group_render_epoch"); });
}

// ---- a render with the accumulator on the devices ----------------------------------------------------------------------
int srt_pt_group_reset_accumulator(srt_pt_group* g) {
  int st = need_group(g, "srt_pt_group_reset_accumulator", true);
  if (st != SRT_OK || (st = ensure_accumulators(g)) != SRT_OK) return st;
  for (GroupRank& R : g->ranks) {
    SRT_HIP(hipSetDevice(R.device));
    SRT_HIP(hipDeviceSynchronize());                     // (between renders: nothing is in flight that matters)
    SRT_HIP(hipMemset(R.acc, 0, R.acc.capacity() * sizeof(float)));
    SRT_HIP(hipDeviceSynchronize());
    R.fold_recorded = R.image_recorded = false;
  }
  return SRT_OK;
}

int srt_pt_group_max_samples_per_launch(srt_pt_group* g, uint32_t* samples) {
  if (!g || !samples) return srt::fail(SRT_ERR_INVALID, "srt_pt_group_max_samples_per_launch: NULL argument");
  uint32_t least = 0xFFFFFFFFu;
  for (GroupRank& R : g->ranks) {
    uint32_t m = 0;
    const int st = srt_pt_max_samples_per_launch(R.ctx, &m);
    if (st != SRT_OK) return st;
    least = std::min(least, m);
  }
  *samples = least;
  return SRT_OK;
}

int srt_pt_group_render_samples(srt_pt_group* g, int lane, uint64_t seed, uint32_t sample_base, uint32_t samples) {
  int st = need_group(g, "srt_pt_group_render_samples", true);
  if (st != SRT_OK) return st;
  if (lane == kDisplayLane) return srt::fail(SRT_ERR_INVALID, "srt_pt_group_render_samples: lane %d belongs to srt_pt_group_accumulator_image", lane);
  if ((st = ensure_lane(g, lane)) != SRT_OK) return st;
  GroupLane& L = g->lanes[lane];
  for (size_t r = 0; r < g->ranks.size(); r++) {
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    if ((st = srt_pt_render_samples_device(g->ranks[r].ctx, L.ranks[r].handle(), seed, sample_base, samples)) != SRT_OK) return st;
  }
  return SRT_OK;
}

int srt_pt_group_wait_lane(srt_pt_group* g, int lane) {
  int st = need_group(g, "srt_pt_group_wait_lane");
  if (st != SRT_OK || !lane_exists(g, lane)) return st;
  GroupLane& L = g->lanes[lane];
  for (size_t r = 0; r < g->ranks.size(); r++) {
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    SRT_HIP(hipStreamSynchronize(L.ranks[r].stream));
    if ((st = srt::pt_check_fault(g->ranks[r].ctx, "srt_pt_group_wait_lane")) != SRT_OK) return st;
  }
  return SRT_OK;
}

int srt_pt_group_fold(srt_pt_group* g, int lane, uint32_t samples_per_epoch, uint32_t position, uint32_t total_samples, uint32_t accumulator_samples) {
  int st = need_group(g, "srt_pt_group_fold");
  if (st != SRT_OK) return st;
  if (!lane_exists(g, lane) || lane == kDisplayLane) return srt::fail(SRT_ERR_INVALID, "srt_pt_group_fold: nothing was rendered on lane %d", lane);
  if ((st = ensure_accumulators(g)) != SRT_OK) return st;
  GroupLane& L = g->lanes[lane];
  for (size_t r = 0; r < g->ranks.size(); r++) {
    GroupRank& R = g->ranks[r];
    LaneRank& S = L.ranks[r];
    SRT_HIP(hipSetDevice(R.device));
    // in launch order behind the previous fold (another lane's stream) and behind whoever is reading the accumulator
    if (R.fold_recorded) SRT_HIP(hipStreamWaitEvent(S.stream, R.fold_done, 0));
    if (R.image_recorded) SRT_HIP(hipStreamWaitEvent(S.stream, R.image_done, 0));
    if ((st = srt_pt_fold_epochs_device(R.ctx, S.handle(), samples_per_epoch, position, total_samples, accumulator_samples, R.acc)) != SRT_OK) return st;
    SRT_HIP(hipEventRecord(R.fold_done, S.stream));
    R.fold_recorded = true;
  }
  return SRT_OK;
}

int srt_pt_group_accumulator_image(srt_pt_group* g, float** d_image_out, void** stream_out) {
  int st = need_group(g, "srt_pt_group_accumulator_image", true);
  if (st != SRT_OK || (st = ensure_lane(g, kDisplayLane)) != SRT_OK || (st = ensure_accumulators(g)) != SRT_OK) return st;
  GroupLane& L = g->lanes[kDisplayLane];
  for (size_t r = 0; r < g->ranks.size(); r++) {
    GroupRank& R = g->ranks[r];
    LaneRank& S = L.ranks[r];
    SRT_HIP(hipSetDevice(R.device));
    if (R.fold_recorded) SRT_HIP(hipStreamWaitEvent(S.stream, R.fold_done, 0));
    if ((st = srt_pt_accumulator_tiles_device(R.ctx, S.handle(), R.acc, S.tiles)) != SRT_OK) return st;
    SRT_HIP(hipEventRecord(R.image_done, S.stream));
    R.image_recorded = true;
  }
  if ((st = exchange(g, L)) != SRT_OK || (st = hold_ranks_behind_copies(g, L)) != SRT_OK) return st;
  if (d_image_out) *d_image_out = L.image;
  if (stream_out) *stream_out = L.ranks[0].handle();
  return SRT_OK;
}

int srt_pt_group_cancel_requested(srt_pt_group* g) {
  if (!g) return 0;
  for (GroupRank& R : g->ranks)
    if (srt_pt_cancel_requested(R.ctx)) return 1;
  return 0;
}

int srt_pt_group_cancel(srt_pt_group* g) {
  const int st = need_group(g, "srt_pt_group_cancel");
  if (st != SRT_OK) return st;
  for (GroupRank& R : g->ranks) (void)srt_pt_cancel(R.ctx);
  return SRT_OK;
}

int srt_pt_group_clear_cancel(srt_pt_group* g) {
  const int st = need_group(g, "srt_pt_group_clear_cancel");
  return st != SRT_OK ? st : each_member(g, [](srt_pt* c) { return srt_pt_clear_cancel(c); });
}

int srt_pt_group_set_env_sampling(srt_pt_group* g, uint32_t mode) {
  const int st = need_group(g, "srt_pt_group_set_env_sampling");
  return st != SRT_OK ? st : each_member(g, [&](srt_pt* c) { return srt_pt_set_env_sampling(c, mode); });
}

int srt_pt_group_set_normal_colors(srt_pt_group* g, int on) {
  const int st = need_group(g, "srt_pt_group_set_normal_colors");
  return st != SRT_OK ? st : each_member(g, [&](srt_pt* c) { return srt_pt_set_normal_colors(c, on); });
}

int srt_pt_group_set_dynamic_lights(srt_pt_group* g, int on) {
  const int st = need_group(g, "srt_pt_group_set_dynamic_lights");
  return st != SRT_OK ? st : each_member(g, [&](srt_pt* c) { return srt_pt_set_dynamic_lights(c, on); });
}

int srt_pt_group_set_active(srt_pt_group* g, const uint32_t* objects, const uint8_t* active, uint32_t n) {
  const int st = need_group(g, "srt_pt_group_set_active");
  return st != SRT_OK ? st : each_member(g, [&](srt_pt* c) { return srt_pt_set_active(c, objects, active, n); });
}

int srt_pt_group_set_active_device(srt_pt_group* g, void* stream, const uint32_t* objects, const uint8_t* const* d_active, uint32_t n) {
  if (!g || (n && !d_active)) return srt::fail(SRT_ERR_INVALID, "srt_pt_group_set_active_device: NULL argument");
  for (size_t r = 0; r < g->ranks.size(); r++) {
    const int st = srt_pt_set_active_device(g->ranks[r].ctx, stream, objects, n ? d_active[r] : nullptr, n);
    if (st != SRT_OK) return st;
  }
  // (the lanes' streams are not ordered behind `stream`: every member settles before the group renders again)
  return each_member(g, [](srt_pt* c) { return srt_pt_sync(c); });
}

int srt_pt_group_set_ray_log(srt_pt_group* g, uint32_t capacity) {
  const int st = need_group(g, "srt_pt_group_set_ray_log");
  return st != SRT_OK ? st : each_member(g, [&](srt_pt* c) { return srt_pt_set_ray_log(c, capacity); });
}

int srt_pt_group_read_ray_log(srt_pt_group* g, int lane, srt_pt_logged_ray* out, size_t cap, size_t* n_out, uint64_t* dropped) {
  int st = need_group(g, "srt_pt_group_read_ray_log");
  if (st != SRT_OK) return st;
  if (n_out) *n_out = 0;
  if (dropped) *dropped = 0;
  if (!lane_exists(g, lane)) return SRT_OK;                            // a lane that never rendered has logged nothing
  GroupLane& L = g->lanes[lane];
  std::vector<srt_pt_logged_ray> all;
  size_t total_waiting = 0;
  for (size_t r = 0; r < g->ranks.size(); r++) {
    srt_pt* const c = g->ranks[r].ctx;
    void* const s = L.ranks[r].handle();
    SRT_HIP(hipSetDevice(g->ranks[r].device));
    size_t waiting = 0;
    if ((st = srt_pt_read_ray_log_stream(c, s, nullptr, 0, &waiting, nullptr)) != SRT_OK) return st;   // how many (nothing consumed)
    total_waiting += waiting;
    if (!waiting || !out) continue;
    const size_t at = all.size();
    all.resize(at + waiting);
    size_t got = 0;
    uint64_t d = 0;
    if ((st = srt_pt_read_ray_log_stream(c, s, all.data() + at, waiting, &got, &d)) != SRT_OK) return st;
    all.resize(at + got);
    if (dropped) *dropped += d;
  }
  if (!out) { if (n_out) *n_out = total_waiting; return SRT_OK; }
  std::sort(all.begin(), all.end(), [](const srt_pt_logged_ray& a, const srt_pt_logged_ray& b) {
    if (a.pixel != b.pixel) return a.pixel < b.pixel;
    if (a.sample != b.sample) return a.sample < b.sample;
    return a.bounce < b.bounce;
  });
  const size_t n = std::min(all.size(), cap);
  if (n) std::memcpy(out, all.data(), n * sizeof(srt_pt_logged_ray));
  if (dropped) *dropped += all.size() - n;
  if (n_out) *n_out = n;
  return SRT_OK;
}

}  // extern "C"
