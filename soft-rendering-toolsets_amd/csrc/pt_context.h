// The path tracer's context (struct srt_pt) and the helpers the translation units behind include/srt_pt.h share:
//   pt.hip          the render kernels, the choice of kernel form, the render paths and what reads back what a render leaves
//   pt_context.cpp  host code only: create / destroy, scene begin / add / commit, camera, image size, tiling and the switches
//   pt_update*.cpp  host code only: what changes or queries a committed scene - pt_update_mesh.cpp (new vertices), pt_update_skin.cpp
//                   (skins and rigs), pt_update_pose.cpp (poses, object timelines), pt_update_shading.cpp (materials, delta lights,
//                   shading timelines), pt_update_emitter.cpp (particle emitters) and pt_update.cpp (what they share - pt_update.h -
//                   and settle())
//   pt_query.hip    per-lane kernels on the committed scene outside a render (samples, hits, particles) and the dumps
//   pt_hit_device.hip  srt_pt_hit_device: rays from device memory through pt.hip's ray-cast kernel (pack, resolve) or the per-lane walk
//   pt_image.hip    untile, accumulate, tonemap
//   pt_probe.hip    the test-only math probes of srt_pt_debug.h
// Only pt.hip may include pt_wave.h / pt_stream.h: they define non-template __global__ functions, which a second includer would
// define again.  So neither may be included here, nor any other header that defines a kernel.
#ifndef SRT_PT_CONTEXT_H
#define SRT_PT_CONTEXT_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "pt_bvh_device.h"
#include "pt_pose.h"
#include "pt_scene.h"
#include "srt_common.h"
#include "srt_pt.h"

namespace srt {
struct StreamCounters;   // pt_stream.h
struct DScene;           // pt_trace.h
constexpr uint32_t kMaxStreamSlots = 1u << 26;   // srt_pt_set_stream_slots: upper bound of the path-slot population (state planes: ~13 GB there)
}

struct srt_pt {
  int device = -1;            // -1: host-only context (scene assembly / BVH inspection, no rendering)
  srt::Stream stream;
  std::vector<srt::ObjectInput> inputs;
  std::vector<srt::Material> materials;
  srt::BuiltScene built;
  bool committed = false;
  srt::Camera cam{};
  bool have_cam = false;
  uint32_t w = 0, h = 0, max_depth = 8;
  srt::TileMap tiles{32, 32, 0, 0, 0, 1, 0};
  uint32_t tiles_per_rank = 0;
  // device copies
  srt::DeviceBuffer<srt::Node> d_nodes; srt::DeviceBuffer<srt::Tri> d_tris; srt::DeviceBuffer<srt::TriNrm> d_nrm; srt::DeviceBuffer<srt::Object> d_objects;
  srt::DeviceBuffer<float> d_tri_packed;                         // the triangle records without padding (pt_scene.h): what the cast kernel reads
  srt::DeviceBuffer<srt::Light> d_lights; srt::DeviceBuffer<srt::LightTri> d_ltris; srt::DeviceBuffer<srt::Material> d_mats;
  srt::DeviceBuffer<srt::WaveInterior> d_wave, d_blas; srt::DeviceBuffer<uint32_t> d_wave_lazy;
  srt::DeviceBuffer<srt::DeltaLight> d_dlights;
  std::vector<srt::DeltaLight> delta_lights;   // srt_pt_add_light, in call order
  uint32_t env_type = 0; float env_radiance[3] = {0, 0, 0};   // srt_pt_set_env_light
  std::vector<float> env_map; uint32_t env_w = 0, env_h = 0; srt::DeviceBuffer<float> d_env_map;   // srt_pt_set_env_map
  // srt_pt_set_env_sampling: the mode (read whenever a launch is enqueued) and, from the first launch that needs them until the map
  // goes (srt_pt_scene_begin, srt_pt_set_env_map), the tables of Samplers::Sphere::Image for env_map (pt_env_image.h) and their
  // device copies - d_tables: _cdf then _pdf, d_trig: the doubles of sample().  Nothing here is made while the mode is off.
  uint32_t env_sampling = 0;
  struct EnvImage {
    bool valid = false;
    float total = 0.0f;
    std::vector<float> cdf_pdf; std::vector<double> trig;
    srt::DeviceBuffer<float> d_tables; srt::DeviceBuffer<double> d_trig;
    void drop() { valid = false; total = 0.0f; cdf_pdf.clear(); trig.clear(); d_tables.reset(); d_trig.reset(); }
  } env_image;
  srt::DeviceBuffer<float> d_tile_buf;
  int kernel_mode = 0;        // srt_pt_set_kernel: 0 auto, 1 per-lane (lane per pixel), 2 wave-uniform, 3 wave-uniform with section stamps, 4 per-lane (lane per
                              // sample), 5 flattened per-lane walk, 6 streamed (logic + ray-cast kernels), 7 streamed sweeps; wave_trav() picks the form
  // Scratch of one epoch in flight.  One set per stream the caller renders on: epochs launched on different streams
  // may overlap on the device (the next epoch's blocks fill the CUs the previous launch's tail leaves idle).
  struct EpochBuffers {
    srt::DeviceBuffer<float> d_samples;                      // per-sample radiance
    // persistent wave forms: the camera table of the launch in flight (pt_wave.h: pt_camera_kernel), rebuilt in front of every launch.
    // Per sample of a launch 20 B - RNG state (2 dwords), then, in a second plane, the direction (3) -, then the shared origin:
    // 1.34 GB per stream at 1024 x 1024 pixels and 64 samples per launch, next to d_samples' 1.07 GB.
    srt::DeviceBuffer<uint32_t> d_camera;
    srt::DeviceBuffer<float> d_records;                      // wave kernel: per-bounce records
    srt::DeviceBuffer<float> d_running;                      // (sum, count) across the launches of one epoch
    srt::DeviceBuffer<unsigned long long> d_queue;           // wave kernel: queue head (+ section stamps)
    // streamed form (pt_stream.h): saved path state, ray queue (origins, then directions: one array), hits, counters
    srt::DeviceBuffer<uint32_t> d_state;
    srt::DeviceBuffer<float4> d_ray_o;
    srt::DeviceBuffer<uint32_t> d_ray_id;
    srt::DeviceBuffer<uint2> d_hits;
    srt::DeviceBuffer<srt::StreamCounters> d_sc;
    srt::DeviceBuffer<unsigned long long> d_block_counters;
    srt::DeviceBuffer<uint32_t> d_cast_spill;                // the ray-cast kernel's traversal frames beyond those in LDS
    srt::DeviceBuffer<uint32_t> d_cancel;                    // srt_pt_cancel as the kernels of this stream have seen it (sticky until srt_pt_clear_cancel)
    srt::DeviceBuffer<uint32_t> d_ray_log; uint32_t ray_log_cap = 0;   // srt_pt_set_ray_log: this stream's ring (pt_trace.h: log_ray_event) and the rays it holds
    srt::DeviceBuffer<uint32_t> d_alive_list;                // streamed forms: the alive slots the next generation works from
    uint32_t last_samples = 0, last_npix = 0;                         // what d_samples holds: samples per pixel and pixel slots of the last launch
  };
  std::map<hipStream_t, EpochBuffers> epoch_buffers;
  // Scratch of srt_pt_hit_device's cast path, one set per stream the caller queries on (44 B per ray of a chunk + the spill columns):
  // the chunk's requests as the cast kernel reads them, the identity list, the hit words; and what the launch keeps to itself - a
  // StreamCounters block, a cancel word that stays zero (a query ignores srt_pt_cancel) and the frames beyond those in LDS.
  struct QueryBuffers {
    srt::DeviceBuffer<float4> d_req;                         // {origin, b0} {dir, b1} per ray
    srt::DeviceBuffer<uint32_t> d_ray_id;
    srt::DeviceBuffer<uint2> d_hits;
    srt::DeviceBuffer<srt::StreamCounters> d_sc;
    srt::DeviceBuffer<uint32_t> d_zero;
    srt::DeviceBuffer<uint32_t> d_spill;
  };
  std::map<hipStream_t, QueryBuffers> query_buffers;
  uint64_t hit_device_paths[3] = {0, 0, 0};                  // srt_pt_hit_device_paths: calls through {the cast kernel, the nested walk, the flattened walk}
  int wave_blocks = 0; size_t wave_lds = 0; int wave_mode = -1; const void* wave_kern = nullptr;
  int wave_cus = 0;           // CUs of the device, read with wave_blocks (the camera pre-pass's launch shape)
  // pt_cast_kernel's launch shape (blocks == 0: not derived yet).  The render's and the queries' are cached apart: on a scene of the
  // streamed sweeps the render launches the walk-only build and a query the general one.
  struct CastShape {
    const void* kern = nullptr; uint32_t lds_frames = 0;     // traversal frames per lane kept in LDS (the deeper ones: the spill columns)
    int blocks = 0, threads = 0; size_t lds = 0; uint32_t depth = 0;
  } cast, query_cast;
  void drop_cast_shapes() { cast.blocks = 0; query_cast.blocks = 0; }   // the ray-cast kernel's stack depth follows the scene
  int bvh_builder = 1; uint32_t bvh_device_min = 16384;         // srt_pt_set_bvh_builder: device build for sets of >= this many primitives
  uint32_t stream_slots = 0;                                    // srt_pt_set_stream_slots (0: default)
  srt::DeviceBuffer<unsigned long long> d_cast_stats;           // SRT_CAST_STATS=1: the STATS build of pt_cast_kernel adds into these
  srt::DeviceBuffer<unsigned long long> d_totals;   // C_COUNT instrumented totals + 4 slots: rays of the epoch kernels, rays elided, streamed forms: entries queued, alive slot-generations
  srt::PinnedBuffer<uint32_t> h_fault;      // mapped: bit 0 = a streamed launch ended with unfinished units (sticky until reported); the kernels' address: device()
  srt::PinnedBuffer<uint32_t> h_cancel;     // mapped: srt_pt_cancel's flag (any host thread may set it)
  uint32_t ray_log_cap = 0;                 // srt_pt_set_ray_log: rays per stream and read; 0: Pathtracer::log_ray is not delivered
  int elide = 0;                            // srt_pt_set_elision
  int normal_colors = 0;                    // srt_pt_set_normal_colors: read whenever a launch is enqueued
  unsigned long long last_counters[srt::C_COUNT] = {0};
  uint64_t camera_samples = 0;
  // srt_pt_kernel_time: event pairs recorded around the dominant kernel's launches, on the launch stream
  bool timing = false;
  std::vector<srt::EventPair> timed;   // pending (recorded, not yet read)
  std::vector<srt::EventPair> spare;
  // srt_pt_stream_times: per-kernel event pairs of the streamed form {logic, compaction, ray cast}
  bool stream_timing = false;
  std::vector<srt::EventPair> stream_timed[4];   // {logic (resolve), compaction, ray cast, probe}
  uint64_t stream_generations = 0;
  // srt_pt_scene_counts: since creation
  uint64_t blas_builds = 0, bytes_uploaded = 0, tri_bytes_uploaded = 0;
  // srt_pt_update_mesh: the index buffers of the meshes that can be updated (no instance, no area light), resident from commit on, one
  // after the other; the device builder's workspace (srt_pt_repose_device builds the BVH<Object> in it too); and the staging of the
  // host form's vertex arrays.  Grown on demand, kept.
  struct MeshState {
    srt::DeviceBuffer<uint32_t> d_idx; size_t idx_words = 0;   // idx_words: the words in use
    std::vector<size_t> idx_off;            // per object in insertion order: first word of its index buffer in d_idx (SIZE_MAX: none)
    // srt_pt_set_dynamic_lights (the switch itself is built.dynamic_lights): the bytes of index buffers that went up for a light's
    // first update or refit (ensure_mesh_idx) and are counted with the verdict
    uint64_t idx_uncounted = 0;
    srt::BvhWorkspace bvh_ws;
    srt::DeviceBuffer<float> d_vpos, d_vnrm;
    // srt_pt_refit_mesh: per refitted mesh (insertion index) what its kernels keep on the device, from the first refit until the mesh
    // is rebuilt (srt_pt_update_mesh) or the scene committed again; and the refits so far
    std::map<uint32_t, srt::RefitTables> refit_tables;
    uint64_t refits = 0;
    // srt_pt_refit_mesh_inplace_device: per mesh refitted that way, as long as its refit tables live, the context's own copy of the
    // vertex arrays (24 B per vertex: the caller's arrays, and a skin's staging, may be overwritten before the host settles) and its
    // family - the mesh and its instances by insertion index, one lane each of the link kernel (pt_pose.h).
    struct Inplace {
      srt::DeviceBuffer<float> d_pos, d_nrm;
      srt::DeviceBuffer<uint32_t> d_family; uint32_t nfamily = 0;
    };
    std::map<uint32_t, Inplace> inplace;
    // The host's record lags the device after srt_pt_refit_mesh_inplace_device until settle(), as TopLevel's below does: the calls not
    // applied yet and the meshes they touched in first-seen order (at most one entry per mesh however many calls are pending).
    // Every such call refits the BVH<Object> too and is one of top.pending: top.event is the event behind the last of them.
    uint64_t pending = 0;
    std::vector<uint32_t> pending_meshes;
    void forget_pending() { pending = 0; pending_meshes.clear(); }
    // The refit tables of `object` (UINT32_MAX: of every mesh): its tree is about to be replaced.
    void drop_refit_tables(uint32_t object) {
      if (object == UINT32_MAX) { refit_tables.clear(); inplace.clear(); }
      else { refit_tables.erase(object); inplace.erase(object); }
    }
  } mesh;
  // srt_pt_repose_device: what its kernels keep on the device between calls - every object's record by insertion index, its
  // object-space box and its posed box - made at the first device repose after a commit and good only while `valid` (drop(): a
  // commit, a mesh update or refit and a host repose change what they mirror; so does a device repose that is refused).  The
  // per-call arrays (the list, the read-back staging, the mesh ordinals per slot, and under srt_pt_set_dynamic_lights the listed
  // lights as {position in the list, light} pairs) are grown on demand and kept.  d_active: srt_pt_set_active's table, one byte per
  // object by insertion index, made with the others from built.active (all 1: a fill on the device, nothing goes up).
  struct PoseTables {
    srt::DeviceBuffer<srt::Object> d_records; srt::DeviceBuffer<float> d_local_boxes, d_posed_boxes;
    srt::DeviceBuffer<uint8_t> d_active;
    bool valid = false;
    srt::DeviceBuffer<uint32_t> d_list;
    srt::DeviceBuffer<srt::PoseOut> d_out;
    srt::DeviceBuffer<uint32_t> d_slot_ordinal;
    srt::DeviceBuffer<uint32_t> d_light_list;
    void drop() {
      d_records.reset(); d_local_boxes.reset(); d_posed_boxes.reset(); d_active.reset();
      valid = false;
    }
  } pose;
  // srt_pt_skin, srt_pt_timeline, srt_pt_shading_timeline: counts srt_pt_scene_begin and srt_pt_scene_commit; a handle made under
  // another count is stale
  uint64_t scene_generation = 0;
  // srt_pt_repose_refit[_device]: the BVH<Object>'s refit tables (RefitTables of pt_bvh_device.h; d_tri_boxes stays empty - the posed
  // boxes of the pose tables are passed in its place) and the slot of every object, made at the first device-form refit of a tree and
  // dropped wherever the tree is replaced (drop_tables()).  list: what pose.d_list (and pose.d_light_list) hold, while list_valid: the
  // last call that wrote them was a device-form refit - a call with the same list uploads nothing.  pinned: host staging of the
  // lists, one buffer per list still on its way (its event tells), so that a call never waits for the one before.
  struct TopLevel {
    srt::RefitTables tables; bool have_tables = false;
    srt::DeviceBuffer<uint32_t> d_slot_of;
    std::vector<uint32_t> list; bool list_valid = false;
    uint32_t lights = 0, light_max_ntri = 0;              // of list: listed lights, and the largest triangle count among them
    struct PinnedList { srt::PinnedBuffer<uint32_t> h; srt::Event done; };
    std::vector<PinnedList> pinned;
    // The host's record lags the device after srt_pt_repose_refit_device until settle(): the calls not applied yet, the SET of
    // objects they listed (a flag per object and the objects in first-seen order: at most one entry per object however many calls
    // are pending), and the event recorded behind the last of them.  (ShadingLag below is the same arrangement for the shading tables.)
    // pending_active: those of the pending calls that were srt_pt_set_active_device (they are no refits, and settle() reads the
    // active table back only behind one of them).  mesh.pending of them were srt_pt_refit_mesh_inplace_device calls (counted by
    // srt_pt_refit_count, not as refits of this tree's poses).
    uint64_t pending = 0, pending_active = 0;
    std::vector<uint8_t> pending_flag;
    std::vector<uint32_t> pending_objects;
    srt::Event event;
    uint64_t refits = 0;                    // srt_pt_top_refit_count
    // The BVH<Object> is about to be replaced (or pose.d_list to be overwritten by another call: then only the list is forgotten).
    void forget_list() { list_valid = false; list.clear(); }
    void drop_tables() {
      tables = srt::RefitTables();
      have_tables = false;
      d_slot_of.reset();
      forget_list();
    }
    // No srt_pt_repose_refit_device call is waiting for settle() any more.
    void forget_pending() {
      pending = pending_active = 0;
      for (uint32_t i : pending_objects) pending_flag[i] = 0;
      pending_objects.clear();
    }
  } top;
  // srt_pt_shading_timeline_apply: the host's record of the materials / delta lights lags the device from a call that wrote them until
  // settle() reads d_mats / d_dlights back, behind the event recorded after the last such call.  While the materials lag,
  // elision_provable (pt.hip) proves nothing.
  struct ShadingLag {
    bool pending_mats = false, pending_lights = false;
    srt::Event event;
  } shade;
};

namespace srt {

// The one exit of scene data to the device, counted.  tri_class: triangle, normal, packed-triangle or BLAS-record bytes - what an
// instance shares and srt_pt_repose leaves alone (srt_pt_scene_counts tells them apart).
template <typename T>
inline int upload(srt_pt* pt, DeviceBuffer<T>* dst, const std::vector<T>& src, bool tri_class = false) {
  const int st = dst->upload(src);
  if (st != SRT_OK) return st;
  pt->bytes_uploaded += src.size() * sizeof(T);
  if (tri_class) pt->tri_bytes_uploaded += src.size() * sizeof(T);
  return SRT_OK;
}

int need_device(srt_pt* pt, const char* what);            // (pt_context.cpp)
// need_device, and the scene is committed, has a camera and an image size (pt_context.cpp)
int need_ready(srt_pt* pt, const char* what);
// In front of a launch of `what` that samples lights: SRT_OK with the mode off (and under the normal-colors view, which samples
// none); with SRT_ENV_SAMPLING_IMAGE the refusal of a scene whose environment is no Env_Map, else the sampler's tables, built and
// uploaded if this map has none yet (pt_context.cpp)
int env_image_ready(srt_pt* pt, const char* what);
// Which build a launch that env_image_ready let through takes: the ENVIMG one exactly when the mode is on and the tables are on the
// device.  device_scene() fills the table pointers under the same condition, so the two cannot disagree.
inline bool image_sampling_launch(const srt_pt* pt) { return pt->env_sampling == SRT_ENV_SAMPLING_IMAGE && pt->env_image.valid; }
// The same without a device: the refusal, or the host's copy of the tables in pt->env_image (the dump reads them)
int env_image_host_tables(srt_pt* pt, const char* what);
// env_image_ready whatever the mode says (the probes of srt_pt_debug.h): the refusal, or the tables on the device
int env_image_upload(srt_pt* pt, const char* what);
// The kernels' view of the committed scene; B: the scratch set whose ray-log ring they write, if any (pt.hip)
DScene device_scene(const srt_pt* pt, const srt_pt::EpochBuffers* B = nullptr);
// The scene fits the flattened per-lane walk of pt_flat.h (pt.hip)
bool flat_walk_fits(const FlatScene& F);
// SRT_CAST_STATS=1: the ray-cast kernel's sums on stderr, for srt_pt_destroy (pt.hip)
void report_cast_stats(srt_pt* pt);
// srt_pt_hit_device's cast path (pt.hip; the caller is pt_hit_device.hip): does pt_cast_kernel take the committed scene's world rays -
// what srt_pt_set_kernel(6) renders, a BVH<Object> on top, the traversal stack fits (the queries' launch shape is derived on the way;
// automatic: and the automatic mode streams the scene's render too);
// stream `s`'s scratch for chunks of up to `cap` rays with its counters zeroed on `s` (*nrays, *head: the words the pack kernel presets,
// *obj_shift: how a hit word packs its object); and the launch over the chunk that was packed.  The last two only enqueue, but for growth.
bool query_cast_applies(srt_pt* pt, bool automatic);
int query_cast_prepare(srt_pt* pt, hipStream_t s, size_t cap, srt_pt::QueryBuffers** out, uint32_t** nrays, uint32_t** head, uint32_t* obj_shift);
int query_cast_launch(srt_pt* pt, hipStream_t s, srt_pt::QueryBuffers& Q);
// (everything below: pt_update.cpp)
// settle(): the host's record catches up with the device after srt_pt_repose_refit_device calls - every entry point that is not itself
// enqueue-only calls it first (need_committed: and refuses, with not_committed's text, a scene that is not committed); discard_pending():
// what is pending describes a scene that goes.
int settle(srt_pt* pt);
void discard_pending(srt_pt* pt);
int not_committed(const char* what);
int need_committed(srt_pt* pt, const char* what);
// The device tables about the tree of mesh `object` (UINT32_MAX: of every mesh), the poses and the BVH<Object>: about to be replaced.
void drop_update_tables(srt_pt* pt, uint32_t object);
// BVH builds of sets at or above the context's threshold go to pt_bvh_device.hip: the context has a device and neither SRT_BVH_BUILDER=host
// nor srt_pt_set_bvh_builder says otherwise.  While a scope with `on` lives, the scene layer's builds do; it leaves the host builder behind.
bool device_builds(const srt_pt* pt);
struct DeviceBuilderScope {
  DeviceBuilderScope(const srt_pt* pt, bool on);
  ~DeviceBuilderScope();
};
// SRT_OK, or the refusal of trees deeper than the traversal stacks.
int check_depth(uint32_t tlas_depth, uint32_t blas_depth);

}  // namespace srt

#endif
