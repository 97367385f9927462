/*
 * srt_pt.h — C ABI of the MI355X (gfx950) path-tracer hot path.
 *
 * Drop-in boundary for PT::Pathtracer of the reference (paths relative to
 * /root/reference/Assignments/Scotty3D/src/):
 *
 *   srt_pt_scene_begin / add_material / add_mesh / add_sphere / scene_commit
 *                          <- Pathtracer::build_scene            rays/pathtracer.cpp:66-176
 *                             (Object ctor rays/object.h:18-34, Tri_Mesh::build student/tri_mesh.cpp:145-170,
 *                              BVH<>::build student/bvh.inl:35-163 — host or device, structure-identical)
 *   srt_pt_set_camera      <- `camera = cam` in begin_render     rays/pathtracer.cpp:267 (Camera: util/camera.h)
 *   srt_pt_set_params      <- Pathtracer::set_params             rays/pathtracer.cpp:182-189
 *   srt_pt_render_epoch    <- Pathtracer::do_trace(samples)      rays/pathtracer.cpp:209-231, i.e. for every pixel
 *                             trace_pixel (student/pathtracer.cpp:14-40) -> trace (:174-218) ->
 *                             sample_direct_lighting (:78-172) / sample_indirect_lighting (:42-76) ->
 *                             BVH<>::hit (student/bvh.inl:227-276), Triangle::hit (student/tri_mesh.cpp:32-111),
 *                             Sphere::hit (student/shapes.cpp:17-80), BBox::hit (student/bbox.cpp:5-62),
 *                             BSDF_*::scatter (student/bsdf.cpp:69-154), Samplers (student/samplers.cpp)
 *   srt_pt_accumulate      <- Pathtracer::accumulate             rays/pathtracer.cpp:195-207
 *   srt_pt_cancel          <- Pathtracer::cancel                 rays/pathtracer.cpp:282-290 (cancel_flag tested per sample, :224)
 *   srt_pt_read_ray_log    <- Pathtracer::log_ray                rays/pathtracer.cpp:191-193, called from student/pathtracer.cpp:148,
 *                             sink Gui::Widget_Render::log_ray   gui/widgets.cpp:625-628
 *
 * The epoch loop, progress/cancel bookkeeping and the GUI texture stay in the host class
 * (soft-rendering-toolsets_amd/host/pathtracer_hip.cpp); see INTEGRATION.md.
 *
 * Determinism: util/rand.cpp (thread_local mt19937 seeded from random_device) is replaced by SRT-RNG v1,
 * a counter-keyed generator re-keyed per (seed, pixel, sample); DESIGN.md states it.  Image rows follow
 * HDR_Image: row 0 = bottom (util/hdr_image.cpp:54-57).  Matrices are 16 floats in Mat4::data order
 * (column-major, lib/mat4.h).
 *
 *   srt_pt_tonemap         <- HDR_Image::tonemap_to              util/hdr_image.cpp:161-187 (Spectrum::to_srgb lib/spectrum.h:61-75)
 *   srt_pt_add_light / set_env_light / set_env_map / add_sphere_light
 *                          <- Pathtracer::build_lights           rays/pathtracer.cpp:26-64 (rays/light.cpp, student/env_light.cpp)
 *
 * Status codes and srt_last_error(): see srt_raster.h.  No CPU fallback: srt_pt_create fails without a
 * HIP device.
 *
 * Threads: a context is used from one host thread at a time (the reference's Pathtracer owns one worker per render).
 * The *_device entry points only enqueue work on the given stream; epochs enqueued on different streams may overlap on
 * the GPU (the library keeps one set of epoch scratch buffers per stream).
 */
#ifndef SRT_PT_H
#define SRT_PT_H

#include <stddef.h>
#include <stdint.h>

#include "srt_raster.h" /* srt_status, srt_last_error */

#ifdef __cplusplus
extern "C" {
#endif

/* Material kinds = the BSDF variants of rays/bsdf.h. */
enum {
    SRT_MAT_LAMBERTIAN = 0,    /* a = albedo as passed to BSDF_Lambertian(albedo) (divided by PI_F inside) */
    SRT_MAT_MIRROR = 1,        /* a = reflectance */
    SRT_MAT_GLASS = 2,         /* a = transmittance, b = reflectance, ior */
    SRT_MAT_DIFFUSE_LIGHT = 3, /* a = emitted radiance (Material::emissive()) */
    SRT_MAT_REFRACT = 4        /* a = transmittance, ior (the reference's scatter is a stub) */
};

typedef struct srt_pt_material {
    uint32_t type;
    float a[3];
    float b[3];
    float ior;
} srt_pt_material;

typedef struct srt_pt srt_pt; /* opaque */

/* One ray of the GUI's ray log (srt_pt_read_ray_log below). */
typedef struct srt_pt_logged_ray {
    float point[3];   /* Ray::point: the shading point */
    float dir[3];     /* Ray::dir, normalised by Ray's constructor */
    float t;          /* 5.0f: the length the reference asks the GUI to draw */
    uint32_t pixel;   /* y * width + x */
    uint32_t sample;  /* absolute sample index (sample_base + k), low 28 bits */
    uint32_t bounce;  /* 0 = the camera ray's hit */
} srt_pt_logged_ray;

int srt_pt_create(int device, srt_pt** out);
int srt_pt_destroy(srt_pt* pt);

/* ---- one render over the GPUs of a node, inside one process ----------------------------------
 * The reference's parallel axis is the epoch fan-out of Pathtracer::begin_render over its thread pool
 * (rays/pathtracer.cpp:250-280); here an epoch is cut into 32 x 32 image tiles dealt round-robin to `n` devices.  A group
 * owns one context per rank (rank r renders the tiles t with t % n == r; the scene is replicated: make every scene / camera /
 * kernel call on each srt_pt_group_context(g, r), r = 0 .. n-1), one stream per rank, and the exchange buffers.
 * srt_pt_group_render_epoch = every rank's srt_pt_render_epoch_device, ONE ncclGather of the tile radiance to rank 0 over
 * RCCL / xGMI (no reduction: the tiles are disjoint), srt_pt_untile_device on rank 0; the image is bit-identical to a
 * single context's.  RCCL is loaded at run time when n > 1 and every rank has its own device; ranks that share a device
 * (how the path is exercised on a one-GPU box) gather with device-to-device copies (SRT_PT_GATHER=copy|rccl forces one).
 * srt_pt_group_set_params replaces srt_pt_set_params for the members (it also sizes the exchange buffers).
 * The device form leaves the width*height*3 float image (row 0 = bottom) on rank 0's device and returns the stream it is
 * ordered on (srt_pt_accumulate_device / srt_pt_tonemap_device can follow on that stream); the host form copies it out.
 * One process per GPU with an external collective (torch.distributed / RCCL) remains available through srt_pt_set_tiling. */
typedef struct srt_pt_group srt_pt_group; /* opaque */
int srt_pt_create_multi(const int* devices, int n, srt_pt_group** out);
int srt_pt_group_destroy(srt_pt_group* g);
int srt_pt_group_size(srt_pt_group* g);
srt_pt* srt_pt_group_context(srt_pt_group* g, int rank);
int srt_pt_group_uses_rccl(srt_pt_group* g);
int srt_pt_group_set_params(srt_pt_group* g, uint32_t width, uint32_t height, uint32_t max_depth);
int srt_pt_group_render_epoch(srt_pt_group* g, uint64_t seed, uint32_t sample_base, uint32_t samples, float* rgb_out);
int srt_pt_group_render_epoch_device(srt_pt_group* g, uint64_t seed, uint32_t sample_base, uint32_t samples, float** d_image_out,
                                     void** stream_out);
/* Epochs in flight side by side.  The members render on one stream each; a second LANE - another stream per rank, another set of
 * exchange buffers and another image on rank 0 - lets the caller enqueue epoch k + 1 while epoch k runs, so that the tail of one
 * launch (the last paths of a few lanes) is filled by the next launch's blocks (Multi-GPU).  lane 0 is what
 * srt_pt_group_render_epoch[_device] use; lanes 0 .. 3 exist on demand.  *d_image_out stays valid until the next epoch on the
 * same lane. */
int srt_pt_group_render_epoch_lane(srt_pt_group* g, int lane, uint64_t seed, uint32_t sample_base, uint32_t samples, float** d_image_out,
                                   void** stream_out);
/* A whole render on the group with the accumulator kept ON THE DEVICES, every rank folding its own tiles (the running mean is per
 * pixel): no exchange per epoch at all - the ONE gather happens when somebody looks at the image.
 *   srt_pt_group_reset_accumulator   zero every rank's accumulator (a render that does not add samples)
 *   srt_pt_group_render_samples      srt_pt_render_samples_device on every rank, on lane `lane`
 *   srt_pt_group_wait_lane           wait for that lane's launches (then: cancelled? srt_pt_group_cancel_requested)
 *   srt_pt_group_fold                srt_pt_fold_epochs_device on every rank for the launch last rendered on `lane`; folds are ordered
 *                                    among themselves and against srt_pt_group_accumulator_image (events): call them in launch order
 *   srt_pt_group_accumulator_image   every rank's running mean as tile radiance, ONE ncclGather to rank 0 (copies between ranks that
 *                                    share a device), un-tiled: the width * height * 3 image on rank 0's device and its stream
 * Threads: fold and accumulator_image are not reentrant against each other - the caller serialises them (the drop-in class holds
 * its accumulator mutex); render_samples / wait_lane / fold belong to the render thread, accumulator_image may come from another.
 * Lanes and accumulators never move once srt_pt_group_set_params has returned (fixed storage, buffers sized there), so that one
 * thread's render_samples / wait_lane / fold / render_epoch_lane / read_ray_log on lanes 0 .. 2 may run concurrently with another
 * thread's accumulator_image (the display lane), and srt_pt_group_cancel may come from any thread at any time.  set_params,
 * reset_accumulator, set_ray_log and clear_cancel run while nothing else is called on the group. */
int srt_pt_group_reset_accumulator(srt_pt_group* g);
int srt_pt_group_max_samples_per_launch(srt_pt_group* g, uint32_t* samples);
int srt_pt_group_render_samples(srt_pt_group* g, int lane, uint64_t seed, uint32_t sample_base, uint32_t samples);
int srt_pt_group_wait_lane(srt_pt_group* g, int lane);
int srt_pt_group_fold(srt_pt_group* g, int lane, uint32_t samples_per_epoch, uint32_t position, uint32_t total_samples, uint32_t accumulator_samples);
int srt_pt_group_accumulator_image(srt_pt_group* g, float** d_image_out, void** stream_out);
int srt_pt_group_cancel_requested(srt_pt_group* g);
/* srt_pt_cancel / srt_pt_clear_cancel on every member; a cancelled srt_pt_group_render_epoch returns SRT_CANCELLED. */
int srt_pt_group_cancel(srt_pt_group* g);
int srt_pt_group_clear_cancel(srt_pt_group* g);
/* srt_pt_set_ray_log on every member / the rays logged by the epochs of `lane` on every member, merged in log order (waits for
 * that lane's streams). */
int srt_pt_group_set_ray_log(srt_pt_group* g, uint32_t capacity);
int srt_pt_group_read_ray_log(srt_pt_group* g, int lane, srt_pt_logged_ray* out, size_t cap, size_t* n_out, uint64_t* dropped);
/* srt_pt_set_normal_colors (below) on every member. */
int srt_pt_group_set_normal_colors(srt_pt_group* g, int on);
/* srt_pt_set_env_sampling (below) on every member. */
int srt_pt_group_set_env_sampling(srt_pt_group* g, uint32_t mode);
/* srt_pt_set_dynamic_lights (below) on every member. */
int srt_pt_group_set_dynamic_lights(srt_pt_group* g, int on);
/* srt_pt_set_active (below) on every member, and srt_pt_set_active_device with one device array per rank (d_active[r]: n bytes on
 * rank r's device; ranks that share a device may share the array), each on `stream` of its rank's device.  The group's lanes render
 * on streams of their own, which nothing orders behind `stream`: the device form settles every member (srt_pt_sync) before it
 * returns, so it waits.  A caller that wants the enqueue-only loop drives the members and their streams itself.  The first member's
 * refusal is returned; the list is the same for every member, so a refused list is refused by the first and nothing was written. */
int srt_pt_group_set_active(srt_pt_group* g, const uint32_t* objects, const uint8_t* active, uint32_t n);
int srt_pt_group_set_active_device(srt_pt_group* g, void* stream, const uint32_t* objects, const uint8_t* const* d_active, uint32_t n);
/* Device time of the exchange step of srt_pt_group_render_epoch[_device] - from the moment rank 0's own tiles are rendered to the end of
 * the un-tiling kernel on rank 0's stream: the gather (RCCL, or copies between ranks that share a device) and what it waits for, i.e. the
 * slowest other rank - summed over the epochs since the previous call (HIP events; waits for them); then recording on / off.  A diagnostic
 * for bench.py --group: together with the members' srt_pt_kernel_time it decomposes a multi-GPU step. */
int srt_pt_group_gather_time(srt_pt_group* g, int enable, double* total_ms, uint64_t* epochs);

/* ---- build_scene ---------------------------------------------------------------------------- */
int srt_pt_scene_begin(srt_pt* pt);
int srt_pt_add_material(srt_pt* pt, const srt_pt_material* m, uint32_t* index_out);
/* Object(Tri_Mesh(mesh, use_bvh), id, material, T).  positions/normals: nverts*3 floats; indices: 3 per
 * triangle.  is_area_light != 0 also appends the Tri_Mesh(mesh, false) copy to the area-light list
 * (materials of kind DIFFUSE_LIGHT, rays/pathtracer.cpp:105-116). */
int srt_pt_add_mesh(srt_pt* pt, const float* positions, const float* normals, uint32_t nverts,
                    const uint32_t* indices, uint32_t nindices, const float trans[16], uint32_t material,
                    int is_area_light);
/* Object(Shape(Sphere(radius)), id, material, T). */
int srt_pt_add_sphere(srt_pt* pt, float radius, const float trans[16], uint32_t material);
/* Object(<the Tri_Mesh of object `source_object`>.copy(), id, material, T) without the copy.  The reference's author names it at
 * rays/pathtracer.cpp:76-77 ("We could also do instancing instead of duplicating the bvh for big meshes"); where it matters is
 * :134-155, one Object per particle of a Scene_Particles, each with a byte copy of ONE built BVH<Triangle>.  source_object is the
 * 0-based insertion index of an object added earlier in this scene by srt_pt_add_mesh (an area light is fine: its light-list copy
 * stays what it is); a sphere, a sphere light, another instance, an index not yet added, a NULL trans or a material of kind
 * DIFFUSE_LIGHT (every emissive object goes into the area-light list with triangles of its own, :105-116) are SRT_ERR_INVALID
 * and leave the scene under construction usable.  The instance takes an insertion index and id like any object; its triangles,
 * normals and BVH<Triangle> are the source's - built, stored and uploaded once - and everything the scene computes is bit for
 * bit what srt_pt_add_mesh of the source's arrays would have given.  srt_pt_dump_bvh on it returns the shared arrays. */
int srt_pt_add_instance(srt_pt* pt, uint32_t source_object, const float trans[16], uint32_t material);
/* An emissive analytic sphere (a Scene_Object with a Shape and a diffuse_light material): rays intersect the sphere
 * (Sphere::hit), while the area-light list gets its triangle approximation obj.posed_mesh() as a Tri_Mesh without BVH
 * (rays/pathtracer.cpp:105-116).  positions / normals / indices = that mesh. */
int srt_pt_add_sphere_light(srt_pt* pt, float radius, const float trans[16], uint32_t material, const float* positions,
                            const float* normals, uint32_t nverts, const uint32_t* indices, uint32_t nindices);

/* A delta light (Pathtracer::point_lights, rays/pathtracer.cpp:26-64; rays/light.{h,cpp}): radiance =
 * Scene_Light::radiance(), trans = light.pose.transform() (column-major), angle_bounds (degrees) for spot lights
 * only.  Shadow rays of these lights are counted as rays like every other scene.hit. */
#define SRT_LIGHT_DIRECTIONAL 0u
#define SRT_LIGHT_POINT 1u
#define SRT_LIGHT_SPOT 2u
int srt_pt_add_light(srt_pt* pt, uint32_t type, const float radiance[3], const float angle_bounds[2], const float trans[16]);

/* The environment light (Pathtracer::env_light, rays/env_light.h): a uniform sphere (Env_Sphere) or upper hemisphere
 * (Env_Hemisphere) of the given radiance; rays that leave the scene see it, and sample_area_lights /
 * area_lights_pdf mix it with the area lights as the reference does (a coin flip, the mean of the pdfs). */
#define SRT_ENV_NONE 0u
#define SRT_ENV_SPHERE 1u
#define SRT_ENV_HEMISPHERE 2u
int srt_pt_set_env_light(srt_pt* pt, uint32_t type, const float radiance[3]);
/* Env_Map (an HDR_Image as environment): rgb = width * height * 3 floats, pixel (x, y) at index y * width + x as in
 * HDR_Image::at.  As in the reference fork, directions are sampled uniformly (pdf 1 / 4 PI) and Env_Map::evaluate
 * looks the image up bilinearly (student/env_light.cpp:7-93).  Every kernel form takes it (the wave kernel's DL build looks the map
 * up from the regenerated camera direction when a sample that left the scene is resolved). */
#define SRT_ENV_MAP 3u
int srt_pt_set_env_map(srt_pt* pt, uint32_t width, uint32_t height, const float* rgb);
/* Which of Env_Map's two samplers (rays/env_light.h:43-52) sample_area_lights / area_lights_pdf use for an environment map:
 * SRT_ENV_SAMPLING_UNIFORM, the fork's "step one" (student/env_light.cpp:8-32) and the default - every output is what it was
 * without the switch - or SRT_ENV_SAMPLING_IMAGE, its "step two": image_sampler, a Samplers::Sphere::Image
 * (student/samplers.cpp:27-137) - luminance * |sin theta| per texel, a normalised CDF, std::upper_bound on ONE draw, a pdf with a
 * Jacobian.  The reference's arithmetic bit for bit, quirks included: sample() returns the texel's corner direction without
 * jitter and draws one number where the uniform sampler draws two (the draw ledger of a sample changes); pdf() takes the sine of
 * the NORMALISED theta in [0, 1]; an index of w * h (row h) is a legal result of sample(); a black map has NaN tables and a map
 * with negative texels a CDF that is not sorted, on which the result is what libstdc++'s bisection steps arrive at.  So this mode
 * does not converge to the uniform mode's image and does not claim to.
 * A launch parameter like srt_pt_set_normal_colors: stored, read when a launch is enqueued, callable before or after the commit
 * and whenever nothing of the context is being enqueued.  An unknown mode is SRT_ERR_INVALID.  SRT_ENV_SAMPLING_IMAGE with an
 * environment that is no map (none, sphere, hemisphere) is refused, SRT_ERR_INVALID, by the LAUNCH that would sample it -
 * srt_pt_render_epoch[_device], srt_pt_render_samples_device, srt_pt_trace_samples and the group forms; the call itself only
 * stores the mode, and the normal-colors view, which samples no light, renders whatever the mode.  The sampler's tables (8 B per
 * texel and the doubles of sample()'s h + 1 rows and w columns) are built on the host in the reference's order - its float total
 * is accumulated serially, row-major - and uploaded by the first launch that needs them for a map; srt_pt_scene_begin and
 * srt_pt_set_env_map drop them.  That first launch is therefore NOT enqueue-only, whichever entry point makes it
 * (srt_pt_render_epoch_device, srt_pt_render_samples_device and the group's lane forms included): it builds the tables on the host,
 * allocates device memory and copies them with a blocking copy before it enqueues its kernels - do not capture it in a graph, and
 * expect a host wait; a caller that needs the loop enqueue-only from its first step makes one launch (srt_pt_trace_samples of one
 * sample will do) after the commit.  Every later launch for the same map only enqueues.  With the mode off nothing is built,
 * allocated, uploaded or counted.  Every kernel form that
 * takes an environment map takes the mode (srt_pt_set_kernel 0, 1, 2, 4, 6); the forms that refuse environment lights still do. */
#define SRT_ENV_SAMPLING_UNIFORM 0u
#define SRT_ENV_SAMPLING_IMAGE 1u
int srt_pt_set_env_sampling(srt_pt* pt, uint32_t mode);
int srt_pt_env_sampling(srt_pt* pt, uint32_t* mode);

/* Builds every BVH<Triangle> (leaf size 4) and the BVH<Object> (leaf size 1) exactly as the reference
 * does — or the List<> forms when use_bvh == 0 — flattens them and uploads the scene. */
int srt_pt_scene_commit(srt_pt* pt, int use_bvh);
/* New transforms for n objects of the committed scene (insertion indices; meshes, instances and spheres; trans: 16 floats per
 * object) without a rebuild: what a renderer of animations gets from the reference only by running build_scene again
 * (rays/pathtracer.cpp:66-176, per frame).  Runs with nothing of the context in flight and waits for the device itself.  The
 * listed Objects' itrans / has_trans / bbox are recomputed, the BVH<Object> is rebuilt (list order is kept when the scene was
 * committed with use_bvh == 0) and the tables that follow object order are uploaded again; no BVH<Triangle> is rebuilt and no
 * triangle, normal or BVH<Triangle> record is uploaded.  Afterwards the scene equals, bit for bit in everything it computes, a
 * fresh srt_pt_scene_begin .. srt_pt_scene_commit of the same objects with the new transforms.  SRT_ERR_INVALID: an area light
 * in the list (its light tables depend on its pose: commit again) unless srt_pt_set_dynamic_lights, a duplicate, an index out of range.  SRT_ERR_STATE: no
 * committed scene.  New poses that make the reference's BVH<Object> build non-terminating or too deep for the traversal stacks
 * fail as srt_pt_scene_commit does (SRT_ERR_UNSUPPORTED) - and the committed scene stays exactly as it was. */
int srt_pt_repose(srt_pt* pt, const uint32_t* objects, const float* trans, uint32_t n);
/* Area lights in srt_pt_repose[_device], srt_pt_update_mesh[_device], srt_pt_refit_mesh[_device] and srt_pt_skin_create.  Default:
 * off - those calls refuse an area light with the status and message they always had, and no output of any call changes.  While
 * it is on:
 *   srt_pt_repose[_device] take emissive meshes (is_area_light) and emissive spheres (srt_pt_add_sphere_light) in their list: next to
 *   the object record, the BVH<Object> and the tables of object order, each listed light's record in the light list - has_trans,
 *   trans, itrans and Object::pdf's pair T = I * trans, iT = itrans * I (rays/object.h:90-94; identities when trans == I) - and the
 *   2 / |cross(T v1 - T v0, T v2 - T v0)| factor of Triangle::pdf (student/tri_mesh.cpp:137) of each of its triangles take the
 *   values a fresh commit with the new transform gives them; the object-space corners and the light-list triangle copies stay.
 *   srt_pt_update_mesh[_device] / srt_pt_refit_mesh[_device] take an emissive MESH (a sphere light stays refused as a sphere): the
 *   object's triangles and BVH<Triangle> go the way any mesh's go, and the light-list copy (Tri_Mesh(mesh, false), index order)
 *   and the light's per-triangle sample corners and factors are rewritten in place; no count changes.
 *   srt_pt_skin_create takes an emissive mesh; srt_pt_skin_pose[_refit] go through the two calls above, and fail with their refusal
 *   if the switch has been cleared since.
 * After a successful call the scene computes, bit for bit, what a fresh commit of the same description computes; a zero-area
 * light triangle (factor inf) and a singular pose (infinities, NaNs) are what a fresh commit gives too, not refusals.  In every
 * failing case the committed scene stays exactly as it was, light tables included: no live light array is written before the
 * verdict.  The device forms write the light tables with kernels after their verdict and their wait (pt_light_update.hip) and
 * upload no light record; the host forms upload the listed lights' records (272 B per light, 64 B per light triangle, and after
 * new vertices 132 B per triangle of the light-list copy).  An emissive mesh's index buffer (12 B per triangle) is resident from
 * the commit when the switch was on by then, otherwise from the light's first update, refit or skin.  May be set or cleared
 * whenever nothing of the context is being enqueued (the rule of srt_pt_set_elision), before or after srt_pt_scene_commit. */
int srt_pt_set_dynamic_lights(srt_pt* pt, int on);
/* The same with the transforms in device memory (a simulation's output: a rigid-body kernel, a torch op,
 * srt_pt_particle_transforms_device): `objects` is a host array of n insertion indices as above, d_trans holds n * 16 floats in
 * Mat4::data order and is read on `stream` (a hipStream_t; NULL: the null stream) behind whatever the caller enqueued there.
 * Preconditions, refusals, their status codes and their messages are srt_pt_repose's, checked on the host before anything is
 * enqueued; a host-only context (device = -1) validates and then returns SRT_ERR_UNSUPPORTED.  A kernel computes what the poses
 * decide - itrans, has_trans and the posed box of the listed objects, one lane each - and those values come back once (156 B per
 * listed object) so that the host's record of the scene stays true: srt_pt_dump_bvh and every later srt_pt_repose /
 * srt_pt_update_mesh / srt_pt_refit_mesh see the new poses.  The BVH<Object> is built by the rule of srt_pt_set_bvh_builder /
 * SRT_BVH_BUILDER: on the device, over the posed boxes where the kernel left them, for a scene of at least min_primitives
 * objects; otherwise on the host, over the boxes read back (24 B per object).  The object records are rewritten in place by a
 * kernel - no record is uploaded: the order of a host-built tree (4 B per slot) and the mesh ordinals (4 B per slot, when a mesh
 * has a real BVH<Triangle>) go up with the nodes and sweep tables srt_pt_repose uploads, and the context's first device repose
 * after a commit sends 24 B of object-space box per object.  Afterwards the scene equals, bit for bit in everything it computes,
 * what srt_pt_repose of the same matrices gives; only storage and the upload counter may differ.  In every refused case the
 * committed scene stays exactly as it was, on the host and on the device: the kernels write tables of their own, and the tree
 * and the tables of object order are built aside and checked before the first write to a live array, which comes after the wait
 * srt_pt_repose makes.  (A HIP failure after that point is SRT_ERR_HIP and leaves the context without a committed scene: commit
 * again.)  Copies and kernels go on `stream`, which the call synchronises where the host needs a verdict and before it returns. */
int srt_pt_repose_device(srt_pt* pt, void* stream, const uint32_t* objects, const float* d_trans, uint32_t n);
/* New transforms for n objects WITHOUT rebuilding the BVH<Object>: the tree keeps its node links {start, size, l, r} and its
 * primitive order and takes new boxes - every leaf the BBox::enclose fold, from BBox(), of Object::bbox of its objects in
 * primitive order (0 or 1), every interior node the enclose of its left child's box and then its right child's, which is how
 * BVH<Primitive>::build forms node boxes (student/bvh.inl:73-75, 119-123).  A refit with the committed poses therefore gives the
 * committed boxes back, as values (the zero-sign caveat of srt_pt_refit_mesh applies).  The listed objects get the itrans,
 * has_trans and posed box the Object ctor and Object::bbox give them; results are those of the reference's BVH<Object>::hit and
 * Object::hit on that tree - the closest hit does not depend on the tree except at exact ties, the cost of finding it does:
 * srt_pt_scene_tree_cost tells when a rebuild (srt_pt_repose[_device]) pays.  Arguments, preconditions, refusals, status codes
 * and messages are srt_pt_repose's (an area light is refused unless srt_pt_set_dynamic_lights is on; a listed light then takes
 * the record and area terms srt_pt_repose gives it).  Non-finite matrices are not refused, by either form: the scene computes
 * what the definition (prepare_top_refit / apply_top_refit, pt_scene.h) computes from them.  Counts, object slots, node_base,
 * ordinals, the lazy tables, the depth of the tree, the kernel form and every BVH<Triangle> stay.  A scene committed with
 * use_bvh == 0 has no tree: the listed records alone are rewritten.  A host-only context runs the definition and nothing else.
 * On a device context the call waits as srt_pt_repose waits, then uploads what changed and nothing else: the top-level nodes
 * (32 B each), the sweep records (64 B each), the listed object records (176 B each) and the listed lights' records - no table
 * of object order. */
int srt_pt_repose_refit(srt_pt* pt, const uint32_t* objects, const float* trans, uint32_t n);
/* The same from device transforms (d_trans: n * 16 floats, read on `stream`), ENQUEUE-ONLY.  The list is validated on the host
 * before anything is enqueued (a host-only context validates and then returns SRT_ERR_UNSUPPORTED); after that the call cannot
 * fail for a reason the scene gives - depth, node count, record count, object order, kernel form and stack sizes are those of
 * the committed tree, so there is no verdict to wait for - and it only enqueues on `stream` and returns: no
 * hipStreamSynchronize, no hipDeviceSynchronize, nothing copied to the host.  On `stream`, in order: the pose kernel of
 * srt_pt_repose_device; the leaves from the posed boxes through the primitive order; the interior levels, deepest first; the
 * boxes into the live top-level nodes and sweep records; the listed objects' trans / itrans / has_trans into their live
 * records; the listed lights' records and area terms.  Box arithmetic is compares and loads only.
 *   Blocking work: the FIRST call after a commit, and after any call that replaces the BVH<Object> (srt_pt_repose[_device],
 * srt_pt_update_mesh*, srt_pt_refit_mesh*, the skin poses), allocates and uploads its tables - the pose tables it shares with
 * srt_pt_repose_device (24 B per object) and the tree's refit tables (about 28 B per object, plus 4 B per level of the tree for
 * the level offsets) - counted once.  A steady-state
 * call uploads the list (4 B per listed object, 8 B more per listed light) through pinned memory, and nothing at all when the
 * list equals the previous call's.  A list longer than any before grows device arrays, which waits, once.
 *   Ordering: the new arrays are visible to whatever is enqueued on `stream` behind the call.  Epochs on other streams, and a
 * later enqueue-only call on another stream, are ordered by the caller with events (the rule of the epoch folds): nothing in
 * flight elsewhere may read the scene while the refit writes it.  The enqueue-only *_device render calls do not settle.
 *   The host's record of the scene LAGS after this call and settles on demand: every entry point that is not itself
 * enqueue-only first waits for an event recorded behind the last such call, reads back the records by insertion index (176 B
 * per object) and the top-level boxes (24 B per node) once - however many calls are pending - and applies them to its own
 * record (the lights' through its own arithmetic).  That covers srt_pt_sync, srt_pt_dump_bvh, srt_pt_dump_lights,
 * srt_pt_scene_tree_cost, srt_pt_scene_counts, srt_pt_repose[_device], srt_pt_repose_refit, srt_pt_update_mesh*,
 * srt_pt_refit_mesh*, the skin poses, srt_pt_hit, srt_pt_trace_samples, srt_pt_particles_step and srt_pt_render_epoch (host
 * forms); srt_pt_scene_begin, srt_pt_scene_commit and srt_pt_destroy wait and discard what is pending (no read-back).  What the
 * context keeps while it lags is one flag and at most one list entry per object, however many calls are pending.  A HIP error
 * found while settling, or after the call has begun to enqueue, is SRT_ERR_HIP and leaves the context without a committed
 * scene and with nothing pending: commit again. */
int srt_pt_repose_refit_device(srt_pt* pt, void* stream, const uint32_t* objects, const float* d_trans, uint32_t n);
/* tree_cost (the SAH figure of srt_pt_mesh_tree_cost) of the BVH<Object> as it is now, after settling: what a caller of
 * srt_pt_repose_refit[_device] watches to decide when to pay for a rebuild with srt_pt_repose_device.  SRT_ERR_UNSUPPORTED for a
 * scene committed without BVHs, SRT_ERR_STATE without a commit. */
int srt_pt_scene_tree_cost(srt_pt* pt, double* cost);
/* One lane per particle: d_trans_out[16 k ..] = Mat4::translate(pos_k) * Mat4::scale(Vec3{scale}), the T of
 * rays/pathtracer.cpp:149, bit-equal to Mat4::operator* (zero signs included).  d_pos holds 3 floats per particle - the layout
 * srt_pt_particles_step_device updates in place - so that step -> transforms -> srt_pt_repose_device -> render has no host data
 * in it (and with srt_pt_repose_refit_device in the place of srt_pt_repose_device, no host wait either).  Only enqueues on
 * `stream`; does not synchronise.  The CAPACITY is fixed: n is the number of particle objects the scene was committed with.  Within it
 * the population changes without a commit: srt_pt_set_active[_device] switches a dead particle's object off and a spawned one's on
 * (the pool loop under srt_pt_set_active_device). */
int srt_pt_particle_transforms_device(srt_pt* pt, void* stream, const float* d_pos, uint32_t n, float scale, float* d_trans_out);
/* Switches objects of the committed scene off and on without committing again: what Scene_Particles::step2 does to its vector of
 * particles each step (dead ones dropped, new ones appended), for a pool of fixed capacity.  `objects` are n insertion indices,
 * active[k] belongs to objects[k], non-zero means active - the layout of srt_pt_particles_step's `alive` with the particles'
 * indices as `objects`.  Every object is active after srt_pt_scene_commit; srt_pt_scene_begin and srt_pt_scene_commit drop the table.
 *   Definition.  With posed_k = Object::bbox of object k, the effective box is E_k = active_k ? posed_k : BBox(), the reference's
 * empty box (min = +FLT_MAX, max = -FLT_MAX on every axis, lib/bbox.h).  The BVH<Object> keeps its links and its primitive order;
 * while any object is inactive its node boxes are srt_pt_repose_refit's fold over E (BBox::enclose of an empty box changes
 * nothing), written into the top-level nodes and the sweep records; with every object active again they are that fold over the
 * posed boxes - the committed boxes as values.  Topology never depends on the flags: every call that builds the BVH<Object>
 * (srt_pt_scene_commit, srt_pt_repose[_device], srt_pt_update_mesh*, srt_pt_refit_mesh*, the skin poses, the timelines' repose)
 * builds over the posed boxes of ALL objects and then, only while an object is inactive, ends with the masked fold;
 * srt_pt_repose_refit[_device] and the timelines' repose_refit feed E to their leaf stage.  Nothing else of an inactive object
 * changes: its record, its material and its posed box stay and keep following repose, refit, update and skin calls, so it returns
 * where it would be.  A mesh that instances are made of may be inactive while its instances stay active.
 *   Results are those of the reference's BVH<Object>::hit and BBox::hit on that tree with those boxes, a leaf whose objects are
 * all inactive holding no primitive.  BBox::hit of the empty box is false for every ray without a NaN component - but that alone
 * hides nothing: find_closest_hit visits the child whose box was MISSED whenever the other child returns a hit farther than
 * ray.dist_bounds.x (cur_far_t starts as ray.dist_bounds, student/bvh.inl:191-192, 216).  So the tables the kernels walk also give
 * such a leaf the count 0 - the count word of its top-level node and the l_cnt / r_cnt of the sweep record above it - as a build
 * gives an empty leaf (a leaf of the BVH<Object> holds 0 or 1); srt_pt_dump_bvh keeps showing the committed links and sizes.
 * Nothing that walks the BVH<Object> - path rays, shadow rays, srt_pt_hit, srt_pt_particles_step[_device] - reaches an inactive
 * object, and closest hits are those of a fresh commit without it, exact ties apart.  CAVEAT: a ray with a NaN component passes
 * every box, today as before; an inactive object shares its leaf with no other (the leaf is empty), so such a ray finds nothing
 * there either, but no promise is made about rays with NaN components.  srt_pt_scene_tree_cost counts a node whose box is empty
 * (mn > mx on an axis) as 0, and an empty root gives cost 0.
 *   Refusals, the scene staying exactly as it was on the host and on the device (nothing live is written before the verdict):
 * SRT_ERR_STATE without a committed scene; SRT_ERR_UNSUPPORTED for a scene committed with use_bvh == 0 (a list scene has no boxes)
 * and for a scene whose BVH<Object> root is a leaf (a single object: find_closest_hit tests children only, the root's box never);
 * SRT_ERR_INVALID for a NULL argument with n > 0, an index out of range, a duplicate, and an emissive object - an emissive mesh or a
 * sphere light, also under srt_pt_set_dynamic_lights: the light list would go on sampling it.
 *   This form BLOCKS: it settles and waits as srt_pt_repose_refit waits, runs the definition on the host's record and uploads the
 * top-level nodes (32 B each: boxes and leaf counts) and the sweep records (64 B each), nothing else.  A call that changes no flag writes and uploads
 * nothing.  A host-only context runs the definition and nothing else. */
int srt_pt_set_active(srt_pt* pt, const uint32_t* objects, const uint8_t* active, uint32_t n);
/* The same with the flags in device memory (d_active: n bytes, read on `stream` - srt_pt_particles_step_device's d_alive as it
 * is), ENQUEUE-ONLY under the contract of srt_pt_repose_refit_device: the list is validated on the host first (refusals and status
 * codes as above; a host-only context validates and then returns SRT_ERR_UNSUPPORTED), then the call only enqueues on `stream`, in
 * order: a kernel copies the listed flags into the context's table (1 B per object, by insertion index); the leaf stage of the
 * refit reads E - the posed boxes masked by the table; the interior levels, deepest first; the boxes into the live top-level nodes
 * and sweep records; the leaf counts into the same (two small launches).  No synchronisation, no read-back.  Steady state uploads the list (4 B per listed object) and nothing when
 * the list equals the previous device-form call's - srt_pt_repose_refit_device's included: the two share the list.  Blocking work
 * only where srt_pt_repose_refit_device has it: the first call after a commit or a rebuild (the same tables; 1 B per object more
 * for the table while an object is inactive), and growth.  Ordering is srt_pt_repose_refit_device's.  The host's record lags and
 * settles on the same path, which behind such a call additionally reads the table back (1 B per object).
 *   The pool loop, all on one stream and without a host wait: srt_pt_particles_step_device -> srt_pt_particle_transforms_device
 * -> srt_pt_set_active_device(d_alive) -> srt_pt_repose_refit_device -> srt_pt_render_epoch_device.  Spawning into the dead slots,
 * the substep loop and the rest of Scene_Particles::step are srt_pt_emitter's (below), which runs this loop for a pool it owns. */
int srt_pt_set_active_device(srt_pt* pt, void* stream, const uint32_t* objects, const uint8_t* d_active, uint32_t n);
/* The table after settling: one byte per object in insertion order (1 active, 0 inactive) into active_out[0 .. objects).
 * SRT_ERR_INVALID when cap is less than the object count, SRT_ERR_STATE without a commit. */
int srt_pt_get_active(srt_pt* pt, uint8_t* active_out, uint32_t cap);
/* New vertex arrays for ONE mesh of the committed scene without committing again: what a renderer of deforming meshes (a skinned
 * skeleton, cloth, a caller's own kernel) gets from the reference only by running build_scene again on Scene_Object::posed_mesh()
 * (rays/pathtracer.cpp:66-176, per frame).  `object` is the insertion index of an object added by srt_pt_add_mesh; positions /
 * normals are nverts * 3 floats and nverts is what the mesh was added with; the index buffer, material, transform and instance
 * relations stay.  Runs with nothing of the context in flight and waits for the device itself.  Exactly one BVH<Triangle> (leaf
 * size 4) is built - on the host or the device by the rule of srt_pt_set_bvh_builder / SRT_BVH_BUILDER; none when the scene was
 * committed with use_bvh == 0: the triangles then stay in index order and the object's box is List<Triangle>::bbox - and the
 * mesh's triangle, normal and packed-triangle records are rewritten in place by a kernel from the 24 B per vertex that go up (and
 * 4 B per triangle of primitive order after a host build); no other mesh's are touched or uploaded.  The mesh's BVH<Triangle>
 * nodes and interior records may be more or fewer than before: the ranges stored behind them are re-packed and uploaded again
 * when they move, left alone when they do not.  Every instance of the mesh follows (its triangles and BVH<Triangle> are the
 * source's, its object-space box the new root box), so the BVH<Object> is rebuilt and the tables that follow object order are
 * replaced as in srt_pt_repose.  Afterwards the scene equals, bit for bit in everything it computes, a fresh srt_pt_scene_begin
 * .. srt_pt_scene_commit of the same objects with the new arrays; only storage and counters may differ.  SRT_ERR_STATE: no
 * committed scene.  SRT_ERR_INVALID: a NULL argument, an index out of range, a sphere or sphere light, an instance (the message
 * names its source: update that), an area light (its light-list copy and light tables depend on the vertices: commit again)
 * unless srt_pt_set_dynamic_lights, nverts differing from the committed count.  Arrays that make the reference's BVH<Triangle> or BVH<Object> build non-terminating
 * or too deep for the traversal stacks fail as srt_pt_scene_commit does (SRT_ERR_UNSUPPORTED).  In every failing case the
 * committed scene stays exactly as it was, on the host and on the device: everything is built aside and checked before the
 * first write.  (A HIP failure after that point - out of device memory while the tables are replaced - is SRT_ERR_HIP and leaves
 * the context without a committed scene: commit again.)  The builder's workspace and the vertex staging are kept between calls;
 * like srt_pt_repose the call allocates the three tables of object order anew, and the node / record arrays too when the mesh's
 * node / record count changed.  Works on a host-only context (device = -1). */
int srt_pt_update_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);
/* The same with the two arrays in device memory (a skinning kernel's output): copies and kernels are enqueued on `stream`
 * (a hipStream_t; NULL: the null stream), which the call synchronises where the host needs a verdict and before it returns.  The
 * arrays are copied back once (24 B per vertex) so that the host's record of the scene stays true; with the host builder, or a
 * mesh below the device builder's threshold, the triangle boxes are computed from that copy. */
int srt_pt_update_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts);

/* New vertex arrays for one mesh WITHOUT rebuilding its BVH<Triangle>: a refit, what every renderer of animations does for a mesh
 * whose connectivity stays while its vertices move.  Arguments, preconditions, refusals and their messages are
 * srt_pt_update_mesh's, plus one: a non-finite position coordinate is SRT_ERR_INVALID.  For finite vertices the mesh's
 * BVH<Triangle> keeps its node links {start, size, l, r} and its primitive order; every leaf box becomes the BBox::enclose fold of
 * Triangle::bbox (student/tri_mesh.cpp:7-30, the +1.0f of a flat axis included) over its triangles, every interior box the enclose
 * of its two children's.  BVH<Primitive>::build forms every node box as such min / max folds of its primitives' boxes
 * (student/bvh.inl:73-75, 119-123), exact and independent of order, so a refit with the committed vertices gives the committed
 * boxes back - as values: where a bound is a zero that some triangles carry as +0 and others as -0 the fold's order picks the
 * sign, and the build's order inside a node is its partition's; no slab test can tell the two zeros apart.  Results are those
 * of the reference's BVH<Triangle>::hit (student/bvh.inl:166-276) and Triangle::hit on that tree.
 * The triangle, normal and packed-triangle records are rewritten in place in the kept order, the mesh's nodes and interior
 * records take the new boxes in place; counts never change, nothing is re-packed or reallocated, and no other mesh's storage is
 * touched.  The object-space box of the mesh and of each of its instances becomes the new root box; the BVH<Object> and the
 * tables of object order are replaced as in srt_pt_repose.  A device context refits on the device whatever
 * srt_pt_set_bvh_builder says (pt_mesh_update.hip: triangle boxes, leaves, the interior levels deepest first) and reads the node
 * boxes back, 24 B per node, so that srt_pt_dump_bvh stays true; the tables the kernels need (primitive order, level lists,
 * record children) go up at the mesh's first refit and are dropped when srt_pt_update_mesh rebuilds the mesh or the scene is
 * committed again.  A host-only context (device = -1) refits on the host: that code (refit_boxes, pt_scene.cpp) is the
 * definition the device is held to.  A BVH<Object> build that does not terminate or comes out too deep is SRT_ERR_UNSUPPORTED.
 * In every failing case the committed scene stays exactly as it was, on the host and on the device: the new boxes are computed
 * aside and the top half is built aside before the first write to a live array.  With a scene committed with use_bvh == 0 there
 * is no tree and the call does what srt_pt_update_mesh does.  A later srt_pt_update_mesh on a refitted mesh rebuilds it (the
 * scene then equals a fresh commit); a skin created before a refit stays valid.  A refitted tree is valid but may be worse than
 * a rebuilt one: srt_pt_mesh_tree_cost tells.  The refusals are srt_pt_update_mesh's: an area light is refused unless
 * srt_pt_set_dynamic_lights. */
int srt_pt_refit_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);
/* The same with the two arrays in device memory: copies and kernels are enqueued on `stream` (a hipStream_t; NULL: the null
 * stream), which the call synchronises where the host needs a verdict (the arrays come back once, 24 B per vertex, and are
 * checked there; the root box comes back with the node boxes) and before it returns. */
int srt_pt_refit_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts);
/* New vertex arrays for one mesh with BOTH trees kept: srt_pt_refit_mesh without the rebuild of the BVH<Object>.  Arguments,
 * preconditions, refusals and their messages are srt_pt_refit_mesh's, a non-finite position coordinate (SRT_ERR_INVALID) included.
 * The mesh's BVH<Triangle>, its triangle, normal and packed records and its light-list copy change exactly as srt_pt_refit_mesh
 * changes them, and the object-space box of the mesh and of each of its instances becomes the new root box.  The BVH<Object> keeps
 * its links {start, size, l, r} and its primitive order and takes new boxes as in srt_pt_repose_refit: a leaf's is the
 * BBox::enclose fold, from BBox(), of Object::bbox (rays/object.h:51-55) of its objects - every object's from its unchanged transform
 * and its object-space box, BBox() for what srt_pt_set_active switched off - an interior node's the enclose of its left and then its
 * right child's (student/bvh.inl:73-75, 119-123).  No link, order, count, slot, ordinal, lazy table or depth changes anywhere, so the
 * call cannot fail for a tree's sake: the scene is what srt_pt_refit_mesh would leave if its last step were srt_pt_repose_refit of
 * the mesh and its instances with their current transforms in place of the rebuild.  Results are those of the reference's
 * BVH<Primitive>::hit (student/bvh.inl:166-276) on those trees; srt_pt_mesh_tree_cost and srt_pt_scene_tree_cost tell when a
 * rebuild (srt_pt_update_mesh, srt_pt_repose) pays.  Blocks, and settles first.  A host-only context (device = -1) runs the
 * definition (prepare_mesh_refit_inplace / apply_mesh_refit_inplace, pt_scene.cpp) and nothing else.  A device context uploads only
 * what changed: the vertices into the staging (24 B each), the top-level nodes and sweep records (32 B and 64 B each); the mesh's
 * boxes and records are written by the kernels of srt_pt_refit_mesh, whose tables it shares.  No table of object order goes up and
 * the refit tables of both trees stay.  With a scene committed with use_bvh == 0 there is no tree and the call does what
 * srt_pt_update_mesh does.  srt_pt_refit_count counts it. */
int srt_pt_refit_mesh_inplace(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);
/* The same from two device arrays, ENQUEUE-ONLY under the contract written at srt_pt_repose_refit_device: the host validates first
 * (srt_pt_update_mesh's refusals, status codes and texts; a host-only context validates and then returns SRT_ERR_UNSUPPORTED) and
 * then only enqueues on `stream` (a hipStream_t; NULL: the null stream) - no wait, no synchronisation, nothing copied to the host.
 * In order: the two arrays are copied device-to-device into buffers the context owns for that mesh (24 B per vertex), so the
 * caller's arrays - and a skin's staging - may be overwritten as soon as work enqueued behind the call may run; the triangle boxes,
 * the leaves and the levels of the mesh's tree (pt_mesh_update.hip); its live nodes and interior records; its triangle records in
 * the kept order; for an emissive mesh under srt_pt_set_dynamic_lights its light tables (pt_light_update.hip); the link (pt_pose.hip,
 * one lane per member of the mesh's family - the mesh and its instances): the new root box as the member's object-space box and
 * Object::bbox of it under the member's current transform, in the tables srt_pt_repose_refit_device keeps; and that call's own
 * stages over them - the leaf stage masked by the active table, the levels, the live top-level nodes and sweep records.  Blocking
 * work only where srt_pt_repose_refit_device has it: the first call after a commit or after a call that replaced a tree (its
 * tables, the mesh's refit tables, the family - 4 B per member - and the vertex buffers; counted once), so a steady-state call
 * uploads nothing.  Ordering is that call's: work enqueued behind it on `stream` sees the new scene, other streams are the
 * caller's to order with events.  The two calls share their tables: a srt_pt_repose_refit_device behind this call poses the new boxes.
 * NON-FINITE VERTICES ARE NOT REFUSED by this form - there is no verdict to wait for: the scene holds what the kernels computed,
 * and the host's record takes the vertices and the node boxes as read back.  A caller who wants the check uses the blocking forms
 * (srt_pt_refit_mesh_inplace, srt_pt_refit_mesh[_device]).  The host's record lags until the next call that is not enqueue-only
 * settles it: one wait, and per mesh touched - however many calls are pending - one read-back of 24 B per vertex and 24 B per node
 * (srt_pt_mesh_refit_pending, srt_pt_debug.h); every pending call is pending for srt_pt_top_refit_pending too, and counted by
 * srt_pt_refit_count, not srt_pt_top_refit_count.  A HIP error after the first enqueue or while settling is SRT_ERR_HIP and leaves
 * the context without a committed scene and with nothing pending.  With a scene committed with use_bvh == 0 the call does what
 * srt_pt_refit_mesh_device does, and BLOCKS as it does. */
int srt_pt_refit_mesh_inplace_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts);
/* SAH cost of the mesh's current BVH<Triangle>, on the host in double from the host node boxes: the sum over interior nodes of
 * SA(n) / SA(root) plus the sum over leaves of size(n) * SA(n) / SA(root), SA = 2 (xy + yz + zx) of a box's extents.  What a
 * caller compares before and after refits to decide when to rebuild with srt_pt_update_mesh.  Refusals as for srt_pt_refit_mesh;
 * SRT_ERR_UNSUPPORTED for a scene committed with use_bvh == 0.  Settles first, so the cost behind enqueue-only in-place refits is
 * the refitted tree's. */
int srt_pt_mesh_tree_cost(srt_pt* pt, uint32_t object, double* cost);

/* ---- Skinning: Skeleton::find_joints and Skeleton::skin on the device ----
 * What Scene_Object::sync_anim_mesh (scene/object.cpp:106-129) does on the CPU per frame - Skeleton::find_joints
 * (student/skeleton.cpp:219-256), Skeleton::skin (:258-307) and, without smooth normals, the flat-normal loop (:114-126) - as
 * kernels whose output feeds srt_pt_update_mesh_device: a frame of a skinned mesh sends 64 B per joint up and nothing else.
 * A skin is bound to one context and to one object of its committed scene added by srt_pt_add_mesh.  Results equal the
 * reference's bit for bit (x86-64, no contraction); where the reference yields NaN (a vertex ON a bone has distance 0 and
 * weight inf / inf) so do the kernels, up to the NaN's sign and payload.
 * Limits (SRT_ERR_UNSUPPORTED beyond): at most 4096 joints per skin, and nverts * njoints <= 2^31 (the map's offsets are
 * 32-bit).  Destroy a context's skins before the context. */
typedef struct srt_pt_skin srt_pt_skin; /* opaque */
/* One joint: `bind` is Skeleton::joint_to_bind(j) in Mat4::data order (column-major), extent and radius are Joint::extent and
 * Joint::radius.  The caller lists the joints in the order Skeleton::for_joints visits them; that order is part of the result: a
 * vertex's influence list, and so the order of its float sums, follows it. */
typedef struct srt_pt_skin_joint {
    float bind[16];
    float extent[3];
    float radius;
} srt_pt_skin_joint;
/* find_joints.  Needs a committed scene (SRT_ERR_STATE).  `object`, and SRT_ERR_INVALID with its messages for a NULL argument,
 * an index out of range, a sphere, an instance, an area light (unless srt_pt_set_dynamic_lights) and nverts differing from the
 * committed count, are as for srt_pt_update_mesh; njoints == 0 is SRT_ERR_INVALID too.  bind_positions / bind_normals (nverts * 3 floats each) are the
 * object's bind-pose mesh - the committed vertices may already be a posed frame - and stay on the device with the skin.  The host
 * computes Mat4::inverse(bind) (lib/mat4.h:299-351, the `/= det()` included) once per joint; kernels build the vertex -> joints
 * map as CSR (count, exclusive scan, fill; a vertex's joints in ascending index) with the reference's capsule test per (vertex,
 * joint) - inverse * pos through Vec4::project, closest_on_line_segment (:195-217) as written, norm() <= radius - and store each
 * influence's weight (1.0f / distance) / sum_of_inv_dis (:280-299), summed in list order: weights do not depend on the pose, so
 * computing them once is what the reference recomputes per frame.  Waits for the device.  A host-only context (device = -1)
 * validates the arguments and returns SRT_ERR_UNSUPPORTED: skinning has no CPU path. */
int srt_pt_skin_create(srt_pt* pt, uint32_t object, const float* bind_positions, const float* bind_normals, uint32_t nverts,
                       const srt_pt_skin_joint* joints, uint32_t njoints, srt_pt_skin** skin);
/* Waits for the device, frees the skin.  NULL is fine. */
int srt_pt_skin_destroy(srt_pt_skin* skin);
/* out = {vertices, joints, influences in the map, triangles}. */
int srt_pt_skin_counts(srt_pt_skin* skin, uint32_t out[4]);
/* The map, copied back for inspection: offsets[nverts + 1]; joints[k] and weights[k] for k in [offsets[v], offsets[v + 1]) are
 * vertex v's influences.  cap: what joints / weights hold; below the influence count is SRT_ERR_INVALID. */
int srt_pt_skin_map(srt_pt_skin* skin, uint32_t* offsets, uint32_t* joints, float* weights, uint32_t cap);
/* skin.  posed: njoints * 16 host floats, Skeleton::joint_to_posed(j) in the joints' order, read before the call returns.  The host
 * forms M_j = posed_j * inverse_bind_j with Mat4::operator*'s loop (lib/mat4.h:136-147) and uploads 64 B per joint; one lane per
 * vertex sums w_ij * (M_j * pos) in list order (M * Vec3: v0 col0 + v1 col1 + v2 col2 + 1.0f col3, then project()); a vertex
 * with no joint keeps its bind position (:293).  flat_normals == 0: the normals are the bind normals (skin does not touch them);
 * != 0: those of sync_anim_mesh without smooth normals (:114-126) - a vertex gets cross(v1 - v0, v2 - v0).unit() of the LAST
 * triangle in index order that names it, its bind normal when none does.  The two outputs are device arrays of nverts * 3 floats.
 * Enqueues on `stream` (a hipStream_t; NULL: the null stream) and returns: no synchronisation.  Calls on one skin use one stream
 * at a time. */
int srt_pt_skin_vertices_device(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals, float* d_positions_out, float* d_normals_out);
/* The same into host arrays, through the skin's staging on the context's stream; waits. */
int srt_pt_skin_vertices(srt_pt_skin* skin, const float* posed, int flat_normals, float* positions_out, float* normals_out);
/* Skins into the skin's staging on `stream`, then srt_pt_update_mesh_device(pt, stream, object, staging, nverts): preconditions,
 * errors and "the committed scene stays as it was on failure" are exactly that call's for those arrays. */
int srt_pt_skin_pose(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);
/* The same with srt_pt_refit_mesh_device in place of the update: skin -> staging -> refit, no BVH<Triangle> build. */
int srt_pt_skin_pose_refit(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);
/* A RIG for the skin: the hierarchy and the joints' keys, so that a frame's matrices are computed on the device from one float.
 * What Skeleton::set_time (scene/skeleton.cpp:47-63) and Joint::joint_to_posed (student/skeleton.cpp:26-52) under
 * Skeleton::joint_to_posed (:106-115) do on the CPU per frame.  Joints are the skin's, in its order: parent[j] is -1 for a root or
 * the index of a joint in front of j (parents come first, as Skeleton::for_joints visits them); base is Skeleton::base_pos;
 * rest_pose holds 3 Euler angles (degrees) per joint - Joint::pose, which set_time leaves alone for a joint without keys;
 * knot_offsets has njoints + 1 entries from 0, joint j's keys being [knot_offsets[j], knot_offsets[j + 1]) of knot_times (strictly
 * ascending per joint, finite) and knot_quats (xyzw, 4 floats per key, not checked: the rig computes what the reference computes
 * from them).  Extents are those srt_pt_skin_create took.  SRT_ERR_INVALID: a NULL argument, a parent out of order, offsets that
 * do not start at 0 or descend, times that do not ascend strictly or are not finite; the skin keeps the rig it had.  Waits for the
 * device, then uploads the tables once (4 B + 12 B per joint, 12 B of base, the offsets, 20 B per key); a second call replaces
 * the rig. */
int srt_pt_skin_set_rig(srt_pt_skin* skin, const int32_t* parent, const float base[3], const float* rest_pose, const uint32_t* knot_offsets,
                        const float* knot_times, const float* knot_quats);
/* Skeleton::joint_to_posed(j) for every joint after Skeleton::set_time(t), njoints * 16 floats in Mat4::data order: a keyed joint's
 * pose is Spline<Quat>::at(t) (geometry/spline.inl:4-15: strict test before the first key, the last value from the last key on,
 * slerp of lib/quat.h:177-189 in between) through Quat::to_euler (lib/quat.h:124-135, lib/mat4.h:163-199); then from
 * iter = Mat4::euler(pose_j), for every ancestor from the parent to the root iter = translate(extent) * iter and iter = euler(pose) *
 * iter; translate(base) in front.  Bit-equal to the reference (x86-64, glibc 2.35's sinf / cosf / acosf / atan2f / hypotf restated;
 * the sin / cos restatement is valid below 6875 degrees).  The host form runs pt_anim.h compiled for the host - the definition the
 * kernels are held to - and touches no device.  The device form enqueues two kernels on `stream` (one lane per joint: the poses,
 * then each joint's own chain, in the reference's order) and returns.  SRT_ERR_STATE without a rig.  The host form only reads
 * the skin and may run next to other calls; the device forms here and below share the skin's per-joint scratch and its device
 * matrices with srt_pt_skin_vertices_device / srt_pt_skin_pose*: device-form calls on one skin use one stream at a time, and
 * srt_pt_skin_set_rig runs with none of them in flight on another thread. */
int srt_pt_skin_posed(srt_pt_skin* skin, float t, float* posed_out);
int srt_pt_skin_posed_device(srt_pt_skin* skin, void* stream, float t, float* d_posed_out);
/* srt_pt_skin_vertices_device, srt_pt_skin_pose and srt_pt_skin_pose_refit with the matrices of time t from the rig: the joint
 * kernels write M_j = joint_to_posed(j) * inverse_bind_j (Mat4::operator*'s loop) straight into the skin's device matrices, the
 * skinning kernels read them behind on the same stream.  Nothing is read from host memory and nothing goes up; waits, refusals
 * and "the committed scene stays as it was on failure" are those of the calls that take `posed`.  SRT_ERR_STATE without a rig. */
int srt_pt_skin_vertices_at_device(srt_pt_skin* skin, void* stream, float t, int flat_normals, float* d_positions_out, float* d_normals_out);
int srt_pt_skin_pose_at(srt_pt_skin* skin, void* stream, float t, int flat_normals);
int srt_pt_skin_pose_refit_at(srt_pt_skin* skin, void* stream, float t, int flat_normals);
/* srt_pt_skin_pose_refit and srt_pt_skin_pose_refit_at with srt_pt_refit_mesh_inplace_device in place of the refit: skin -> staging ->
 * both trees refitted, ENQUEUE-ONLY as that call is (it copies the staging, so the next pose may overwrite it at once).  With a rig
 * a frame is one float and uploads nothing; from `posed` it uploads 64 B per joint, through pinned staging of the skin's own (one
 * buffer per copy still on its way), so that copy too is only enqueued and `posed` is not read after the call returns. */
int srt_pt_skin_pose_inplace(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);
int srt_pt_skin_pose_inplace_at(srt_pt_skin* skin, void* stream, float t, int flat_normals);
/* ---- IK handles: Skeleton::do_ik / step_ik on the device ----
 * A skin with a rig keeps the CURRENT Joint::pose of every joint on the device (3 Euler angles in degrees per joint, the joints'
 * order), with a mirror on the host that an enqueue-only call leaves behind and the next host read settles.  srt_pt_skin_set_rig
 * sets it to the rest pose (and drops the handles: the hierarchy they were made for is gone).  The `_at(t)` calls above neither
 * read nor write it.  The calls below change it as the reference's Animate mode does - Skeleton::set_time, then Skeleton::do_ik -
 * and skin from it, so that targets -> IK -> skin -> refit -> render is one stream's work.
 *   The arithmetic is Skeleton::step_ik with Joint::compute_gradient (student/skeleton.cpp:117-191) operation for operation: exactly
 * 50 iterations with tau = 1 / 50.0f, and per joint the gradient summed from 0.0f over the enabled handles whose chain holds the
 * joint IN THE ORDER OF THE HANDLE LIST - that order is part of the result.  Results equal the reference's bit for bit while every
 * angle stays below the 6875 degrees of the sin / cos restatement (NaN beyond).  Targets and poses are not checked for NaN / Inf: the
 * rig computes what the reference computes.  Limits (SRT_ERR_UNSUPPORTED beyond): the skin's 4096 joints, and 1024 handles per skin.
 *
 * srt_pt_skin_set_ik_handles: the joints of the handles (indices into the skin's joints), in the order Skeleton::do_ik visits
 * them; n == 0 clears.  Builds, once per handle set, the per-joint lists of the handles whose chain holds the joint, and uploads
 * them with the list (waits).  SRT_ERR_STATE without a rig; SRT_ERR_INVALID for NULL or a joint out of range, SRT_ERR_UNSUPPORTED for
 * more than 1024 handles: the skin keeps the handles it had. */
int srt_pt_skin_set_ik_handles(srt_pt_skin* skin, const uint32_t* joints, uint32_t n);
/* Write and read the current pose: njoints * 3 host floats.  Both wait for the device; the read settles the mirror. */
int srt_pt_skin_set_joint_pose(srt_pt_skin* skin, const float* euler3);
int srt_pt_skin_joint_pose(srt_pt_skin* skin, float* euler3_out);
/* Skeleton::set_time(t) on the current pose (scene/skeleton.cpp:47-54), ENQUEUE-ONLY on `stream`: a joint with keys takes
 * anim.at(t).to_euler(); a joint without keys keeps its current pose - IK's changes included, as in the reference; it does not go
 * back to the rest pose.  (Handle keys, h->anim, stay with the caller: the reference's set_time only copies them into target /
 * enabled, which are arguments here.) */
int srt_pt_skin_set_time(srt_pt_skin* skin, void* stream, float t);
/* Skeleton::do_ik once: targets3 holds 3 floats per handle (IK_Handle::target, skeleton space - no base_pos), enabled one byte per
 * handle (nonzero: enabled; NULL: every handle).  With no handle enabled the poses keep their bits (do_ik returns before step_ik).
 * The host form uploads both, runs the kernel on the context's stream and waits.  SRT_ERR_STATE without a rig or without handles. */
int srt_pt_skin_step_ik(srt_pt_skin* skin, const float* targets3, const uint8_t* enabled);
/* The same with both arrays in device memory (d_enabled: srt_pt_set_active_device's byte convention; NULL: every handle),
 * ENQUEUE-ONLY under srt_pt_skin_pose_inplace's contract: one launch on `stream` does all 50 iterations; nothing is read from host
 * memory, nothing is uploaded, and there is no synchronisation. */
int srt_pt_skin_step_ik_device(srt_pt_skin* skin, void* stream, const float* d_targets3, const uint8_t* d_enabled);
/* Skeleton::joint_to_posed(j) (with base_pos) of every joint from the current pose: srt_pt_skin_posed / srt_pt_skin_posed_device
 * without a time.  The host form settles the mirror (waits) and computes on the host. */
int srt_pt_skin_posed_current(srt_pt_skin* skin, float* posed_out);
int srt_pt_skin_posed_current_device(srt_pt_skin* skin, void* stream, float* d_posed_out);
/* srt_pt_skin_vertices_at_device, and srt_pt_skin_pose_at / srt_pt_skin_pose_refit_at / srt_pt_skin_pose_inplace_at selected by `how`,
 * fed from the current pose instead of from time t: the same kernels, only the source of the Euler angles differs.  Waits,
 * refusals and counters are those of the `_at` call that `how` selects; SRT_ERR_INVALID for another `how`. */
#define SRT_PT_SKIN_UPDATE 0  /* srt_pt_update_mesh_device: the BVH<Triangle> rebuilt */
#define SRT_PT_SKIN_REFIT 1   /* srt_pt_refit_mesh_device */
#define SRT_PT_SKIN_INPLACE 2 /* srt_pt_refit_mesh_inplace_device: enqueue-only */
int srt_pt_skin_vertices_current_device(srt_pt_skin* skin, void* stream, int flat_normals, float* d_positions_out, float* d_normals_out);
int srt_pt_skin_pose_current(srt_pt_skin* skin, void* stream, int flat_normals, int how);
/* Every call on a skin but destroy and counts returns SRT_ERR_STATE once its context's scene was begun or committed again (the
 * skin is stale: destroy it, create another), and SRT_ERR_INVALID for a NULL argument. */
/* ---- Timelines: the Animate mode's keyframes evaluated on the device ----
 * What Scene_Object::set_time (scene/object.cpp:68-72) does on the CPU per frame and object: Anim_Pose::at(t) (scene/pose.cpp:54-57)
 * - Spline<Vec3>::at for position and scale as the fork wrote it (student/spline.inl:5-72: T() without knots, the end values at
 * and beyond the ends, a missing neighbour mirrored in time and value, tangents ((k2 - p0) / (t2 - t0)) * interval, the Hermite sum
 * left to right), Spline<Quat>::at for the rotation (geometry/spline.inl:4-15, slerp of lib/quat.h:177-189), Quat::to_euler
 * (lib/quat.h:124-135, lib/mat4.h:163-199) - and Pose::transform() = translate * euler * scale (scene/pose.cpp:4-10,
 * lib/mat4.h:382-418, Mat4::rotate's general-axis expressions as written).  The keys do not change between frames: they go up once,
 * and a frame sends one float.  Results equal the reference's bit for bit (x86-64, no contraction, glibc 2.35's sinf / cosf /
 * acosf / atan2f / hypotf restated; the sin / cos restatement is valid below 6875 degrees, which to_euler's angles never
 * reach); where the reference yields NaN (a zero quaternion) so do these, up to the NaN's sign and payload.
 * A timeline is bound to one context and its committed scene and goes stale as a skin does: every call but destroy returns
 * SRT_ERR_STATE once the scene was begun or committed again.  Destroy a context's timelines before the context. */
typedef struct srt_pt_timeline srt_pt_timeline; /* opaque */
/* `objects`: nobjects insertion indices under srt_pt_repose's rules (meshes, instances, spheres; an area light only under
 * srt_pt_set_dynamic_lights; no duplicate).  track_offsets has 3 * nobjects + 1 entries from 0: object k's position, rotation
 * and scale tracks are the knots [track_offsets[3 k + i], track_offsets[3 k + i + 1]) of knot_times and knot_values (4 floats per
 * knot: xyz_ for position and scale, xyzw for the rotation).  An empty track gives T(): a zero position, Quat(), a ZERO scale.
 * SRT_ERR_STATE: no committed scene.  SRT_ERR_INVALID: a NULL argument; srt_pt_repose's refusals with their messages; offsets that
 * do not start at 0 or descend; times of a track that do not ascend strictly or are not finite; an object whose three tracks are
 * all empty (Splines::any() is false for it: the reference would not move it).  Knot values are not checked: the scene computes
 * what the reference computes from them.  The scene is not touched.  Uploads the tables once (12 B per object, 20 B per knot). */
int srt_pt_timeline_create(srt_pt* pt, const uint32_t* objects, uint32_t nobjects, const uint32_t* track_offsets, const float* knot_times,
                           const float* knot_values, srt_pt_timeline** timeline);
/* Waits for the device, frees the timeline.  NULL is fine. */
int srt_pt_timeline_destroy(srt_pt_timeline* timeline);
/* trans_out[16 k ..] = Pose::transform() of object k's Anim_Pose::at(t), Mat4::data order.  The host form: pt_anim.h compiled for the
 * host, the definition the kernel is held to; works on a host-only context and touches no device. */
int srt_pt_timeline_transforms(srt_pt_timeline* timeline, float t, float* trans_out);
/* The same into a device array of nobjects * 16 floats: one kernel (one lane per object: three binary searches, the splines, the
 * Euler angles, the products) enqueued on `stream` (a hipStream_t; NULL: the null stream); no wait, nothing uploaded.  A host-only
 * context validates and then returns SRT_ERR_UNSUPPORTED. */
int srt_pt_timeline_transforms_device(srt_pt_timeline* timeline, void* stream, float t, float* d_trans_out);
/* The transforms of time t into the timeline's own device buffer, then srt_pt_repose_refit_device(pt, stream, the timeline's list,
 * that buffer): ENQUEUE-ONLY under that call's contract, with its first-call work, its ordering rules and the lagging host record.
 * In the steady state nothing is uploaded at all: the list repeats.  Calls on one timeline use one stream at a time. */
int srt_pt_timeline_repose_refit(srt_pt_timeline* timeline, void* stream, float t);
/* The same with srt_pt_repose_device, the rebuild: what a caller uses when srt_pt_scene_tree_cost says a refitted tree has
 * degraded.  Waits as that call waits. */
int srt_pt_timeline_repose(srt_pt_timeline* timeline, void* stream, float t);
/* ---- New shading values for a committed scene: materials, delta lights, the environment's radiance ----
 * What the reference changes per frame besides poses: Scene_Object::set_time's material.anim.at(time, material.opt)
 * (scene/object.cpp:71, Material::Anim_Material::at, scene/material.cpp:44-52) and Scene_Light::set_time (scene/light.cpp:30-38:
 * lanim.at(time, opt), Anim_Light::at :139-144, and pose = anim.at(time)).  The kernels read materials and delta lights at trace time;
 * trees, light lists, kernel forms and stack sizes depend only on a material's TYPE and on the NUMBER of lights, so new values need
 * no commit.  The three calls below follow srt_pt_repose's discipline: they settle a lagging host record first, validate everything
 * before the first write, run with nothing of the context in flight and wait as srt_pt_repose waits, upload only the listed records
 * (32 B per material, 160 B per light, counted in srt_pt_scene_counts) and work on a host-only context.  After a successful call the
 * scene computes, bit for bit, what a fresh commit with those values computes; after a refused one it is exactly what it was, on
 * both sides.  No count, tree, light-list entry, kernel form or stack size changes.  (The values srt_pt_add_material / srt_pt_add_light
 * collected stay what they were: a commit without a srt_pt_scene_begin builds from those, as it does after srt_pt_repose.)
 * SRT_ERR_STATE: no committed scene.  SRT_ERR_INVALID: a NULL argument, an index out of range, an index listed twice, and what each
 * call says below.
 *
 * materials[i]: indices srt_pt_add_material returned.  m[i].type must equal the committed type - the type decides area-light
 * membership, the instancing refusal and the elision proof - otherwise SRT_ERR_INVALID with a message naming both types.  Values are
 * taken as srt_pt_add_material takes them: a Lambertian `a` is divided by PI_F (rays/bsdf.h:26) as at a commit. */
int srt_pt_update_materials(srt_pt* pt, const uint32_t* materials, const srt_pt_material* m, uint32_t n);
/* lights[i]: the 0-based call order of srt_pt_add_light; the type stays.  radiance: 3 floats per light, angle_bounds: 2 per light
 * (may be NULL when no listed light is a spot light), trans: 16 per light.  Each record is what srt_pt_add_light makes of the new
 * values (Delta_Light, rays/light.h:57-96): itrans = Mat4::inverse(trans), has_trans = trans != Mat4::I. */
int srt_pt_update_lights(srt_pt* pt, const uint32_t* lights, const float* radiance, const float* angle_bounds, const float* trans, uint32_t n);
/* A new radiance for an SRT_ENV_SPHERE / SRT_ENV_HEMISPHERE environment light; SRT_ERR_INVALID for SRT_ENV_NONE / SRT_ENV_MAP.  The
 * radiance is a launch parameter, like the camera: it is stored, nothing is uploaded or waited for, and it takes effect at the next launch. */
int srt_pt_update_env_light(srt_pt* pt, const float radiance[3]);

/* ---- Shading timelines: the Animate mode's material and light keys, evaluated on the device ----
 * The keys of listed materials and delta lights (and of the environment light) as srt_pt_timeline_create takes an object's: a CSR of
 * knots, 4 floats per knot.  Tracks, in order: per material six - albedo, reflectance, transmittance, emissive (xyz_), intensity,
 * ior (x___), the order of Anim_Material::at's tuple (scene/material.cpp:44-52); then per light six - spectrum (xyz_), intensity
 * (x___), angle_bounds (xy__) (Anim_Light::at, scene/light.cpp:139-144), then the Anim_Pose triple position / rotation (xyzw) /
 * scale; then, with env != 0, two - spectrum and intensity of the environment light.  track_offsets has one entry per track plus one,
 * from 0.
 *   Semantics are the reference's.  Spline<Spectrum>, Spline<Vec2> and Spline<float> are the fork's Spline<T>::at
 * (student/spline.inl:5-72) channel by channel (lib/spectrum.h:84-102,136-138, lib/vec2.h:83-107,175-177).  A material takes all six
 * options from at(t): an empty track gives T() - a zero Spectrum, a 0.0f intensity or ior (geometry/spline.h:99-101) - so emissive
 * keys without an intensity key give a black light, as in the reference.  A light's option triple and its pose triple are
 * independent (Scene_Light::set_time, scene/light.cpp:30-38): a triple without a key leaves the scene's values in place.  From the
 * options the record is what Pathtracer::build_scene / build_lights make (rays/pathtracer.cpp:26-64,93-117), by committed type:
 * Lambertian a = albedo.to_linear() / PI_F (Spectrum::to_linear, lib/spectrum.h:54-60, both branches); Mirror a = reflectance; Glass
 * a = transmittance, b = reflectance, ior; Refract a = transmittance, ior; Diffuse light a = emissive * intensity
 * (Material::emissive, scene/material.cpp:34-36); a light's radiance = spectrum * intensity (scene/light.cpp:98-100), angle_bounds,
 * trans = Pose::transform() of Anim_Pose::at(t), itrans, has_trans.  Fields a material type does not read are written as zeros.
 *   to_linear: the host form uses libm's powf, as the reference does; the kernel uses the SRT-MATH restatement of glibc 2.35's powf,
 * whose argument (f + 0.055f) / 1.055f with f > 0.04045f is a positive normal number for every finite albedo.  A non-finite albedo
 * channel yields the same on both sides: NaN stays NaN and -inf stays -inf (the f / 12.92f branch), +inf gives +inf (the kernel
 * answers it before its powf, which takes normal arguments only).
 * SRT_ERR_STATE: no committed scene.  SRT_ERR_INVALID: a NULL argument (materials / lights may be NULL where their count is 0);
 * nothing listed; an index out of range or listed twice; env != 0 without a sphere / hemisphere environment light; the refusals of
 * srt_pt_timeline_create about offsets and times, with its messages; a material whose six tracks are all empty, a light whose two
 * triples are both empty, an environment whose two tracks are empty (Splines::any() is false).  Knot values are not checked.  The
 * scene is not touched.  Uploads the tables once.  A shading timeline goes stale as a timeline does (SRT_ERR_STATE from every call
 * but destroy once the scene was begun or committed again) and is destroyed before its context. */
typedef struct srt_pt_shading_timeline srt_pt_shading_timeline; /* opaque */
int srt_pt_shading_timeline_create(srt_pt* pt, const uint32_t* materials, uint32_t nmaterials, const uint32_t* lights, uint32_t nlights, int env,
                                   const uint32_t* track_offsets, const float* knot_times, const float* knot_values, srt_pt_shading_timeline** out);
/* Waits for the device, frees the timeline.  NULL is fine. */
int srt_pt_shading_timeline_destroy(srt_pt_shading_timeline* timeline);
/* The host form: the functions of pt_anim.h compiled for the host, the definition the kernel is held to.  materials_out[k]: material
 * k of the list as srt_pt_update_materials takes it (a Lambertian `a` is albedo.to_linear(), not yet divided); lights_out: 21 floats
 * per light - radiance3, angle_bounds2, trans16, a triple without a key giving the scene's values; env_out: the environment's
 * radiance.  An array may be NULL where the timeline lists nothing for it.  Launches nothing and works on a host-only context (a
 * lagging host record is settled first: the values a light keeps are read from it). */
int srt_pt_shading_timeline_values(srt_pt_shading_timeline* timeline, float t, srt_pt_material* materials_out, float* lights_out, float env_out[3]);
/* The values of time t through srt_pt_update_materials, srt_pt_update_lights and srt_pt_update_env_light: the host form of apply. */
int srt_pt_shading_timeline_update(srt_pt_shading_timeline* timeline, float t);
/* The device form, ENQUEUE-ONLY: validates on the host and enqueues one kernel on `stream` (a hipStream_t; NULL: the null stream) -
 * one lane per item, materials first, then lights - which writes the listed records of the live material and delta-light tables in
 * place.  No synchronisation, no read-back, and in the steady state nothing uploaded: the tables went up at create.  A light's
 * itrans / has_trans come from the arithmetic srt_pt_repose_device gives an object's.  The environment's three floats are one item
 * and no scene memory: they are evaluated on the host inside the call, by the same function of pt_anim.h a kernel would run, and
 * stored as the launch parameter.  Results equal the host form's bit for bit.
 *   Ordering is srt_pt_repose_refit_device's: the new values are visible to whatever is enqueued on `stream` behind the call; epochs
 * on other streams are ordered by the caller with events.  The host's record LAGS after the call and settles under that call's rule:
 * every entry point that is not enqueue-only waits for an event recorded behind the last apply and reads the material and / or
 * delta-light table back once (32 B / 160 B per record).  While the material record lags, srt_pt_set_elision's proof is not
 * attempted: the image is bit-identical either way, only the cost differs, and srt_pt_rays_elided shows it.  A host-only context
 * validates and returns SRT_ERR_UNSUPPORTED.  A HIP error is SRT_ERR_HIP and leaves the context without a committed scene. */
int srt_pt_shading_timeline_apply(srt_pt_shading_timeline* timeline, void* stream, float t);
/* Where srt_pt_scene_commit runs BVH<Primitive>::build (student/bvh.inl:35-163): device != 0 (default) builds primitive sets of at
 * least min_primitives (default 16384) on the GPU, smaller ones and device == 0 on the host.  Both produce the reference's node
 * arrays and primitive order bit for bit (the candidate planes' std::partition sequence included); SRT_BVH_BUILDER=host in the
 * environment forces the host build. */
int srt_pt_set_bvh_builder(srt_pt* pt, int device, uint32_t min_primitives);
/* The streamed forms (kernel modes 6 / 7, what auto takes for scenes with a real BVH<Triangle> or many objects) keep this many
 * paths in flight per launch (rounded up to 256; 0 = the default, 3 Mi; at most 2^26, SRT_ERR_INVALID beyond; ~1 KB of device
 * memory per slot).  The image does not depend on it. */
int srt_pt_set_stream_slots(srt_pt* pt, uint32_t slots);

int srt_pt_set_camera(srt_pt* pt, const float iview[16], float vert_fov_deg, float aspect_ratio);
/* Image size and Pathtracer::max_depth.  Limits (SRT_ERR_UNSUPPORTED beyond): width, height <= 65535, width * height < 2^31,
 * max_depth <= 16. */
int srt_pt_set_params(srt_pt* pt, uint32_t width, uint32_t height, uint32_t max_depth);

/* ---- image-tile sharding (one process per GPU) ---------------------------------------------------
 * The image is cut into tile_w x tile_h tiles numbered row-major; rank r of `world` renders the tiles
 * t with t % world == r.  Defaults: 32 x 32, rank 0, world 1. */
int srt_pt_set_tiling(srt_pt* pt, uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t world);
/* Number of tiles this rank renders / the per-rank capacity every rank pads to (ceil(ntiles / world)),
 * and floats per tile (tile_w * tile_h * 3). */
int srt_pt_tile_info(srt_pt* pt, uint32_t* local_tiles, uint32_t* tiles_per_rank, uint32_t* floats_per_tile);

/* ---- do_trace ------------------------------------------------------------------------------------
 * One epoch: for every pixel of this rank's tiles, the mean over the VALID samples
 * sample_base .. sample_base + samples - 1 of trace_pixel (invalid = non-finite, dropped as in
 * rays/pathtracer.cpp:219-222).
 * Host form: rgb_out is a full width*height*3 float image (row 0 = bottom); only this rank's pixels are
 * written.  Synchronous. */
int srt_pt_render_epoch(srt_pt* pt, uint64_t seed, uint32_t sample_base, uint32_t samples, float* rgb_out);
/* Device form: d_tiles_out is DEVICE memory of tiles_per_rank * floats_per_tile floats, tile-major
 * (local tile k = global tile rank + k * world); enqueued on `stream` (hipStream_t; NULL = the HIP
 * default stream, which is also PyTorch's default), not synchronized.  This is the buffer the RCCL gather moves. */
int srt_pt_render_epoch_device(srt_pt* pt, void* stream, uint64_t seed, uint32_t sample_base, uint32_t samples,
                               float* d_tiles_out);
/* d_gathered: DEVICE, world * tiles_per_rank * floats_per_tile floats as gathered on the root (rank-major).
 * Scatters the tiles into the width*height*3 DEVICE image d_image (row 0 = bottom). */
int srt_pt_untile_device(srt_pt* pt, void* stream, const float* d_gathered, float* d_image);
/* Pathtracer::accumulate on DEVICE buffers of nfloats: acc += (epoch - acc) * (1.0f / accumulator_samples). */
int srt_pt_accumulate_device(srt_pt* pt, void* stream, float* d_accumulator, const float* d_epoch, size_t nfloats,
                             uint32_t accumulator_samples);

/* ---- launches decoupled from the reference's epochs (what the drop-in class renders with) -------------------------------
 * Pathtracer::begin_render cuts a render into epochs of samples_per_epoch = max(1, n / (hardware_concurrency * 10)) samples
 * (rays/pathtracer.cpp:250-256) - one sample per epoch for a 256-spp render on a 32-thread host - and the image is the running
 * mean of the epoch means in epoch order (:195-207), so the epoch size is part of the result.  A GPU launch wants tens of samples
 * per pixel.  These entry points keep both: srt_pt_render_samples_device renders ONE launch of up to
 * srt_pt_max_samples_per_launch samples per pixel of this rank's tiles and leaves every sample's radiance in the stream's
 * sample buffer; srt_pt_fold_epochs_device then replays do_trace's and accumulate's arithmetic over that buffer, epoch by epoch
 * and sample by sample in order - epoch mean = (sum of the valid samples) * (1.0f / count), accumulator += (mean - accumulator) *
 * (1.0f / k) - into the rank's accumulator: bit-identical to one srt_pt_render_epoch + srt_pt_accumulate_device per epoch.
 *   d_accumulator   DEVICE, srt_pt_accumulator_floats floats (per pixel slot: the running mean, and the epoch in progress so that
 *                   an epoch may span launches), zeroed by the caller before a render that does not add samples
 *   position        samples of this render folded before this launch;  total_samples: of the whole render (its last epoch may
 *                   be short);  accumulator_samples: epochs the accumulator held before the render (Add Samples continues it).
 *                   A fold at position 0 starts with an empty epoch in progress: whatever partial epoch an earlier render left in
 *                   d_accumulator (one that was cancelled, or whose launches ended off an epoch boundary) is discarded, as the
 *                   reference drops a cancelled epoch; only the running mean carries over into an Add Samples render
 * The fold goes on the same stream as the launch it folds (it reads that stream's sample buffer) and is skipped when the
 * launch was cancelled.  Launches on two streams overlap; their folds must be ordered by the caller (events).
 * srt_pt_accumulator_tiles_device writes the running mean in the tile layout of srt_pt_render_epoch_device (gather, un-tile). */
int srt_pt_max_samples_per_launch(srt_pt* pt, uint32_t* samples);
int srt_pt_accumulator_floats(srt_pt* pt, size_t* nfloats);
int srt_pt_render_samples_device(srt_pt* pt, void* stream, uint64_t seed, uint32_t sample_base, uint32_t samples);
int srt_pt_fold_epochs_device(srt_pt* pt, void* stream, uint32_t samples_per_epoch, uint32_t position, uint32_t total_samples,
                              uint32_t accumulator_samples, float* d_accumulator);
int srt_pt_accumulator_tiles_device(srt_pt* pt, void* stream, const float* d_accumulator, float* d_tiles_out);

/* ---- cancel (Pathtracer::cancel, rays/pathtracer.cpp:282-290) ------------------------------------------------------
 * The reference's do_trace tests cancel_flag after every sample (rays/pathtracer.cpp:224) and drops the epoch.  srt_pt_cancel
 * raises a flag in pinned host memory that the kernels watch: a persistent launch stops handing out work units (one of its
 * waves looks at the flag whenever it fetches work and then drains the unit queue for all the others), the streamed forms end
 * at the next generation, and every launch of the epoch still enqueued returns at its first instruction - an epoch of 2048
 * samples per pixel ends within a few milliseconds.  It is the ONE call that may be made from another host thread while a
 * render call is running (it does nothing but store the flag).  From then on srt_pt_render_epoch returns SRT_CANCELLED (1, not
 * an error; its output is not written) and srt_pt_render_epoch_device enqueues nothing and returns the same; epochs of the
 * *_device forms that were in flight leave unspecified tiles - the caller drops them, as the reference drops its partial
 * epoch.  srt_pt_clear_cancel waits for the device and lowers the flag (before the next render). */
int srt_pt_cancel(srt_pt* pt);
int srt_pt_cancel_requested(srt_pt* pt);   /* 1 while the flag is raised */
int srt_pt_clear_cancel(srt_pt* pt);

/* ---- log_ray (Pathtracer::log_ray -> Gui::Widget_Render::log_ray, gui/widgets.cpp:625-628) ----------------------------
 * sample_direct_lighting flips RNG::coin_flip(0.0005f) at every shading point of a continuous BSDF and, when it comes up,
 * logs the ray it is about to trace toward the light / along the BSDF sample: log_ray(world_ray_task6, 5.0f)
 * (student/pathtracer.cpp:146-148; the GUI draws point .. point + t * dir in white).  The kernels always draw the coin (the RNG
 * ledger needs it); with a ring of `capacity` > 0 rays per stream they also record the selected rays, and srt_pt_read_ray_log
 * hands them to the host - the drop-in class replays them into gui.log_ray after every epoch.  Rays beyond the capacity
 * between two reads are counted in *dropped.  Order: pixel (y * width + x), then sample, then bounce - the order a
 * single-threaded do_trace logs them in.  srt_pt_read_ray_log waits for the device and reads every stream's ring;
 * the _stream form waits for `stream` only and reads the ring of the epochs rendered on it.  out may be NULL: *n_out is then
 * the number of rays waiting, and they stay; otherwise the rings are emptied, and what `cap` does not take counts as dropped. */
int srt_pt_set_ray_log(srt_pt* pt, uint32_t capacity);   /* 0 (default): nothing is recorded */
int srt_pt_read_ray_log(srt_pt* pt, srt_pt_logged_ray* out, size_t cap, size_t* n_out, uint64_t* dropped);
int srt_pt_read_ray_log_stream(srt_pt* pt, void* stream, srt_pt_logged_ray* out, size_t cap, size_t* n_out, uint64_t* dropped);

/* ---- the normal-colors debug view (debug_data.normal_colors, student/debug.h; "Pathtracer: use normal colors",
 * student/debug.cpp:43) ---------------------------------------------------------------------------------------------------
 * With the box ticked Pathtracer::trace returns {Spectrum::direction(result.normal), {}} right after scene.hit
 * (student/pathtracer.cpp:199): a render is a first-hit view.  on != 0 reproduces it bit for bit.  A sample draws the two
 * numbers of Rect(1,1).sample() (student/pathtracer.cpp:29-30), builds the camera ray and calls scene.hit ONCE: 2 RNG draws, 1
 * ray, and the ray-log coin of :148 is never reached, so a ray log of any capacity stays empty.  A miss is
 * env_light.evaluate(ray.dir) or zero, as in any render (:182-188).  A hit is Spectrum::direction(normal) (lib/spectrum.h:47-52:
 * Vec3::normalize, lib/vec3.h:141-147, then absolute values; the to_linear() of :50 discards its result, so no sRGB curve is
 * applied) BEFORE the emissive test: light sources show their normals too.  The normal is Trace::normal as Object::hit returns
 * it - interpolated vertex normals for meshes, not unit length in general; a zero normal gives NaN in every channel and the
 * sample is dropped as do_trace drops invalid samples (rays/pathtracer.cpp:219-222).
 * While it is on, srt_pt_render_epoch[_device], srt_pt_render_samples_device (+ srt_pt_fold_epochs_device; under kernel mode 1
 * as well, this kernel always keeps per-sample radiance), srt_pt_trace_samples and the group forms take one first-hit kernel
 * (one lane per pixel and sample, no path state) for every scene srt_pt_scene_commit accepts, whatever srt_pt_set_kernel says;
 * tiling, streams, cancel, srt_pt_sync and srt_pt_kernel_time behave as for any other form, srt_pt_ray_count counts one ray per
 * camera sample and srt_pt_rays_elided stays 0.  srt_pt_hit, the particle step, tone mapping and the BVH dumps do not look at it.
 * The reference reads its global on every trace call; here the switch is read when a launch is enqueued: a change takes effect
 * at the next launch.  It needs no re-commit and may be called whenever nothing of the context is being enqueued (the rule of
 * srt_pt_set_elision).  Default: off - every output is what it was without the switch. */
int srt_pt_set_normal_colors(srt_pt* pt, int on);

/* Rays (scene.hit calls) and camera samples traced by this context since the last reset. */
int srt_pt_ray_count(srt_pt* pt, uint64_t* rays, uint64_t* camera_samples, int reset);

/* ---- parity / inspection -------------------------------------------------------------------------- */
/* Dead-ray elision.  In sample_direct_lighting the reference adds the term of the BSDF-sampled
 * direct ray and subtracts it again (student/pathtracer.cpp:118-125): without delta / environment lights the ray cannot
 * change the result of a Lambertian bounce (its random draws are still consumed).  on != 0 lets the kernels skip tracing
 * it where that is provable - no delta or environment light, every continuous BSDF Lambertian: the wave-uniform kernel
 * then runs two-ray batches, the per-lane kernels skip the call; other scenes (and the flattened-walk and stamped
 * diagnostic builds) ignore the switch.  The image is bit-identical either way.
 * srt_pt_ray_count keeps counting the rays the REFERENCE issues; srt_pt_rays_elided reports how many of them were not
 * traced.  Default: off (every ray traced). */
int srt_pt_set_elision(srt_pt* pt, int on);
int srt_pt_rays_elided(srt_pt* pt, uint64_t* elided, int reset);

/* trace_pixel for explicit (x, y, sample) triples (host arrays of n).  rgb_out: 3 floats per sample;
 * draws_out / rays_out (nullable): RNG draws and scene.hit calls of that sample. */
int srt_pt_trace_samples(srt_pt* pt, uint64_t seed, const uint32_t* xs, const uint32_t* ys, const uint32_t* ss,
                         size_t n, float* rgb_out, uint32_t* draws_out, uint32_t* rays_out);
/* scene.hit for explicit rays.  out9: {hit, distance, position[3], normal[3], material} per ray (Trace).  Directions need
 * not be normalised (the particle step passes velocities): times, distances and dist_bounds follow lib/ray.h and
 * student/bvh.inl exactly as the reference scales them. */
int srt_pt_hit(srt_pt* pt, const float* origins, const float* dirs, const float* bounds, size_t n, float* out9);
/* The same for rays that lie in device memory, results into device memory, ENQUEUE-ONLY under the contract written at
 * srt_pt_repose_refit_device: the host validates first, then the call only enqueues on `stream` (NULL = the HIP default stream) and
 * returns - no synchronisation, nothing copied to the host.  d_origins / d_dirs: 3 floats per ray; d_bounds: 2 per ray as
 * srt_pt_hit's bounds, NULL = {0, +inf} for every ray.  Each output may be NULL, not all three:
 *   d_out9  srt_pt_hit's record bit for bit: {hit, distance, position[3], normal[3], material}, nine zeros on a miss;
 *   d_ids   two words per ray: the 0-based insertion index of the object hit, then the triangle's place in that object's own
 *           BVH<Triangle> primitive order (the index into srt_pt_dump_bvh's `order` of the object; the index order in a scene
 *           committed without BVHs; an instance reports its OWN insertion index and the shared mesh's place).  A sphere gives
 *           0xFFFFFFFF as the second word, a miss 0xFFFFFFFF for both;
 *   d_hit   one byte per ray: 1 when a closest hit exists within the bounds, else 0 - the shadow-ray question (it is the closest-hit
 *           walk all the same: there is no early exit).  Asked alone, no surface is computed and one byte per ray is written.
 * It reads the LIVE device scene - every enqueue-only update enqueued on `stream` before it is seen (srt_pt_repose_refit_device,
 * srt_pt_set_active_device, the skin poses, srt_pt_shading_timeline_apply; other streams: the caller's events) - and does not
 * settle the host's record.  It ignores srt_pt_cancel and leaves srt_pt_ray_count and the timing brackets alone.
 *   Routing: a scene srt_pt_set_kernel(6) would render (a BVH<Object> on top, hits that pack into one word, a traversal stack that
 * fits) goes through the persistent ray-cast kernel of the streamed forms: pack (32-byte requests), cast, resolve - 44 B of scratch
 * per ray, one set per stream, grown on demand (growth waits, once); a call of more than 4 Mi rays is cut into chunks enqueued back
 * to back (SRT_HIT_CHUNK overrides the chunk: a diagnostic).  Every other scene and kernel modes 1 and 4 take srt_pt_hit's
 * per-lane walk straight from the caller's arrays; mode 5 the flattened walk (1..31 objects, refused otherwise).  The automatic
 * mode follows the measurement: it takes the ray-cast kernel for calls of at least 2^19 rays - the crossover for
 * incoherent rays; a persistent launch has a fixed cost - on the scenes whose render it streams as well (a mesh with a real
 * BVH<Triangle>, or more than 16 objects), and the per-lane walk otherwise: on a Cornell box of single-leaf meshes that walk is
 * ahead at every size.  Modes 2, 3, 6 and 7 take the ray-cast kernel wherever it applies.  The results are identical on every route.
 *   SRT_ERR_INVALID: NULL pt, NULL origins or directions with n > 0, no output at all.  SRT_ERR_STATE: no committed scene.
 * SRT_ERR_UNSUPPORTED: n > 0x7fffffff; a host-only context.  n == 0 enqueues nothing.  A ray with a NaN component or an all-zero
 * direction terminates with an unspecified result (the caveat of srt_pt_set_active). */
int srt_pt_hit_device(srt_pt* pt, void* stream, const float* d_origins, const float* d_dirs, const float* d_bounds, size_t n,
                      float* d_out9, uint32_t* d_ids, uint8_t* d_hit);
/* Scene_Particles::Particle::update (student/particles.cpp:5-59) for n particles against the committed scene - the loop body of
 * Scene_Particles::step2 (scene/particles.cpp:134-138), the second caller of Object::hit besides the path tracer (the scene
 * it collides with is Simulate::build_scene's BVH<Object>, gui/simulate.cpp:69-99: commit the same objects).  pos / vel: 3
 * floats per particle, age: 1, updated in place; alive[k] = update()'s return value (age > 0).  dt is one simulation step
 * (Options::dt), radius the particle radius times Options::scale.  Spawning and removing particles are srt_pt_emitter's (below).
 * The reference's loop never returns when its hit_time stays <= 0; the kernel gives such a particle up after 4096 legs.
 * Host form: synchronous.  Device form: device pointers, enqueued on `stream` (NULL = the HIP default stream). */
int srt_pt_particles_step(srt_pt* pt, float* pos, float* vel, float* age, size_t n, float dt, float radius, uint8_t* alive);
int srt_pt_particles_step_device(srt_pt* pt, void* stream, float* d_pos, float* d_vel, float* d_age, size_t n, float dt, float radius,
                                 uint8_t* d_alive);

/* ---- srt_pt_emitter: the whole Scene_Particles::step (scene/particles.cpp:101-162) for a pool of fixed capacity ----
 * The `enabled` and `opt.dt < EPS_F` exits, the `last_update` substep loop, step2 - update, deaths, the cooldown loop, the spawn
 * arithmetic - and gen_instances, bit-equal to the reference's own code, on one stream without a host wait.
 *   The pool: `objects` are `capacity` objects of `render`'s committed scene (insertion indices), one per slot, validated exactly
 * as srt_pt_set_active validates its list - the same refusals, the same codes.  The emitter owns pos / vel (3 floats per slot), age
 * (1), alive (1 byte) and birth (a uint32: the birth ordinal of the particle in the slot) on the device; every slot starts dead.
 * `radius` is Scene_Particles::radius; the step uses radius * scale as the reference does.
 *   The collide context: `collide` is the context whose committed scene the particles bounce off, on the same device.  The
 * reference collides with Simulate::build_scene's scene of Scene_Objects only (gui/simulate.cpp:69-99); a collide context that
 * holds those objects and nothing else is what makes the step the reference's.  collide == render is allowed and gives the pool
 * loop of srt_pt_set_active_device: the particles then also bounce off each other's active meshes, which the reference never does.
 *   The schedule is the host's, exactly: last_update (float) and particle_cooldown (double) depend on the dts and the options
 * only, so the host mirrors them with the reference's types and expressions (`particle_cooldown -= dt` is a double minus a float,
 * `cooldown = 1.0 / opt.pps` is computed in double, the comparison is `<= 0.0f`) and knows every substep's spawn count without
 * reading the device.  The reference's loops are unbounded; one call is bounded by 4096 substeps and by 1048576 spawns per
 * substep, and a call beyond either is refused with SRT_ERR_UNSUPPORTED before anything is enqueued, the schedule unchanged.
 *   Per substep, on the stream, two launches: Particle::update for the ALIVE slots only against collide's scene (a dead slot is
 * neither traced nor written; 4096 legs at most, as srt_pt_particles_step); then the spawns: the k-th spawn of the substep goes to
 * the k-th dead slot in ascending slot index, counted after that substep's deaths - a slot that died in this substep can be reused
 * in it.  Spawns beyond the dead slots are dropped and counted; birth ordinals and uniforms advance as if they had spawned, so the
 * stream of uniforms stays aligned with the reference's.
 *   Uniforms: the spawn with birth ordinal b consumes two, the z one first, then the angle one.  With a buffer set
 * (srt_pt_emitter_set_uniforms_device: n floats on the device, kept by the caller) they are d_uniforms[2 b] and d_uniforms[2 b + 1];
 * a step whose last ordinal lies beyond the buffer is refused with SRT_ERR_INVALID before anything is enqueued.  Without one they are
 * the first two draws of SRT-RNG v1 keyed (seed, emitter key, b) - the emitter key is objects[0] - with unit() as DESIGN.md
 * section 4 defines it.
 *   Order: the reference keeps survivors in order and appends births, so its vector is always sorted by birth; the pool's alive
 * slots sorted by `birth` equal that vector bit for bit (pos, velocity, age).  The slot order itself is the pool's own.
 *   Deviations from the reference: the fixed capacity with a drop counter, the slot order, and the 4096-leg cap of the step.
 * Anim_Particles / Anim_Pose keys of the emitter stay with the caller (srt_pt_emitter_set_options / _set_pose per frame); the
 * particle colour is the pool objects' material.
 *   A handle is stale once `render`'s scene is begun or committed again (SRT_ERR_STATE); `collide` must hold a committed scene
 * whenever a step runs.  Destroy the emitter before either context.  On a host-only `render` (device -1) the emitter validates
 * and keeps the schedule; everything that touches the pool returns SRT_ERR_UNSUPPORTED. */
typedef struct srt_pt_emitter srt_pt_emitter; /* opaque */
int srt_pt_emitter_create(srt_pt* render, srt_pt* collide, const uint32_t* objects, uint32_t capacity, float radius, srt_pt_emitter** out);
int srt_pt_emitter_destroy(srt_pt_emitter* em);
/* Scene_Particles::Options without name and colour; the defaults are the reference's: velocity 25, angle 0, scale 0.1, lifetime 15,
 * pps 5, dt 0.01, enabled 0.  Nothing is uploaded: the values are launch parameters. */
int srt_pt_emitter_set_options(srt_pt_emitter* em, float velocity, float angle, float scale, float lifetime, float pps, float dt, int enabled);
/* Scene_Particles::pose: pos3 and euler3 (degrees), stored like the camera, nothing uploaded.  Starts as Pose::id(). */
int srt_pt_emitter_set_pose(srt_pt_emitter* em, const float* pos3, const float* euler3);
int srt_pt_emitter_seed(srt_pt_emitter* em, uint64_t seed);
/* d_uniforms NULL or n 0: back to the seeded generator. */
int srt_pt_emitter_set_uniforms_device(srt_pt_emitter* em, const float* d_uniforms, size_t n);
/* Scene_Particles::step(scene, dt) without gen_instances.  _device: only enqueues on `stream` - no synchronisation, no read-back,
 * no upload; a disabled emitter enqueues srt_pt_emitter_clear_device.  The blocking form runs on render's own stream and waits. */
int srt_pt_emitter_step_device(srt_pt_emitter* em, void* stream, float dt);
int srt_pt_emitter_step(srt_pt_emitter* em, float dt);
/* gen_instances: srt_pt_particle_transforms_device(pos, scale) into the emitter's own matrices, srt_pt_set_active_device(alive) and
 * srt_pt_repose_refit_device on `render`, under their contracts - what they upload and where they block is all this call does. */
int srt_pt_emitter_present_device(srt_pt_emitter* em, void* stream);
/* step + present */
int srt_pt_emitter_frame_device(srt_pt_emitter* em, void* stream, float dt);
/* Scene_Particles::clear(): every slot becomes dead; last_update and particle_cooldown stay, as in the reference. */
int srt_pt_emitter_clear_device(srt_pt_emitter* em, void* stream);
int srt_pt_emitter_clear(srt_pt_emitter* em);
/* The five arrays, blocking (the device is idle when they return); a NULL array is skipped.  pos / vel: capacity * 3 floats, age:
 * capacity floats, alive: capacity bytes, birth: capacity uint32.  For seeding a pool, saving and restoring it, and tests. */
int srt_pt_emitter_read(srt_pt_emitter* em, float* pos, float* vel, float* age, uint8_t* alive, uint32_t* birth);
int srt_pt_emitter_write(srt_pt_emitter* em, const float* pos, const float* vel, const float* age, const uint8_t* alive, const uint32_t* birth);
/* out[0] = alive slots, out[1] = birth ordinals consumed so far (dropped spawns included), out[2] = spawns dropped.  Blocking.  On a
 * host-only context out[0] and out[2] are 0. */
int srt_pt_emitter_counts(srt_pt_emitter* em, uint64_t out[3]);
/* The device pointers {pos, vel, age, alive, birth}, for callers with kernels of their own. */
int srt_pt_emitter_arrays_device(srt_pt_emitter* em, void* out[5]);

/* Host-side BVH arrays after commit.  which = -1: the BVH<Object> (order = 1-based insertion index of the
 * objects in BVH primitive order); which >= 0: the BVH<Triangle> of the which-th BVH<Object> primitive
 * (order = first vertex index of each triangle in BVH primitive order).  boxes: 6 floats per node,
 * links: {start, size, l, r} per node.  Returns the node count or a negative status. */
long srt_pt_dump_bvh(srt_pt* pt, int which, float* boxes, uint32_t* links, size_t cap, uint32_t* order);
/* Tone mapping for display: HDR_Image::tonemap_to (util/hdr_image.cpp:161-187) with Spectrum::to_srgb
 * (lib/spectrum.h:61-75).  rgb: height*width*3 floats, row 0 first (the accumulated radiance, as srt_pt_render_epoch
 * returns it); rgba_out: height*width*4 bytes, rows flipped as the reference flips them for display, per channel
 * (unsigned char)round(to_srgb(1 - exp(-c * exposure)) * 255), alpha 255.  exposure must be positive (the reference
 * substitutes the image's own exposure for e <= 0; the caller passes that value).  Bit-identical to the reference built
 * against glibc 2.35 on an x86-64 host with FMA.  The _device form takes device pointers (rgba 4-byte aligned) and
 * enqueues on `stream` exactly as the other *_device calls do (hipStream_t; NULL = the HIP default stream) without
 * synchronising: a tone map enqueued behind srt_pt_accumulate_device on the same stream sees that accumulate's result. */
int srt_pt_tonemap(srt_pt* pt, const float* rgb, uint32_t width, uint32_t height, float exposure, uint8_t* rgba_out);
int srt_pt_tonemap_device(srt_pt* pt, void* stream, const float* d_rgb, uint32_t width, uint32_t height, float exposure,
                          uint8_t* d_rgba);

/* (Kernel selection, timing brackets, traversal counters and the device math probes: include/srt_pt_debug.h.) */

/* Waits for the context's own stream.  Like srt_pt_render_epoch and srt_pt_ray_count it returns SRT_ERR_STATE (once) when a
 * streamed launch since the last such call ended with unfinished work units - the epoch image of that launch is invalid. */
int srt_pt_sync(srt_pt* pt);

#ifdef __cplusplus
}
#endif
#endif /* SRT_PT_H */
