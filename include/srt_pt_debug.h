/*
 * srt_pt_debug.h - diagnostic and test entry points of the path-tracer library (libsrt_hip.so).  NOT part of the drop-in
 * boundary (include/srt_pt.h): nothing here is needed to render; the parity tests, bench.py and the profiling tools use them.
 *
 *   kernel selection / timing brackets / counters of the forms that implement Pathtracer::do_trace
 *   (rays/pathtracer.cpp:209-231; student/pathtracer.cpp:14-218, student/bvh.inl:166-276), and the device's restatements of the
 *   libm functions the reference's arithmetic goes through (glibc 2.35), evaluated for host arrays.
 */
#ifndef SRT_PT_DEBUG_H
#define SRT_PT_DEBUG_H

#include "srt_pt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel selection for render_epoch*: 0 = automatic (default: the persistent wave kernel with wave-uniform
 * sweeps for scenes of <= 16 objects whose meshes are single BVH leaves - the Cornell boxes -, the streamed forms 7 / 6
 * for scenes with a real BVH<Triangle> or more objects, the per-lane kernel with one lane per sample for what is left), 1 = per-lane kernel, one lane per pixel (any scene), 2 = persistent wave kernel with wave-uniform
 * sweeps (<= 16 objects; fails otherwise), 3 = the same with in-kernel section stamps (diagnostic build, slower),
 * 4 = per-lane kernel, one lane per sample (any scene), 5 = persistent wave kernel with the flattened per-lane
 * walk of both tree levels (<= 31 objects; fails otherwise; srt_pt_hit then also goes through that walk),
 * 6 = streamed form (any number of objects): a logic kernel per generation (consume hits, shade, refill, emit rays) and a
 * persistent ray-cast kernel that walks one ray per lane through both tree levels with LDS stacks and pulls rays from a
 * dense queue; 7 = streamed sweeps (<= 16 objects of which 1..4 meshes with a real BVH<Triangle>: BASELINE configs[4]): the
 * wave-uniform sweeps stay in the logic kernel, only the walks of those meshes are queued to the ray-cast kernel.
 * Automatic picks 7 where it applies, 6 for scenes the sweeps do not take.  All
 * produce bit-identical images; the switch exists for A/B tests and profiling. */
int srt_pt_set_kernel(srt_pt* pt, int mode);   /* modes 6 and 7: see below */
/* Mode 3 only: shader-clock cycles summed over waves per loop section
 * {refill, top-down sweep, leaf objects, combine, finish-direct, shade, terminate, 0}. */
int srt_pt_section_cycles(srt_pt* pt, uint64_t out[8], int reset);

/* Device time of the dominant kernel of render_epoch[_device] (pt_wave_kernel / pt_unit_kernel / pt_epoch_kernel,
 * whichever the scene selects; pt_normals_kernel while srt_pt_set_normal_colors is on), measured with HIP events recorded on the launch stream around each launch.
 * Returns the sum over the launches recorded since the previous call (waits for them), then switches
 * recording on (enable != 0) or off.  Off by default. */
int srt_pt_kernel_time(srt_pt* pt, int enable, double* total_ms, uint64_t* launches);

/* Streamed forms (kernel modes 6, 7) only: device time of the kernels of a generation - {logic (the resolve kernel where the
 * generation is split), compaction, ray cast, probe (0 where logic is one kernel)} - summed over every generation launched since
 * the previous call (HIP events around each launch, on the launch stream; waits for them), and the number of generations
 * enqueued; then switches recording on (enable != 0) or off.  Off by default: a diagnostic. */
int srt_pt_stream_times(srt_pt* pt, int enable, double ms_out[4], uint64_t* generations);
/* Streamed forms only: {entries queued to the ray-cast kernel, alive path-slot generations} summed over every generation of every launch since
 * the last reset (device counters of the compaction kernel; waits for the device), and the bytes the forms move through memory per alive
 * slot-generation (saved path state, both logic kernels) and per queued entry (ray planes, list entry, hit) as the kernels' layout has them.
 * bench.py prices the "ray state" term of SURVEY.md 8(d)'s byte figure with these. */
int srt_pt_stream_counters(srt_pt* pt, uint64_t out[4], int reset);
/* Which form render_epoch* takes for the committed scene under the current kernel mode: 0 persistent wave kernel with sweeps,
 * 1 the same with inline BVH<Triangle> walks, 2 persistent waves with the flattened walk, 3 streamed (every ray through the
 * ray-cast kernel), 4 streamed sweeps (BVH<Triangle> walks queued), -1 lane per sample, -2 lane per pixel; -3 while
 * srt_pt_set_normal_colors is on: the first-hit kernel of the normal-colors view, whatever the scene and the kernel mode. */
int srt_pt_kernel_form(srt_pt* pt, int* form);

/* Which route srt_pt_hit_device took: the calls since creation that went through {the ray-cast kernel, the nested per-lane walk,
 * the flattened per-lane walk}.  Lets a test state that the cast path really ran.  Works on a host-only context (all zero). */
int srt_pt_hit_device_paths(srt_pt* pt, uint64_t out[3]);

/* Traversal counters of the LAST srt_pt_trace_samples call (an instrumented launch):
 * {rays, box_tests, objects_entered, tri_tests, sphere_tests, tlas_nodes, blas_nodes, light_tri_tests}. */
int srt_pt_counters(srt_pt* pt, uint64_t out[8]);
/* What the scene holds and what it cost: {objects, triangle records stored, BVH<Triangle> nodes stored, BVH<Triangle> interior
 * records stored, BVH<Triangle> builds performed by this context since creation, scene bytes resident on the device, scene bytes
 * uploaded since creation, of those the triangle / normal / packed-triangle / BVH<Triangle>-record bytes}.  Lets a test state
 * that srt_pt_add_instance shared and srt_pt_repose left the triangles alone.  Works on a host-only context (device = -1): the
 * two byte figures of the device are then 0 and nothing is ever uploaded.  The first four are 0 before the first commit.
 * The resident bytes include the index buffers srt_pt_update_mesh's kernels read (12 B per triangle of every mesh that is neither
 * an instance nor an area light; under srt_pt_set_dynamic_lights an emissive mesh's too, from the commit or from its first update).  A successful srt_pt_update_mesh[_device] adds exactly 1 to the builds (nothing in a scene
 * committed without BVHs, where nothing is built) and to the two upload figures the bytes it actually copied from host to device:
 * the vertex arrays (host form), the primitive order of a host build, the nodes and records that are new or moved, the tables of
 * object order - the records its kernel writes on the device are not uploads.  A refused update adds nothing to the builds. */
int srt_pt_scene_counts(srt_pt* pt, uint64_t out[8]);
/* The trailing counter of the same family, in a call of its own so that out[8] above keeps its size for existing callers: the
 * successful srt_pt_refit_mesh[_device] / srt_pt_skin_pose_refit calls since creation, and the srt_pt_refit_mesh_inplace[_device] /
 * srt_pt_skin_pose_inplace calls (settles first, so the enqueue-only ones are counted).  A refit adds nothing to the builds and
 * nothing to the triangle-class upload figure (its kernels write the records); to the uploads it adds the vertex arrays (host
 * form), the BVH<Object> nodes and the tables of object order, and at a mesh's first refit its refit tables (4 B per triangle,
 * 8 B per node and per interior record, the level offsets).  A refused refit adds nothing to any figure: the vertices it had
 * staged are not counted at all, and tables it made stay resident and are counted with the mesh's first refit that succeeds. */
int srt_pt_refit_count(srt_pt* pt, uint64_t* refits);
/* The same for the BVH<Object>: the successful srt_pt_repose_refit[_device] calls since creation.  Settles first, so device-form
 * calls whose results the host has not read back yet are counted.  A top-level refit adds nothing to the builds or the
 * triangle-class figure; to the uploads it adds what srt_pt_repose_refit[_device] document. */
int srt_pt_top_refit_count(srt_pt* pt, uint64_t* refits);
/* What the host's record lags by, WITHOUT settling: out[0] = the srt_pt_repose_refit_device calls not applied yet, out[1] = the
 * entries of the set of objects they listed - at most the scene's object count, however many calls are pending.  (A pending
 * srt_pt_refit_mesh_inplace_device call refits the BVH<Object> too: it is counted in out[0] and lists no object.) */
int srt_pt_top_refit_pending(srt_pt* pt, uint64_t out[2]);
/* The same for srt_pt_refit_mesh_inplace_device, WITHOUT settling: out[0] = the calls not applied yet, out[1] = the meshes they
 * touched - at most one entry per mesh, however many calls are pending. */
int srt_pt_mesh_refit_pending(srt_pt* pt, uint64_t out[2]);
/* The area-light tables of the committed scene (what srt_pt_set_dynamic_lights keeps true).  Returns the number of lights, or a
 * negative status.  Per light li < cap_lights: heads[4 li ..] = {has_trans, first light triangle (tri_base - first light triangle
 * of the scene), triangle count, insertion index of the object}, mats[64 li ..] = trans, itrans, pdfT, pdfiT.  Per light triangle
 * t < cap_tris (every light's, in light order): tris[31 t ..] = v0 v1 v2 (four floats each, the padding included), area_term, then
 * p0 e1 e2 and n0 n1 n2 of the light-list copy (three floats each).  from_device == 0 reads the host's mirror; from_device != 0
 * waits for the device and reads the device arrays back (SRT_ERR_UNSUPPORTED on a host-only context).  The arrays may be NULL
 * where their capacity is 0. */
long srt_pt_dump_lights(srt_pt* pt, int from_device, uint32_t* heads, float* mats, size_t cap_lights, float* tris, size_t cap_tris);
/* The shading tables of the committed scene (what srt_pt_update_materials / srt_pt_update_lights / srt_pt_update_env_light and the
 * shading timelines write).  counts = {materials, delta lights}.  Per material k < cap_materials: the record the kernels read (a
 * Lambertian `a` already divided by PI_F, rays/bsdf.h:26).  Per delta light j < cap_lights: light_heads[2 j ..] = {type, has_trans},
 * light_values[37 j ..] = radiance3, angle_bounds2, trans16, itrans16.  env_type / env_radiance (may be NULL): the environment light;
 * the radiance is a launch parameter and the same on both sides.  from_device == 0 reads the host's record (after settling);
 * from_device != 0 waits for the device and reads the device tables back (SRT_ERR_UNSUPPORTED on a host-only context).  The arrays
 * may be NULL where their capacity is 0. */
int srt_pt_dump_shading(srt_pt* pt, int from_device, uint32_t counts[2], srt_pt_material* materials, size_t cap_materials, uint32_t* light_heads,
                        float* light_values, size_t cap_lights, uint32_t* env_type, float env_radiance[3]);
/* cosf/sinf of the kernel (SRT-MATH v2) for n host floats; parity tests compare them with glibc. */
int srt_pt_math_cos_sin(srt_pt* pt, const float* x, size_t n, float* cos_out, float* sin_out);
/* The same through srt_sincosf2 (both values from one reduction: what the samplers call); srt_pt_math_cos_sin goes through the
 * single-function forms.  Argument i is evaluated by lane i % 64 of wave i / 64, every wave with all of its lanes. */
int srt_pt_math_sincos2(srt_pt* pt, const float* x, size_t n, float* cos_out, float* sin_out);
/* The kernels' atan2f (glibc 2.35's algorithm restated; Spot_Light::sample) evaluated on the device. */
int srt_pt_math_atan2(srt_pt* pt, const float* y, const float* x, size_t n, float* out);
/* The kernels' acosf (glibc 2.35's algorithm restated; Samplers::Hemisphere::Uniform) evaluated on the device. */
int srt_pt_math_acos(srt_pt* pt, const float* x, size_t n, float* out);
/* The kernels' DOUBLE sin of a float in [0, 1] (glibc 2.35's __sin restated with the fused multiply-adds of its FMA build;
 * Samplers::Sphere::Image::pdf, student/samplers.cpp:135) evaluated on the device.  out: n doubles. */
int srt_pt_math_sin_unit(srt_pt* pt, const float* x, size_t n, double* out);
/* Samplers::Sphere::Image of the context's environment map (srt_pt_set_env_map; SRT_ERR_INVALID without one), whatever
 * srt_pt_set_env_sampling says: dims = {w, h}, *total the constructor's float total, cdf / pdf the normalised _cdf / _pdf (w * h
 * floats each, row-major), trig the doubles of sample() (student/samplers.cpp:103-112) - sin theta of rows 0 .. h, cos theta of rows
 * 0 .. h, cos phi of columns 0 .. w - 1, sin phi of columns 0 .. w - 1: 2 (h + 1) + 2 w doubles.  from_device == 0: the host's
 * tables (built if this map has none yet; a host-only context will do); != 0: the device copies read back (made and uploaded if
 * missing; waits for the device; total is the host's - the device holds the normalised tables).  NULL arrays are skipped. */
int srt_pt_dump_env_sampler(srt_pt* pt, int from_device, uint32_t dims[2], float* total, float* cdf, float* pdf, size_t cap_texels,
                            double* trig, size_t cap_trig);
/* sample() and pdf() of that sampler by a kernel, through the device functions the render uses (env_image_upper_bound,
 * env_image_direction, env_image_pdf in csrc/pt_trace.h): for each of nu chosen draws u the index std::upper_bound arrives at and
 * the direction (3 floats) sample() returns for it; for each of nd directions (3 floats, not normalised by the call) pdf(). */
int srt_pt_env_sampler_probe(srt_pt* pt, const float* u, size_t nu, uint32_t* index_out, float* dir_out, const float* dirs, size_t nd,
                             float* pdf_out);
/* The timelines' hypotf (glibc 2.35's __hypotf restated: evaluated in fp64; Mat4::to_euler, lib/mat4.h:177) evaluated on the device. */
int srt_pt_math_hypot(srt_pt* pt, const float* x, const float* y, size_t n, float* out);
/* What srt_pt_skin_set_rig validates and srt_pt_skin_posed computes, without a skin or a context (a host-only context has no skins):
 * Skeleton::set_time(t) and Skeleton::joint_to_posed (student/skeleton.cpp:26-52, 106-115) of a rig given as srt_pt_skin_set_rig
 * takes it, with the joints' extents (3 floats each) in the place of the skin's.  euler_out (3 floats per joint, may be NULL) takes
 * Joint::pose after set_time, posed_out 16 floats per joint.  SRT_ERR_INVALID as for srt_pt_skin_set_rig. */
int srt_pt_rig_posed_host(uint32_t njoints, const int32_t* parent, const float* extents, const float base[3], const float* rest_pose,
                          const uint32_t* knot_offsets, const float* knot_times, const float* knot_quats, float t, float* euler_out, float* posed_out);
/* What srt_pt_skin_step_ik computes, without a skin or a context: Skeleton::do_ik `calls` times on pose_inout (3 floats per joint,
 * in place) for a hierarchy as srt_pt_skin_set_rig takes it (parents first), the joints' extents (3 floats each), the handles'
 * joints in do_ik's order, their targets (3 floats each, skeleton space) and enabled bytes (NULL: every handle).  The same functions
 * the kernel runs (pt_ik.h), on the host.  SRT_ERR_INVALID for a NULL argument, a parent out of order or a handle's joint out of
 * range; SRT_ERR_UNSUPPORTED beyond 4096 joints or 1024 handles; pose_inout is untouched then. */
int srt_pt_rig_step_ik_host(uint32_t njoints, const int32_t* parent, const float* extents, float* pose_inout, const uint32_t* handle_joints,
                            const float* targets, const uint8_t* enabled, uint32_t nhandles, uint32_t calls);
/* The schedule half of srt_pt_emitter_step(em, dt) alone - last_update, particle_cooldown and the birth ordinals advance as the step
 * advances them, nothing is enqueued - on any context, a host-only one included.  *substeps = the substeps of the call,
 * spawns_out[i] (i < min(*substeps, cap)) = the spawns behind substep i, *cleared = 1 when the emitter is disabled (the step would
 * clear).  schedule_out (may be NULL): {last_update as a double, particle_cooldown} afterwards.  Refusals are the step's. */
int srt_pt_emitter_advance_host(srt_pt_emitter* em, float dt, uint32_t* substeps, uint32_t* spawns_out, uint32_t cap, int* cleared, double schedule_out[2]);

/* The epilogue's expf / powf (glibc 2.35's algorithms restated, FMA build) evaluated on the device. */
int srt_pt_math_exp(srt_pt* pt, const float* x, size_t n, float* out);
int srt_pt_math_pow(srt_pt* pt, const float* x, const float* y, size_t n, float* out);
/* The wave kernel's batched IEEE divide / square root (pt_device.h: div3x3, sqrt3) on host operands, called exactly as
 * the batch tests call them: lane i handles operands 3i, 3i+1, 3i+2.  in: five planes of 3*lanes floats (num0, num1,
 * num2, den, x); out: four planes (num0/den, num1/den, num2/den, sqrt(x)).  shared_c2 != 0: a lane's three rays share
 * num2[3i].  Parity tests compare the planes with the host's correctly rounded `/` and sqrtf. */
int srt_pt_math_div_sqrt(srt_pt* pt, const float* in, size_t lanes, int shared_c2, float* out);
/* The wave kernel's batch Triangle::hit (pt_device.h: tri_hitN<3>, inside / outside verdict from the numerators and det, only t
 * divided) next to the plain per-ray tri_hit, lane i on its own triangle, origin and three rays.  in: 27 planes of `lanes`
 * floats (p0 xyz, e1 xyz, e2 xyz, origin xyz, direction xyz of rays 0, 1, 2, dist_bounds.x of the three rays, dist_bounds.y of
 * the three rays); out: 19 planes ({hit as 0 / 1, t, dist} of rays 0, 1, 2 from the batch form, the same nine from tri_hit, and
 * 1 where the lane's wave held an ambiguous lane and computed u and v after all; a wave is 64 consecutive lanes). */
int srt_pt_math_tri_verdict(srt_pt* pt, const float* in, size_t lanes, float* out);
/* The leaf fold of the wave kernel's mesh branch (pt_device.h: leaf_foldN - a candidate pass over the leaf's triangles, then one
 * quotient and one root per ray; a wave with a bad lane folds the leaf the long way) next to the plain ordered fold over tri_hit
 * (ret = Trace::min(ret, Triangle::hit)), one leaf per wave of 64 consecutive lanes, lane i on its own origin and three rays.
 * lanes must be a multiple of 64.  in: first, per wave, 148 words - the number of triangles as a uint32 (1..12), three unused
 * words, then twelve triangles of 12 floats (p0 xyz and a pad, e1 xyz and a pad, e2 xyz and a pad) -, then 18 planes of `lanes`
 * floats (origin xyz, direction xyz of rays 0, 1, 2, dist_bounds.x of the three rays, dist_bounds.y of the three rays); out: 25
 * planes (per ray {hit as 0 / 1, winning triangle as a uint32 or 0 without a hit, t, dist} from the leaf code and the same four
 * from the plain fold, then 1 where the lane's wave fell back).  SRT_ERR_INVALID for a count outside 1..12 or lanes % 64 != 0. */
int srt_pt_math_leaf_fold(srt_pt* pt, const float* in, size_t lanes, float* out);
/* The wave kernel's batch Sphere::hit (pt_device.h: sphere_hitN<3>, whose tangent root is computed wave-uniformly, then the distance
 * step of Object::hit through sqrtN, as the sphere branch of object_testN in pt_wave.h performs it) next to the plain per-ray form
 * (sphere_hit and |Ray::at(t) - origin|), lane i on its own radius, origin and three rays.  in: 19 planes of `lanes` floats (radius,
 * origin xyz, direction xyz of rays 0, 1, 2, dist_bounds.x of the three rays, dist_bounds.y of the three rays); out: 22 planes ({hit
 * as 0 / 1, t, dist} of rays 0, 1, 2 from the batch form, the same nine from the plain form, delta of rays 0, 1, 2, and 1 where the
 * lane's wave held a lane with delta == 0 and computed the tangent root; a wave is 64 consecutive lanes). */
int srt_pt_math_sphere_batch(srt_pt* pt, const float* in, size_t lanes, float* out);
/* BBox::hit as the sweeps of pt_wave.h evaluate it (box_hit_inv - both products per axis, the select on the results) next to the
 * form of the per-lane traversals (box_hit_rec - the bound selected first; both in pt_trace.h), lane i on its own operands.  in: 14 planes
 * of `lanes` floats (box min xyz, box max xyz, origin xyz, reciprocal direction xyz, incoming times x and y); out: 6 planes ({hit
 * as 0 / 1, times.x, times.y} of box_hit_inv, the same three of box_hit_rec). */
int srt_pt_math_box_sweep(srt_pt* pt, const float* in, size_t lanes, float* out);
/* Mat4 * Vec3 as the leaf section of pt_wave.h transforms points with an object's matrix (pt_device.h: mat_point_affine - for a
 * bottom row of (+-0, +-0, +-0, 1) and a finite first output row in every lane of the wave, w is not computed) next to the plain
 * projective product (mat_point), one matrix per wave of 64 consecutive lanes, lane i on its own point.  lanes must be a multiple
 * of 64.  in: first, per wave, the matrix as Mat4::data has it (16 floats, column-major), then 3 planes of `lanes` floats (the point);
 * out: 7 planes (x, y, z from mat_point_affine, x, y, z from mat_point, and 1 where the lane's wave did not compute w). */
int srt_pt_math_point_affine(srt_pt* pt, const float* in, size_t lanes, float* out);
/* The top-down sweep of pt_wave.h over a seven-node tree with the min / max step behind its no-NaN guard (pt_trace.h: box_hit_minmax;
 * a wave takes it iff every box of its tree is finite with lo <= hi and every lane's origin is finite and its reciprocals finite and
 * not zero) next to the same sweep through the old step, one tree per wave of 64 consecutive lanes, lane i on its own ray.  lanes must
 * be a multiple of 64.  in: first, per wave, seven WaveInterior records (16 words each: left box min xyz max xyz, right box the same,
 * l_ref, r_ref, two counts; a child reference is negative for a leaf or the index of a later node of the seven), then 10 planes of
 * `lanes` floats (origin xyz, reciprocal direction xyz, the root's times x and y, dist_bounds x and y); out: 85 planes - per node
 * {flag nibble as a 32-bit integer, cur_far_t.x, left child's times x, y, right child's times x, y} of the guarded sweep (42), the
 * same of the old step (42), and 1 where the lane's wave took the min / max step. */
int srt_pt_math_topdown_minmax(srt_pt* pt, const float* in, size_t lanes, float* out);

/* The HIP resources the library holds at this moment, process-wide (every path-tracer and rasterizer context, multi-device group,
 * skin and timeline): out = {device buffers, pinned host buffers, events, streams}.  Each counts the live allocations, not their
 * bytes.  A test reads it before and after a sequence of calls that ends with the destroys: equal readings mean nothing leaked and
 * nothing was freed twice.  Needs no context and no device. */
int srt_pt_live_resources(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* SRT_PT_DEBUG_H */
