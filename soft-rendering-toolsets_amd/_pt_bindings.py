"""ctypes bindings of include/srt_pt.h and a mirror of PT::Pathtracer's public surface
(/root/reference/Assignments/Scotty3D/src/rays/pathtracer.h:24-40).  Plumbing only: every number
is produced by the HIP kernels behind the C ABI."""
from __future__ import annotations

import ctypes
import os
import weakref
from ctypes import POINTER, c_float, c_int, c_long, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np


class PtMaterial(ctypes.Structure):
    _fields_ = [("type", c_uint32), ("a", c_float * 3), ("b", c_float * 3), ("ior", c_float)]


# srt_pt_logged_ray (include/srt_pt.h): one call of Pathtracer::log_ray
LOGGED_RAY_DTYPE = np.dtype([("point", np.float32, 3), ("dir", np.float32, 3), ("t", np.float32), ("pixel", np.uint32),
                             ("sample", np.uint32), ("bounce", np.uint32)])
SRT_CANCELLED = 1


class SrtCancelled(Exception):
    """A render call returned SRT_CANCELLED: srt_pt_cancel cut it short, its output was not written."""


_HIP_MEMCPY_D2H = 2   # hipMemcpyDeviceToHost

SCENE_COUNT_NAMES = ("objects", "triangles", "blas_nodes", "blas_records", "blas_builds", "device_bytes", "uploaded_bytes",
                     "uploaded_triangle_bytes", "refits")
COUNTER_NAMES = ("rays", "box_tests", "objects_entered", "tri_tests", "sphere_tests", "tlas_nodes", "blas_nodes",
                 "light_tri_tests")


def bind(lib: ctypes.CDLL) -> None:
    lib.srt_pt_create.argtypes = [c_int, POINTER(c_void_p)]
    lib.srt_pt_create_multi.argtypes = [c_void_p, c_int, POINTER(c_void_p)]
    lib.srt_pt_group_destroy.argtypes = [c_void_p]
    lib.srt_pt_group_size.argtypes = [c_void_p]
    lib.srt_pt_group_context.argtypes = [c_void_p, c_int]
    lib.srt_pt_group_context.restype = c_void_p
    lib.srt_pt_group_uses_rccl.argtypes = [c_void_p]
    lib.srt_pt_group_set_params.argtypes = [c_void_p, c_uint32, c_uint32, c_uint32]
    lib.srt_pt_group_render_epoch.argtypes = [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p]
    lib.srt_pt_group_render_epoch_device.argtypes = [c_void_p, c_uint64, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p)]
    lib.srt_pt_group_gather_time.argtypes = [c_void_p, c_int, POINTER(ctypes.c_double), POINTER(c_uint64)]
    lib.srt_pt_destroy.argtypes = [c_void_p]
    lib.srt_pt_scene_begin.argtypes = [c_void_p]
    lib.srt_pt_add_material.argtypes = [c_void_p, POINTER(PtMaterial), POINTER(c_uint32)]
    lib.srt_pt_add_mesh.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p, c_uint32, c_int]
    lib.srt_pt_set_env_light.argtypes = [c_void_p, c_uint32, c_void_p]
    lib.srt_pt_set_env_map.argtypes = [c_void_p, c_uint32, c_uint32, c_void_p]
    lib.srt_pt_add_sphere_light.argtypes = [c_void_p, c_float, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32]
    lib.srt_pt_add_light.argtypes = [c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_add_sphere.argtypes = [c_void_p, c_float, c_void_p, c_uint32]
    lib.srt_pt_add_instance.argtypes = [c_void_p, c_uint32, c_void_p, c_uint32]
    lib.srt_pt_scene_commit.argtypes = [c_void_p, c_int]
    lib.srt_pt_repose.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_repose_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_particle_transforms_device.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_float, c_void_p]
    lib.srt_pt_update_mesh.argtypes = [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_update_mesh_device.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_refit_mesh.argtypes = [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_refit_mesh_device.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_skin_pose_refit.argtypes = [c_void_p, c_void_p, c_void_p, c_int]
    lib.srt_pt_refit_mesh_inplace.argtypes = [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_refit_mesh_inplace_device.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_mesh_refit_pending.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_skin_pose_inplace.argtypes = [c_void_p, c_void_p, c_void_p, c_int]
    lib.srt_pt_skin_pose_inplace_at.argtypes = [c_void_p, c_void_p, c_float, c_int]
    lib.srt_pt_repose_refit.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_repose_refit_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_scene_tree_cost.argtypes = [c_void_p, POINTER(ctypes.c_double)]
    lib.srt_pt_set_active.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_set_active_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_get_active.argtypes = [c_void_p, c_void_p, c_uint32]
    lib.srt_pt_group_set_active.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_group_set_active_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_top_refit_count.argtypes = [c_void_p, POINTER(c_uint64)]
    lib.srt_pt_top_refit_pending.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_mesh_tree_cost.argtypes = [c_void_p, c_uint32, POINTER(ctypes.c_double)]
    lib.srt_pt_refit_count.argtypes = [c_void_p, POINTER(c_uint64)]
    lib.srt_pt_skin_create.argtypes = [c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_void_p]
    lib.srt_pt_skin_destroy.argtypes = [c_void_p]
    lib.srt_pt_skin_counts.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_skin_map.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_skin_vertices_device.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.srt_pt_skin_vertices.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.srt_pt_skin_pose.argtypes = [c_void_p, c_void_p, c_void_p, c_int]
    lib.srt_pt_skin_set_rig.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_skin_posed.argtypes = [c_void_p, c_float, c_void_p]
    lib.srt_pt_skin_posed_device.argtypes = [c_void_p, c_void_p, c_float, c_void_p]
    lib.srt_pt_skin_vertices_at_device.argtypes = [c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]
    lib.srt_pt_skin_pose_at.argtypes = [c_void_p, c_void_p, c_float, c_int]
    lib.srt_pt_skin_pose_refit_at.argtypes = [c_void_p, c_void_p, c_float, c_int]
    lib.srt_pt_rig_posed_host.argtypes = [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p]
    lib.srt_pt_skin_set_ik_handles.argtypes = [c_void_p, c_void_p, c_uint32]
    lib.srt_pt_skin_set_joint_pose.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_skin_joint_pose.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_skin_set_time.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_skin_step_ik.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.srt_pt_skin_step_ik_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_skin_posed_current.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_skin_posed_current_device.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.srt_pt_skin_vertices_current_device.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
    lib.srt_pt_skin_pose_current.argtypes = [c_void_p, c_void_p, c_int, c_int]
    lib.srt_pt_rig_step_ik_host.argtypes = [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_uint32]
    lib.srt_pt_math_hypot.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_live_resources.argtypes = [c_void_p]
    lib.srt_pt_timeline_create.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_timeline_destroy.argtypes = [c_void_p]
    lib.srt_pt_timeline_transforms.argtypes = [c_void_p, c_float, c_void_p]
    lib.srt_pt_timeline_transforms_device.argtypes = [c_void_p, c_void_p, c_float, c_void_p]
    lib.srt_pt_timeline_repose_refit.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_timeline_repose.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_update_materials.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_update_lights.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32]
    lib.srt_pt_update_env_light.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_shading_timeline_create.argtypes = [c_void_p, c_void_p, c_uint32, c_void_p, c_uint32, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_shading_timeline_destroy.argtypes = [c_void_p]
    lib.srt_pt_shading_timeline_values.argtypes = [c_void_p, c_float, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_shading_timeline_update.argtypes = [c_void_p, c_float]
    lib.srt_pt_shading_timeline_apply.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_dump_shading.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.srt_pt_scene_counts.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_set_bvh_builder.argtypes = [c_void_p, c_int, c_uint32]
    lib.srt_pt_set_stream_slots.argtypes = [c_void_p, c_uint32]
    lib.srt_pt_set_camera.argtypes = [c_void_p, c_void_p, c_float, c_float]
    lib.srt_pt_set_params.argtypes = [c_void_p, c_uint32, c_uint32, c_uint32]
    lib.srt_pt_set_tiling.argtypes = [c_void_p, c_uint32, c_uint32, c_uint32, c_uint32]
    lib.srt_pt_tile_info.argtypes = [c_void_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32)]
    lib.srt_pt_render_epoch.argtypes = [c_void_p, c_uint64, c_uint32, c_uint32, c_void_p]
    lib.srt_pt_render_epoch_device.argtypes = [c_void_p, c_void_p, c_uint64, c_uint32, c_uint32, c_void_p]
    lib.srt_pt_untile_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_accumulate_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_uint32]
    lib.srt_pt_set_kernel.argtypes = [c_void_p, c_int]
    lib.srt_pt_section_cycles.argtypes = [c_void_p, c_void_p, c_int]
    lib.srt_pt_kernel_time.argtypes = [c_void_p, c_int, POINTER(ctypes.c_double), POINTER(c_uint64)]
    lib.srt_pt_ray_count.argtypes = [c_void_p, POINTER(c_uint64), POINTER(c_uint64), c_int]
    lib.srt_pt_stream_times.argtypes = [c_void_p, c_int, c_void_p, POINTER(c_uint64)]
    lib.srt_pt_stream_counters.argtypes = [c_void_p, c_void_p, c_int]
    lib.srt_pt_kernel_form.argtypes = [c_void_p, POINTER(c_int)]
    lib.srt_pt_trace_samples.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_hit.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_hit_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_hit_device_paths.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_particles_step.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_void_p]
    lib.srt_pt_particles_step_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_void_p]
    lib.srt_pt_emitter_create.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_float, c_void_p]
    lib.srt_pt_emitter_destroy.argtypes = [c_void_p]
    lib.srt_pt_emitter_set_options.argtypes = [c_void_p, c_float, c_float, c_float, c_float, c_float, c_float, c_int]
    lib.srt_pt_emitter_set_pose.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.srt_pt_emitter_seed.argtypes = [c_void_p, c_uint64]
    lib.srt_pt_emitter_set_uniforms_device.argtypes = [c_void_p, c_void_p, c_size_t]
    lib.srt_pt_emitter_step_device.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_emitter_step.argtypes = [c_void_p, c_float]
    lib.srt_pt_emitter_present_device.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_emitter_frame_device.argtypes = [c_void_p, c_void_p, c_float]
    lib.srt_pt_emitter_clear_device.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_emitter_clear.argtypes = [c_void_p]
    lib.srt_pt_emitter_read.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_emitter_write.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_emitter_counts.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_emitter_arrays_device.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_emitter_advance_host.argtypes = [c_void_p, c_float, POINTER(c_uint32), c_void_p, c_uint32, POINTER(c_int), c_void_p]
    lib.srt_pt_dump_bvh.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_dump_bvh.restype = c_long
    lib.srt_pt_counters.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_math_cos_sin.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.srt_pt_math_sincos2.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]
    lib.srt_pt_math_acos.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_atan2.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_set_elision.argtypes = [c_void_p, c_int]
    lib.srt_pt_rays_elided.argtypes = [c_void_p, POINTER(c_uint64), c_int]
    lib.srt_pt_set_normal_colors.argtypes = [c_void_p, c_int]
    lib.srt_pt_set_env_sampling.argtypes = [c_void_p, c_uint32]
    lib.srt_pt_env_sampling.argtypes = [c_void_p, c_void_p]
    lib.srt_pt_group_set_env_sampling.argtypes = [c_void_p, c_uint32]
    lib.srt_pt_math_sin_unit.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_dump_env_sampler.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]
    lib.srt_pt_env_sampler_probe.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_group_set_normal_colors.argtypes = [c_void_p, c_int]
    lib.srt_pt_set_dynamic_lights.argtypes = [c_void_p, c_int]
    lib.srt_pt_group_set_dynamic_lights.argtypes = [c_void_p, c_int]
    lib.srt_pt_dump_lights.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]
    lib.srt_pt_dump_lights.restype = c_long
    lib.srt_pt_math_exp.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_pow.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_tonemap.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32, c_float, c_void_p]
    lib.srt_pt_tonemap_device.argtypes = [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_float, c_void_p]
    lib.srt_pt_math_div_sqrt.argtypes = [c_void_p, c_void_p, c_size_t, ctypes.c_int, c_void_p]
    lib.srt_pt_math_tri_verdict.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_leaf_fold.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_box_sweep.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_point_affine.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_topdown_minmax.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_math_sphere_batch.argtypes = [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.srt_pt_sync.argtypes = [c_void_p]
    lib.srt_pt_cancel.argtypes = [c_void_p]
    lib.srt_pt_cancel_requested.argtypes = [c_void_p]
    lib.srt_pt_clear_cancel.argtypes = [c_void_p]
    lib.srt_pt_set_ray_log.argtypes = [c_void_p, c_uint32]
    lib.srt_pt_read_ray_log.argtypes = [c_void_p, c_void_p, c_size_t, POINTER(c_size_t), POINTER(c_uint64)]
    lib.srt_pt_read_ray_log_stream.argtypes = [c_void_p, c_void_p, c_void_p, c_size_t, POINTER(c_size_t), POINTER(c_uint64)]
    lib.srt_pt_group_render_epoch_lane.argtypes = [c_void_p, c_int, c_uint64, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p)]
    lib.srt_pt_group_cancel.argtypes = [c_void_p]
    lib.srt_pt_group_clear_cancel.argtypes = [c_void_p]
    lib.srt_pt_group_set_ray_log.argtypes = [c_void_p, c_uint32]
    lib.srt_pt_group_read_ray_log.argtypes = [c_void_p, c_int, c_void_p, c_size_t, POINTER(c_size_t), POINTER(c_uint64)]
    lib.srt_pt_max_samples_per_launch.argtypes = [c_void_p, POINTER(c_uint32)]
    lib.srt_pt_accumulator_floats.argtypes = [c_void_p, POINTER(c_size_t)]
    lib.srt_pt_render_samples_device.argtypes = [c_void_p, c_void_p, c_uint64, c_uint32, c_uint32]
    lib.srt_pt_fold_epochs_device.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p]
    lib.srt_pt_accumulator_tiles_device.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.srt_pt_group_reset_accumulator.argtypes = [c_void_p]
    lib.srt_pt_group_max_samples_per_launch.argtypes = [c_void_p, POINTER(c_uint32)]
    lib.srt_pt_group_render_samples.argtypes = [c_void_p, c_int, c_uint64, c_uint32, c_uint32]
    lib.srt_pt_group_wait_lane.argtypes = [c_void_p, c_int]
    lib.srt_pt_group_fold.argtypes = [c_void_p, c_int, c_uint32, c_uint32, c_uint32, c_uint32]
    lib.srt_pt_group_accumulator_image.argtypes = [c_void_p, POINTER(c_void_p), POINTER(c_void_p)]
    lib.srt_pt_group_cancel_requested.argtypes = [c_void_p]
    # (the HIP runtime's own calls, for PathtracerGroup.accumulator_image's read-back)
    lib.hipSetDevice.argtypes = [c_int]
    lib.hipMemcpyAsync.argtypes = [c_void_p, c_void_p, c_size_t, c_int, c_void_p]
    lib.hipStreamSynchronize.argtypes = [c_void_p]


def live_resources() -> tuple:
    """srt_pt_live_resources: the (device buffers, pinned buffers, events, streams) the library holds right now, process-wide."""
    from . import _check, load_library
    lib = load_library()
    out = np.zeros(4, np.uint64)
    _check(lib, lib.srt_pt_live_resources(out.ctypes.data_as(c_void_p)))
    return tuple(int(v) for v in out)


def _p(a):
    return a.ctypes.data_as(c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


SKIN_JOINT_DTYPE = np.dtype([("bind", np.float32, 16), ("extent", np.float32, 3), ("radius", np.float32)])   # srt_pt_skin_joint


def skin_joints(joints) -> np.ndarray:
    """srt_pt_skin_joint records from an array of SKIN_JOINT_DTYPE or a sequence of (bind16, extent3, radius) / dicts with those keys,
    in Skeleton::for_joints order."""
    if isinstance(joints, np.ndarray) and joints.dtype == SKIN_JOINT_DTYPE:
        return np.ascontiguousarray(joints)
    out = np.zeros(len(joints), SKIN_JOINT_DTYPE)
    for k, j in enumerate(joints):
        bind, extent, radius = (j["bind"], j["extent"], j["radius"]) if isinstance(j, dict) else j
        out[k] = (_f32(bind).reshape(16), _f32(extent).reshape(3), np.float32(radius))
    return out


class Skin:
    """srt_pt_skin: Skeleton::find_joints done once at creation (Pathtracer.create_skin), Skeleton::skin per call.  `posed` is
    (njoints, 16): Skeleton::joint_to_posed(j) in Mat4::data order, in the joints' order."""

    def __init__(self, pt, handle, nverts: int, njoints: int):
        self._pt, self._lib, self._check = pt, pt._lib, pt._check
        self._h = handle
        self.nverts, self.njoints = nverts, njoints

    def _posed(self, posed):
        posed = _f32(posed).reshape(-1, 16)
        if len(posed) != self.njoints:
            raise ValueError(f"{len(posed)} posed matrices for {self.njoints} joints")
        return posed

    def counts(self) -> dict:
        out = np.zeros(4, np.uint32)
        self._check(self._lib, self._lib.srt_pt_skin_counts(self._h, _p(out)))
        return dict(zip(("vertices", "joints", "influences", "triangles"), (int(v) for v in out)))

    def map(self):
        """(offsets[nverts + 1], joints[n], weights[n]): vertex v's influences are [offsets[v], offsets[v + 1])."""
        n = self.counts()["influences"]
        off, jidx, w = np.zeros(self.nverts + 1, np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_map(self._h, _p(off), _p(jidx), _p(w), n))
        return off, jidx[:n], w[:n]

    def vertices(self, posed, flat_normals: bool = False):
        """srt_pt_skin_vertices: the skinned (positions, normals), (nverts, 3) each."""
        posed = self._posed(posed)
        pos, nrm = np.zeros((self.nverts, 3), np.float32), np.zeros((self.nverts, 3), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_vertices(self._h, _p(posed), int(bool(flat_normals)), _p(pos), _p(nrm)))
        return pos, nrm

    def vertices_device(self, posed, d_pos_ptr: int, d_nrm_ptr: int, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_vertices_device: the same into two device arrays of nverts * 3 floats; only enqueues."""
        posed = self._posed(posed)
        self._check(self._lib, self._lib.srt_pt_skin_vertices_device(self._h, c_void_p(stream), _p(posed), int(bool(flat_normals)),
                                                                     c_void_p(d_pos_ptr), c_void_p(d_nrm_ptr)))

    def pose(self, posed, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose: skin, then srt_pt_update_mesh_device with the result - the committed mesh takes the pose."""
        posed = self._posed(posed)
        self._check(self._lib, self._lib.srt_pt_skin_pose(self._h, c_void_p(stream), _p(posed), int(bool(flat_normals))))

    def pose_refit(self, posed, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_refit: skin, then srt_pt_refit_mesh_device with the result - the committed mesh takes the pose and keeps its tree."""
        posed = self._posed(posed)
        self._check(self._lib, self._lib.srt_pt_skin_pose_refit(self._h, c_void_p(stream), _p(posed), int(bool(flat_normals))))

    def pose_inplace(self, posed, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_inplace: skin, then srt_pt_refit_mesh_inplace_device with the result - both trees kept, only enqueued on
        `stream`: no wait, no read-back (64 B per joint go up).  The host's record settles as after repose_refit_device."""
        posed = self._posed(posed)
        self._check(self._lib, self._lib.srt_pt_skin_pose_inplace(self._h, c_void_p(stream), _p(posed), int(bool(flat_normals))))

    def pose_inplace_at(self, t: float, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_inplace_at: pose_inplace() with the matrices of time t computed on the device from the rig - a frame is
        one float, nothing goes up and nothing is waited for."""
        self._check(self._lib, self._lib.srt_pt_skin_pose_inplace_at(self._h, c_void_p(stream), float(t), int(bool(flat_normals))))

    def set_rig(self, parent, base, rest_pose, knot_offsets, knot_times, knot_quats) -> None:
        """srt_pt_skin_set_rig: the hierarchy (parent[j] < j or -1, the joints in the skin's order), Skeleton::base_pos, the rest pose
        (3 Euler angles in degrees per joint) and the joints' keys as CSR (knot_offsets[njoints + 1], times, xyzw quaternions).
        Uploaded once; posed_at / pose_at / pose_refit_at then take a time."""
        parent = np.ascontiguousarray(parent, np.int32).reshape(-1)
        rest, off = _f32(rest_pose).reshape(-1, 3), np.ascontiguousarray(knot_offsets, np.uint32).reshape(-1)
        times, quats = _f32(knot_times).reshape(-1), _f32(knot_quats).reshape(-1, 4)
        if len(parent) != self.njoints or len(rest) != self.njoints or len(off) != self.njoints + 1:
            raise ValueError(f"{len(parent)} parents, {len(rest)} rest poses and {len(off)} offsets for {self.njoints} joints")
        if len(times) != len(quats) or (len(off) and int(off.max()) > len(times)):
            raise ValueError(f"{len(times)} knot times, {len(quats)} quaternions, offsets up to {int(off.max())}")
        if len(times) == 0:
            times, quats = np.zeros(1, np.float32), np.zeros((1, 4), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_set_rig(self._h, _p(parent), _p(_f32(base).reshape(3)), _p(rest), _p(off), _p(times), _p(quats)))

    def posed_at(self, t: float) -> np.ndarray:
        """srt_pt_skin_posed: Skeleton::joint_to_posed of every joint after Skeleton::set_time(t), (njoints, 16), computed on the host."""
        out = np.zeros((self.njoints, 16), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_posed(self._h, float(t), _p(out)))
        return out

    def posed_at_device(self, t: float, d_posed_ptr: int, stream: int = 0) -> None:
        """srt_pt_skin_posed_device: the same by the joint kernels into a device array of njoints * 16 floats; only enqueues."""
        self._check(self._lib, self._lib.srt_pt_skin_posed_device(self._h, c_void_p(stream), float(t), c_void_p(d_posed_ptr)))

    def vertices_at_device(self, t: float, d_pos_ptr: int, d_nrm_ptr: int, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_vertices_at_device: vertices_device with the matrices of time t from the rig; nothing goes up."""
        self._check(self._lib, self._lib.srt_pt_skin_vertices_at_device(self._h, c_void_p(stream), float(t), int(bool(flat_normals)), c_void_p(d_pos_ptr),
                                                                        c_void_p(d_nrm_ptr)))

    def pose_at(self, t: float, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_at: pose() with the matrices of time t computed on the device from the rig."""
        self._check(self._lib, self._lib.srt_pt_skin_pose_at(self._h, c_void_p(stream), float(t), int(bool(flat_normals))))

    def pose_refit_at(self, t: float, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_refit_at: pose_refit() with the matrices of time t computed on the device from the rig."""
        self._check(self._lib, self._lib.srt_pt_skin_pose_refit_at(self._h, c_void_p(stream), float(t), int(bool(flat_normals))))

    # ---- the current Joint::pose and the IK handles (Skeleton::set_time, Skeleton::do_ik) ----
    HOW = {"update": 0, "refit": 1, "inplace": 2}          # SRT_PT_SKIN_UPDATE / _REFIT / _INPLACE

    def set_ik_handles(self, joints) -> None:
        """srt_pt_skin_set_ik_handles: the handles' joints in the order Skeleton::do_ik visits them (that order is part of the
        result); an empty list clears."""
        joints = np.ascontiguousarray(joints, np.uint32).reshape(-1)
        self._check(self._lib, self._lib.srt_pt_skin_set_ik_handles(self._h, _p(joints) if len(joints) else None, len(joints)))
        self.nhandles = len(joints)

    def set_joint_pose(self, euler) -> None:
        """srt_pt_skin_set_joint_pose: the current Joint::pose, (njoints, 3) Euler angles in degrees."""
        euler = _f32(euler).reshape(-1, 3)
        if len(euler) != self.njoints:
            raise ValueError(f"{len(euler)} poses for {self.njoints} joints")
        self._check(self._lib, self._lib.srt_pt_skin_set_joint_pose(self._h, _p(euler)))

    def joint_pose(self) -> np.ndarray:
        """srt_pt_skin_joint_pose: the current Joint::pose, (njoints, 3); waits for what was enqueued."""
        out = np.zeros((self.njoints, 3), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_joint_pose(self._h, _p(out)))
        return out

    def set_time(self, t: float, stream: int = 0) -> None:
        """srt_pt_skin_set_time: Skeleton::set_time(t) on the current pose - keyed joints take their keys' value, the others keep
        what they have; only enqueues."""
        self._check(self._lib, self._lib.srt_pt_skin_set_time(self._h, c_void_p(stream), float(t)))

    def _handle_arrays(self, targets, enabled):
        n = getattr(self, "nhandles", 0)
        targets = _f32(targets).reshape(-1, 3)
        if enabled is not None:
            enabled = np.ascontiguousarray(enabled, np.uint8).reshape(-1)
        if n and (len(targets) != n or (enabled is not None and len(enabled) != n)):
            raise ValueError(f"{len(targets)} targets and {None if enabled is None else len(enabled)} enabled bytes for {n} handles")
        return targets, enabled

    def step_ik(self, targets, enabled=None) -> None:
        """srt_pt_skin_step_ik: Skeleton::do_ik once - 50 iterations towards `targets` ((nhandles, 3), skeleton space) for the handles
        whose `enabled` byte is nonzero (None: all); uploads, runs the kernel, waits."""
        targets, enabled = self._handle_arrays(targets, enabled)
        self._check(self._lib, self._lib.srt_pt_skin_step_ik(self._h, _p(targets), None if enabled is None else _p(enabled)))

    def step_ik_device(self, d_targets_ptr: int, d_enabled_ptr: int = 0, stream: int = 0) -> None:
        """srt_pt_skin_step_ik_device: the same with targets (nhandles * 3 floats) and enabled bytes (0: all) in device memory; one
        launch, only enqueued."""
        self._check(self._lib, self._lib.srt_pt_skin_step_ik_device(self._h, c_void_p(stream), c_void_p(d_targets_ptr), c_void_p(d_enabled_ptr or None)))

    def posed_current(self) -> np.ndarray:
        """srt_pt_skin_posed_current: Skeleton::joint_to_posed of every joint from the current pose, (njoints, 16)."""
        out = np.zeros((self.njoints, 16), np.float32)
        self._check(self._lib, self._lib.srt_pt_skin_posed_current(self._h, _p(out)))
        return out

    def posed_current_device(self, d_posed_ptr: int, stream: int = 0) -> None:
        self._check(self._lib, self._lib.srt_pt_skin_posed_current_device(self._h, c_void_p(stream), c_void_p(d_posed_ptr)))

    def vertices_current_device(self, d_pos_ptr: int, d_nrm_ptr: int, flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_vertices_current_device: vertices_at_device from the current pose."""
        self._check(self._lib, self._lib.srt_pt_skin_vertices_current_device(self._h, c_void_p(stream), int(bool(flat_normals)), c_void_p(d_pos_ptr),
                                                                             c_void_p(d_nrm_ptr)))

    def pose_current(self, how: str = "inplace", flat_normals: bool = False, stream: int = 0) -> None:
        """srt_pt_skin_pose_current: pose_at ("update"), pose_refit_at ("refit") or pose_inplace_at ("inplace") from the current pose."""
        self._check(self._lib, self._lib.srt_pt_skin_pose_current(self._h, c_void_p(stream), int(bool(flat_normals)), self.HOW[how]))

    def close(self) -> None:
        if self._h:
            self._lib.srt_pt_skin_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if self._pt._ctx:                # (a skin is destroyed before its context; after it, there is nothing left to free safely)
                self.close()
        except Exception:
            pass


def _settle(members) -> None:
    """srt_pt_sync on every member (a Pathtracer each).  The group's lanes render on streams of their own, which nothing orders behind
    the stream an enqueue-only call was given: the group forms of such calls settle every member before they return."""
    for m in members:
        m.sync()


def _one_per_rank(ptrs, ranks: int, message: str = "{ranks} ranks but {got} device arrays") -> list:
    """The per-rank device pointers of a group call as a list, or ValueError when there is not one per rank."""
    ptrs = list(ptrs)
    if len(ptrs) != ranks:
        raise ValueError(message.format(ranks=ranks, got=len(ptrs)))
    return ptrs


def _handle_per_rank(make, *per_rank) -> list:
    """[make(*one of each per-rank list) for every rank]; when one fails the handles made so far are closed and the error goes on."""
    made = []
    try:
        for args in zip(*per_rank):
            made.append(make(*args))
    except Exception:
        for h in made:
            h.close()
        raise
    return made


class _HandleGroup:
    """What the handle groups of a PathtracerGroup share: one handle per rank (the scene is replicated), every rank gets the same calls
    (_all), rank 0 answers the read-backs (_first: the ranks hold the same bits)."""

    def __init__(self, handles):
        self._handles = handles

    def _all(self, name, *args, **kw):
        return [getattr(h, name)(*args, **kw) for h in self._handles]

    def _first(self, name, *args, **kw):
        return getattr(self._handles[0], name)(*args, **kw)

    def _settle(self) -> None:
        _settle(h._pt for h in self._handles)

    def close(self) -> None:
        self._all("close")


class SkinGroup(_HandleGroup):
    """PathtracerGroup.create_skin: one Skin per rank (the scene is replicated), posed together."""

    def __init__(self, skins):
        super().__init__(skins)
        self.skins = skins

    def map(self):
        return self._first("map")

    def vertices(self, posed, flat_normals: bool = False):
        return self._first("vertices", posed, flat_normals)

    def pose(self, posed, flat_normals: bool = False) -> None:
        self._all("pose", posed, flat_normals)

    def pose_refit(self, posed, flat_normals: bool = False) -> None:
        self._all("pose_refit", posed, flat_normals)

    def pose_inplace(self, posed, flat_normals: bool = False) -> None:
        """Skin.pose_inplace on every rank.  The group's lanes render on streams of their own, which nothing orders behind the
        pose's stream: every member is settled (srt_pt_sync) before this returns, as PathtracerGroup.set_active_device does and for
        the same reason.  A caller that wants the enqueue-only loop drives the members' skins and streams itself."""
        self._all("pose_inplace", posed, flat_normals)
        self._settle()

    def pose_inplace_at(self, t: float, flat_normals: bool = False) -> None:
        """Skin.pose_inplace_at on every rank with the same t; every member is settled before this returns (see pose_inplace)."""
        self._all("pose_inplace_at", t, flat_normals)
        self._settle()

    def set_rig(self, parent, base, rest_pose, knot_offsets, knot_times, knot_quats) -> None:
        self._all("set_rig", parent, base, rest_pose, knot_offsets, knot_times, knot_quats)

    def posed_at(self, t: float) -> np.ndarray:
        return self._first("posed_at", t)

    def pose_at(self, t: float, flat_normals: bool = False) -> None:
        """Every rank's skin takes the pose of the same time t."""
        self._all("pose_at", t, flat_normals)

    def pose_refit_at(self, t: float, flat_normals: bool = False) -> None:
        self._all("pose_refit_at", t, flat_normals)

    def set_ik_handles(self, joints) -> None:
        self._all("set_ik_handles", joints)

    def set_joint_pose(self, euler) -> None:
        self._all("set_joint_pose", euler)

    def joint_pose(self) -> np.ndarray:
        return self._first("joint_pose")

    def set_time(self, t: float) -> None:
        self._all("set_time", t)

    def step_ik(self, targets, enabled=None) -> None:
        """Every rank's skin takes the same step: the ranks' poses stay the same bits."""
        self._all("step_ik", targets, enabled)

    def step_ik_device(self, d_targets_ptrs, d_enabled_ptrs=None) -> None:
        """Skin.step_ik_device on every rank, with one device array per rank (ranks that share a device may share it)."""
        for r, k in enumerate(self.skins):
            k.step_ik_device(d_targets_ptrs[r], d_enabled_ptrs[r] if d_enabled_ptrs else 0)

    def posed_current(self) -> np.ndarray:
        return self._first("posed_current")

    def pose_current(self, how: str = "inplace", flat_normals: bool = False) -> None:
        """Skin.pose_current on every rank; with "inplace" every member is settled before this returns (see pose_inplace)."""
        self._all("pose_current", how, flat_normals)
        if how == "inplace":
            self._settle()


def timeline_tracks(tracks):
    """(track_offsets, knot_times, knot_values) from either that triple or a sequence with one entry per object, each
    (position, rotation, scale) with a track given as (times, values) or None: values (n, 3) for position and scale, (n, 4) xyzw
    quaternions for the rotation."""
    if isinstance(tracks, tuple) and len(tracks) == 3 and isinstance(tracks[0], np.ndarray) and tracks[0].ndim == 1 and tracks[0].dtype.kind in "ui":
        off, times, values = tracks
        return np.ascontiguousarray(off, np.uint32), _f32(times).reshape(-1), _f32(values).reshape(-1, 4)
    off, times, values = [0], [], []
    for obj in tracks:
        if len(obj) != 3:
            raise ValueError("an object has three tracks: position, rotation, scale")
        for track in obj:
            if track is not None:
                ts, vs = track
                vs = _f32(vs).reshape(len(ts), -1)
                times.extend(float(t) for t in ts)
                values.extend(np.concatenate([v, np.zeros(4 - len(v), np.float32)]) for v in vs)
            off.append(len(times))
    return np.array(off, np.uint32), np.array(times, np.float32), np.array(values, np.float32).reshape(-1, 4)


class Timeline:
    """srt_pt_timeline (Pathtracer.create_timeline): the Animate mode's keys of some objects of the committed scene, on the device.
    A frame is one float: transforms(t) / transforms_device(t) evaluate Anim_Pose::at(t) and Pose::transform() per object,
    repose_refit(t) / repose(t) hand the result to srt_pt_repose_refit_device / srt_pt_repose_device where it lies.  Closing the
    Pathtracer closes the timelines it created; close() after that does nothing."""

    def __init__(self, pt, handle, objects):
        self._pt, self._lib, self._check = pt, pt._lib, pt._check
        self._h = handle
        self.objects = objects

    def transforms(self, t: float) -> np.ndarray:
        """srt_pt_timeline_transforms: (nobjects, 16), computed on the host (works on a host-only context)."""
        out = np.zeros((len(self.objects), 16), np.float32)
        self._check(self._lib, self._lib.srt_pt_timeline_transforms(self._h, float(t), _p(out)))
        return out

    def transforms_device(self, t: float, d_trans_ptr: int, stream: int = 0) -> None:
        """srt_pt_timeline_transforms_device: the same by the kernel into a device array of nobjects * 16 floats; only enqueues."""
        self._check(self._lib, self._lib.srt_pt_timeline_transforms_device(self._h, c_void_p(stream), float(t), c_void_p(d_trans_ptr)))

    def repose_refit(self, t: float, stream: int = 0) -> None:
        """srt_pt_timeline_repose_refit: the poses of time t, then the BVH<Object> refitted in place - enqueue-only, nothing uploaded in
        the steady state."""
        self._check(self._lib, self._lib.srt_pt_timeline_repose_refit(self._h, c_void_p(stream), float(t)))

    def repose(self, t: float, stream: int = 0) -> None:
        """srt_pt_timeline_repose: the poses of time t, then the BVH<Object> rebuilt (srt_pt_repose_device)."""
        self._check(self._lib, self._lib.srt_pt_timeline_repose(self._h, c_void_p(stream), float(t)))

    def close(self) -> None:
        if self._h:
            self._lib.srt_pt_timeline_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if self._pt._ctx:                # (Pathtracer.close() has closed the timelines it made: after it there is nothing left to free)
                self.close()
        except Exception:
            pass


class TimelineGroup(_HandleGroup):
    """PathtracerGroup.create_timeline: one Timeline per rank (the scene is replicated); all ranks get the same t."""

    def __init__(self, timelines):
        super().__init__(timelines)
        self.timelines = timelines

    def transforms(self, t: float) -> np.ndarray:
        return self._first("transforms", t)

    def repose_refit(self, t: float, stream: int = 0) -> None:
        """Timeline.repose_refit on every rank; like PathtracerGroup.repose_refit_device each member is settled before this returns."""
        self._all("repose_refit", t, stream)
        self._settle()

    def repose(self, t: float, stream: int = 0) -> None:
        self._all("repose", t, stream)


class Emitter:
    """srt_pt_emitter (Pathtracer.create_emitter): the whole Scene_Particles::step for a pool of fixed capacity whose slots are objects of
    the committed scene - the substep loop, Particle::update against the collide context's scene, deaths, the spawns into the lowest
    dead slots, gen_instances - on one stream without a host wait.  Closing the Pathtracer closes the emitters it created."""

    def __init__(self, pt, collide, handle, objects):
        self._pt, self._collide, self._lib, self._check = pt, collide, pt._lib, pt._check
        self._h = handle
        self.objects = objects
        self.capacity = len(objects)

    def set_options(self, velocity: float = 25.0, angle: float = 0.0, scale: float = 0.1, lifetime: float = 15.0, pps: float = 5.0, dt: float = 0.01,
                    enabled: bool = False) -> None:
        """srt_pt_emitter_set_options: Scene_Particles::Options (the defaults are the reference's)."""
        self._check(self._lib, self._lib.srt_pt_emitter_set_options(self._h, float(velocity), float(angle), float(scale), float(lifetime), float(pps), float(dt),
                                                                   int(bool(enabled))))

    def set_pose(self, pos, euler) -> None:
        """srt_pt_emitter_set_pose: Scene_Particles::pose, position and Euler angles in degrees."""
        p, e = _f32(pos).reshape(3), _f32(euler).reshape(3)
        self._check(self._lib, self._lib.srt_pt_emitter_set_pose(self._h, _p(p), _p(e)))

    def seed(self, seed: int) -> None:
        self._check(self._lib, self._lib.srt_pt_emitter_seed(self._h, c_uint64(seed)))

    def set_uniforms_device(self, d_uniforms_ptr: int, n: int) -> None:
        """srt_pt_emitter_set_uniforms_device: n floats on the device, two per birth ordinal (0: back to the seeded generator)."""
        self._check(self._lib, self._lib.srt_pt_emitter_set_uniforms_device(self._h, c_void_p(d_uniforms_ptr), c_size_t(n)))

    def step_device(self, dt: float, stream: int = 0) -> None:
        """srt_pt_emitter_step_device: Scene_Particles::step(scene, dt) without gen_instances; only enqueues."""
        self._check(self._lib, self._lib.srt_pt_emitter_step_device(self._h, c_void_p(stream), float(dt)))

    def step(self, dt: float) -> None:
        self._check(self._lib, self._lib.srt_pt_emitter_step(self._h, float(dt)))

    def present_device(self, stream: int = 0) -> None:
        """srt_pt_emitter_present_device: gen_instances - the transforms, the active flags and the refit of the render scene; only enqueues."""
        self._check(self._lib, self._lib.srt_pt_emitter_present_device(self._h, c_void_p(stream)))

    def frame_device(self, dt: float, stream: int = 0) -> None:
        self._check(self._lib, self._lib.srt_pt_emitter_frame_device(self._h, c_void_p(stream), float(dt)))

    def clear_device(self, stream: int = 0) -> None:
        self._check(self._lib, self._lib.srt_pt_emitter_clear_device(self._h, c_void_p(stream)))

    def clear(self) -> None:
        self._check(self._lib, self._lib.srt_pt_emitter_clear(self._h))

    def read(self) -> dict:
        """srt_pt_emitter_read: {"pos", "vel" (capacity, 3), "age", "alive" (uint8), "birth" (uint32)}; blocking."""
        n = self.capacity
        out = {"pos": np.zeros((n, 3), np.float32), "vel": np.zeros((n, 3), np.float32), "age": np.zeros(n, np.float32), "alive": np.zeros(n, np.uint8),
               "birth": np.zeros(n, np.uint32)}
        self._check(self._lib, self._lib.srt_pt_emitter_read(self._h, _p(out["pos"]), _p(out["vel"]), _p(out["age"]), _p(out["alive"]), _p(out["birth"])))
        return out

    def write(self, pos=None, vel=None, age=None, alive=None, birth=None) -> None:
        """srt_pt_emitter_write: the arrays given (None: left as they are); blocking."""
        n = self.capacity
        arrays = []
        for a, dtype, shape in ((pos, np.float32, (n, 3)), (vel, np.float32, (n, 3)), (age, np.float32, (n,)), (alive, np.uint8, (n,)), (birth, np.uint32, (n,))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype)
                if a.shape != shape:
                    raise ValueError(f"an array of shape {a.shape} for a pool of {n} slots")
            arrays.append(a)
        self._check(self._lib, self._lib.srt_pt_emitter_write(self._h, *(None if a is None else _p(a) for a in arrays)))

    def counts(self) -> dict:
        """srt_pt_emitter_counts: {"alive", "born", "dropped"}; blocking."""
        out = np.zeros(3, np.uint64)
        self._check(self._lib, self._lib.srt_pt_emitter_counts(self._h, _p(out)))
        return {"alive": int(out[0]), "born": int(out[1]), "dropped": int(out[2])}

    def arrays_device(self) -> dict:
        """srt_pt_emitter_arrays_device: the device pointers of pos, vel, age, alive and birth."""
        out = (c_void_p * 5)()
        self._check(self._lib, self._lib.srt_pt_emitter_arrays_device(self._h, out))
        return {k: int(out[i] or 0) for i, k in enumerate(("pos", "vel", "age", "alive", "birth"))}

    def advance_host(self, dt: float):
        """srt_pt_emitter_advance_host (srt_pt_debug.h): the schedule half of step(dt) alone - (spawns per substep, cleared, (last_update, particle_cooldown))."""
        n, cleared = c_uint32(), c_int()
        spawns, sched = np.zeros(4096, np.uint32), np.zeros(2, np.float64)
        self._check(self._lib, self._lib.srt_pt_emitter_advance_host(self._h, float(dt), ctypes.byref(n), _p(spawns), len(spawns), ctypes.byref(cleared), _p(sched)))
        return spawns[:n.value].copy(), bool(cleared.value), (float(sched[0]), float(sched[1]))

    def close(self) -> None:
        if self._h:
            self._lib.srt_pt_emitter_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if self._pt._ctx and self._collide._ctx:      # (Pathtracer.close() has closed the emitters it made)
                self.close()
        except Exception:
            pass


class EmitterGroup(_HandleGroup):
    """PathtracerGroup.create_emitter: one Emitter per rank (the scene is replicated); every rank gets the same calls.  The device forms
    take one uniform buffer per rank."""

    def __init__(self, emitters):
        super().__init__(emitters)
        self.emitters = emitters
        self.capacity = emitters[0].capacity

    def set_options(self, *args, **kw) -> None:
        self._all("set_options", *args, **kw)

    def set_pose(self, pos, euler) -> None:
        self._all("set_pose", pos, euler)

    def seed(self, seed: int) -> None:
        self._all("seed", seed)

    def set_uniforms_device(self, d_uniforms_ptrs, n: int) -> None:
        for e, p in zip(self.emitters, _one_per_rank(d_uniforms_ptrs, len(self.emitters), "{got} uniform buffers for {ranks} ranks")):
            e.set_uniforms_device(p, n)

    def step_device(self, dt: float, stream: int = 0) -> None:
        self._all("step_device", dt, stream)

    def step(self, dt: float) -> None:
        self._all("step", dt)

    def present_device(self, stream: int = 0) -> None:
        """Emitter.present_device on every rank; like TimelineGroup.repose_refit each member is settled before this returns."""
        self._all("present_device", stream)
        self._settle()

    def frame_device(self, dt: float, stream: int = 0) -> None:
        self._all("frame_device", dt, stream)
        self._settle()

    def clear(self) -> None:
        self._all("clear")

    def read(self) -> dict:
        return self._first("read")

    def write(self, **arrays) -> None:
        self._all("write", **arrays)

    def counts(self) -> dict:
        return self._first("counts")


MATERIAL_DTYPE = np.dtype([("type", np.uint32), ("a", np.float32, 3), ("b", np.float32, 3), ("ior", np.float32)])   # srt_pt_material


def material_records(materials) -> np.ndarray:
    """srt_pt_material records from an array of MATERIAL_DTYPE or a sequence of dicts with type / a / b / ior (the scene descriptions' form)."""
    if isinstance(materials, np.ndarray) and materials.dtype == MATERIAL_DTYPE:
        return np.ascontiguousarray(materials).reshape(-1)
    out = np.zeros(len(materials), MATERIAL_DTYPE)
    for k, m in enumerate(materials):
        out[k] = (int(m["type"]), _f32(m["a"]), _f32(m.get("b", (0, 0, 0))), float(m.get("ior", 0.0)))
    return out


def shading_tracks(tracks):
    """(track_offsets, knot_times, knot_values) from either that triple or a flat sequence of tracks in the order of
    srt_pt_shading_timeline_create - six per material, six per light, two of the environment - each (times, values) or None, values
    (n, 1 .. 4)."""
    if isinstance(tracks, tuple) and len(tracks) == 3 and isinstance(tracks[0], np.ndarray) and tracks[0].ndim == 1 and tracks[0].dtype.kind in "ui":
        off, times, values = tracks
        return np.ascontiguousarray(off, np.uint32), _f32(times).reshape(-1), _f32(values).reshape(-1, 4)
    off, times, values = [0], [], []
    for track in tracks:
        if track is not None:
            ts, vs = track
            vs = _f32(vs).reshape(len(ts), -1)
            times.extend(float(t) for t in ts)
            values.extend(np.concatenate([v, np.zeros(4 - len(v), np.float32)]) for v in vs)
        off.append(len(times))
    return np.array(off, np.uint32), np.array(times, np.float32), np.array(values, np.float32).reshape(-1, 4)


class ShadingTimeline:
    """srt_pt_shading_timeline (Pathtracer.create_shading_timeline): the Animate mode's keys of some materials and delta lights of the
    committed scene (and of its environment light), on the device.  values(t) is the host form, update(t) hands it to
    update_materials / update_lights / update_env_light, apply(t) is the kernel: enqueue-only, nothing uploaded.  Closing the
    Pathtracer closes the timelines it created; close() after that does nothing."""

    def __init__(self, pt, handle, materials, lights, env):
        self._pt, self._lib, self._check = pt, pt._lib, pt._check
        self._h = handle
        self.materials, self.lights, self.env = materials, lights, bool(env)

    def values(self, t: float) -> dict:
        """srt_pt_shading_timeline_values: {"materials": MATERIAL_DTYPE (nmaterials) as update_materials takes them, "lights":
        float32 (nlights, 21) = radiance3, angle_bounds2, trans16, "env": float32 (3) or None}, computed on the host."""
        mats, lights, env = np.zeros(len(self.materials), MATERIAL_DTYPE), np.zeros((len(self.lights), 21), np.float32), np.zeros(3, np.float32)
        self._check(self._lib, self._lib.srt_pt_shading_timeline_values(self._h, float(t), _p(mats) if len(mats) else None, _p(lights) if len(lights) else None,
                                                                        _p(env) if self.env else None))
        return {"materials": mats, "lights": lights, "env": env if self.env else None}

    def update(self, t: float) -> None:
        """srt_pt_shading_timeline_update: the host form - values(t) through the update calls (waits, uploads the listed records)."""
        self._check(self._lib, self._lib.srt_pt_shading_timeline_update(self._h, float(t)))

    def apply(self, t: float, stream: int = 0) -> None:
        """srt_pt_shading_timeline_apply: one kernel on `stream` writes the listed records in place - enqueue-only, nothing uploaded."""
        self._check(self._lib, self._lib.srt_pt_shading_timeline_apply(self._h, c_void_p(stream), float(t)))

    def close(self) -> None:
        if self._h:
            self._lib.srt_pt_shading_timeline_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            if self._pt._ctx:                # (Pathtracer.close() has closed the timelines it made: after it there is nothing left to free)
                self.close()
        except Exception:
            pass


class ShadingTimelineGroup(_HandleGroup):
    """PathtracerGroup.create_shading_timeline: one ShadingTimeline per rank (the scene is replicated); all ranks get the same t."""

    def __init__(self, timelines):
        super().__init__(timelines)
        self.timelines = timelines

    def values(self, t: float) -> dict:
        return self._first("values", t)

    def update(self, t: float) -> None:
        self._all("update", t)

    def apply(self, t: float, stream: int = 0) -> None:
        """ShadingTimeline.apply on every rank; like TimelineGroup.repose_refit each member is settled before this returns (the
        group's lanes render on streams of their own, which nothing orders behind `stream`)."""
        self._all("apply", t, stream)
        self._settle()


class Scene:
    """A scene description (see scenes.py): materials, objects, camera — the inputs of build_scene."""

    def __init__(self, description: dict):
        self.description = description


class Pathtracer:
    """Mirror of PT::Pathtracer for the HIP path.

    Reference call sequence (gui/widgets.cpp:921-967): set_params(w, h, samples, depth, use_bvh) ->
    begin_render(scene, camera) -> poll in_progress()/progress() -> get_output().  Here begin_render is
    synchronous (the C++ drop-in keeps the reference's asynchronous worker); the epoch
    scheme is the reference's: samples_per_epoch = max(1, n / (n_threads * 10)), running mean of epoch
    means (rays/pathtracer.cpp:250-280, 195-207).

    device = -1 creates a host-only context: scene assembly and BVH inspection work, rendering raises.
    """

    def __init__(self, device: int = 0, n_threads: int | None = None, _borrowed_ctx=None):
        from . import SrtError, _check, load_library

        self._SrtError, self._check = SrtError, _check
        self._lib = load_library()
        self._ctx = c_void_p()
        self._borrowed = _borrowed_ctx is not None       # a member context of a PathtracerGroup: the group destroys it
        if self._borrowed:
            self._ctx = c_void_p(_borrowed_ctx)
        else:
            _check(self._lib, self._lib.srt_pt_create(device, ctypes.byref(self._ctx)))
        self.n_threads = n_threads or os.cpu_count() or 1
        self.out_w = self.out_h = 0
        self.n_samples = 0
        self.max_depth = 8
        self.scene_use_bvh = True
        self.accumulator = None
        self.accumulator_samples = 0
        self.total_epochs = self.completed_epochs = 0
        self.seed = 0
        self._sample_cursor = 0
        self._timelines = []                             # weak references: close() destroys the live ones before the context goes

    def close(self) -> None:
        if self._ctx:
            for ref in self._timelines:
                tl = ref()
                if tl is not None:
                    tl.close()
            self._timelines = []
            if not self._borrowed:
                self._lib.srt_pt_destroy(self._ctx)
            self._ctx = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- reference surface -------------------------------------------------------------------------
    def set_params(self, w: int, h: int, pixel_samples: int, depth: int, use_bvh: bool) -> None:
        self.out_w, self.out_h, self.n_samples, self.max_depth = int(w), int(h), int(pixel_samples), int(depth)
        self.scene_use_bvh = bool(use_bvh)
        self.accumulator = np.zeros((self.out_h, self.out_w, 3), np.float32)
        self._check(self._lib, self._lib.srt_pt_set_params(self._ctx, self.out_w, self.out_h, self.max_depth))

    def set_samples(self, samples: int) -> None:
        self.n_samples = int(samples)

    def build_scene(self, scene) -> None:
        d = scene.description if isinstance(scene, Scene) else scene
        L = self._lib
        self._check(L, L.srt_pt_scene_begin(self._ctx))
        for m in d["materials"]:
            pm = PtMaterial(int(m["type"]), (c_float * 3)(*[float(v) for v in m["a"]]), (c_float * 3)(*[float(v) for v in m["b"]]),
                            float(m["ior"]))
            self._check(L, L.srt_pt_add_material(self._ctx, ctypes.byref(pm), None))
        for o in d["objects"]:
            T = _f32(o["T"])
            if o["kind"] == "mesh":
                pos, nrm = _f32(o["pos"]), _f32(o["nrm"])
                idx = np.ascontiguousarray(o["idx"], np.uint32)
                self._check(L, L.srt_pt_add_mesh(self._ctx, _p(pos), _p(nrm), len(pos), _p(idx), len(idx), _p(T),
                                                 int(o["material"]), int(bool(o["is_light"]))))
            elif o["kind"] == "instance":      # {"kind": "instance", "of": insertion index of a mesh, "T", "material"} (scenes.share_meshes)
                self._check(L, L.srt_pt_add_instance(self._ctx, int(o["of"]), _p(T), int(o["material"])))
            elif o.get("light_mesh") is not None:   # emissive sphere
                lm = o["light_mesh"]
                pos, nrm, idx = _f32(lm["pos"]), _f32(lm["nrm"]), np.ascontiguousarray(lm["idx"], np.uint32)
                self._check(L, L.srt_pt_add_sphere_light(self._ctx, float(o["radius"]), _p(T), int(o["material"]), _p(pos), _p(nrm),
                                                         len(pos), _p(idx), len(idx)))
            else:
                self._check(L, L.srt_pt_add_sphere(self._ctx, float(o["radius"]), _p(T), int(o["material"])))
        if d.get("env"):               # {"type": 1 sphere | 2 hemisphere, "radiance"} or {"type": 3, "image": float32 [h, w, 3]}
            if int(d["env"]["type"]) == 3:
                img = _f32(d["env"]["image"])
                self._check(L, L.srt_pt_set_env_map(self._ctx, img.shape[1], img.shape[0], _p(img)))
            else:
                rad = _f32(d["env"]["radiance"])
                self._check(L, L.srt_pt_set_env_light(self._ctx, int(d["env"]["type"]), _p(rad)))
        for l in d.get("lights", []):   # delta lights (Pathtracer::build_lights): type 0 directional, 1 point, 2 spot
            rad, ab, T = _f32(l["radiance"]), _f32(l.get("angle_bounds", (0.0, 0.0))), _f32(l["T"])
            self._check(L, L.srt_pt_add_light(self._ctx, int(l["type"]), _p(rad), _p(ab), _p(T)))
        self._check(L, L.srt_pt_scene_commit(self._ctx, int(self.scene_use_bvh)))

    def repose(self, indices, Ts) -> None:
        """srt_pt_repose: new transforms (16 floats each, column-major) for the objects with these insertion indices of the
        committed scene - no BVH<Triangle> is rebuilt, no triangle uploaded."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        T = _f32(Ts).reshape(-1, 16)
        if len(T) != len(idx):
            raise ValueError(f"{len(idx)} objects but {len(T)} transforms")
        self._check(self._lib, self._lib.srt_pt_repose(self._ctx, _p(idx), _p(T), len(idx)))

    def repose_device(self, indices, d_trans_ptr: int, stream: int = 0) -> None:
        """srt_pt_repose_device: the same from a device array of len(indices) * 16 floats (e.g. tensor.data_ptr()), read on `stream`."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._lib, self._lib.srt_pt_repose_device(self._ctx, c_void_p(stream), _p(idx), c_void_p(d_trans_ptr), len(idx)))

    def repose_refit(self, indices, Ts) -> None:
        """srt_pt_repose_refit: new transforms for these objects with the BVH<Object> kept - same links and object order, new boxes;
        no build, no table of object order uploaded.  scene_tree_cost() tells when a rebuild (repose / repose_device) pays."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        T = _f32(Ts).reshape(-1, 16)
        if len(T) != len(idx):
            raise ValueError(f"{len(idx)} objects but {len(T)} transforms")
        self._check(self._lib, self._lib.srt_pt_repose_refit(self._ctx, _p(idx), _p(T), len(idx)))

    def repose_refit_device(self, indices, d_trans_ptr: int, stream: int = 0) -> None:
        """srt_pt_repose_refit_device: the same from a device array of len(indices) * 16 floats, only enqueued on `stream`: no wait,
        no read-back.  The host's record settles at the next call that is not enqueue-only (dump_bvh, hit, sync, ...)."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._lib, self._lib.srt_pt_repose_refit_device(self._ctx, c_void_p(stream), _p(idx), c_void_p(d_trans_ptr), len(idx)))

    def set_active(self, indices, flags) -> None:
        """srt_pt_set_active: switches the objects with these insertion indices off (flag 0) or on (non-zero) without committing
        again - an inactive object keeps its record and pose, and nothing that walks the BVH<Object> reaches it.  Blocks."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        if len(f) != len(idx):
            raise ValueError(f"{len(idx)} objects but {len(f)} flags")
        self._check(self._lib, self._lib.srt_pt_set_active(self._ctx, _p(idx), _p(f), len(idx)))

    def set_active_device(self, indices, d_active_ptr: int, stream: int = 0) -> None:
        """srt_pt_set_active_device: the same from a device array of len(indices) bytes (particles_step_device's d_alive), only
        enqueued on `stream`: no wait, no read-back.  The host's record settles as after repose_refit_device."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self._lib, self._lib.srt_pt_set_active_device(self._ctx, c_void_p(stream), _p(idx), c_void_p(d_active_ptr), len(idx)))

    def active(self) -> np.ndarray:
        """srt_pt_get_active: one uint8 per object in insertion order, 1 = active (after settling)."""
        n = int(self.scene_counts()["objects"])
        out = np.zeros(max(n, 1), np.uint8)
        self._check(self._lib, self._lib.srt_pt_get_active(self._ctx, _p(out), n))
        return out[:n]

    def scene_tree_cost(self) -> float:
        """srt_pt_scene_tree_cost: SAH cost of the current BVH<Object> (after settling)."""
        c = ctypes.c_double()
        self._check(self._lib, self._lib.srt_pt_scene_tree_cost(self._ctx, ctypes.byref(c)))
        return float(c.value)

    def top_refit_pending(self):
        """srt_pt_top_refit_pending: (device-form refits the host has not applied yet, entries of the set of objects they listed);
        does not settle."""
        out = np.zeros(2, np.uint64)
        self._check(self._lib, self._lib.srt_pt_top_refit_pending(self._ctx, _p(out)))
        return int(out[0]), int(out[1])

    def top_refit_count(self) -> int:
        """srt_pt_top_refit_count: the successful repose_refit / repose_refit_device calls since creation (after settling)."""
        r = c_uint64()
        self._check(self._lib, self._lib.srt_pt_top_refit_count(self._ctx, ctypes.byref(r)))
        return int(r.value)

    def particle_transforms_device(self, d_pos_ptr: int, n: int, scale: float, d_trans_ptr: int, stream: int = 0) -> None:
        """srt_pt_particle_transforms_device: translate(pos_k) * scale(scale) for n particles, device array (n, 3) -> device array
        (n, 16); only enqueued on `stream`."""
        self._check(self._lib, self._lib.srt_pt_particle_transforms_device(self._ctx, c_void_p(stream), c_void_p(d_pos_ptr), int(n), float(scale),
                                                                           c_void_p(d_trans_ptr)))

    def update_mesh(self, index: int, pos, nrm) -> None:
        """srt_pt_update_mesh: new vertex positions and normals ((nverts, 3) each, the count the mesh was added with) for the mesh
        object with this insertion index of the committed scene - one BVH<Triangle> is rebuilt, no other mesh is touched."""
        pos, nrm = _f32(pos).reshape(-1, 3), _f32(nrm).reshape(-1, 3)
        if len(pos) != len(nrm):
            raise ValueError(f"{len(pos)} positions but {len(nrm)} normals")
        self._check(self._lib, self._lib.srt_pt_update_mesh(self._ctx, int(index), _p(pos), _p(nrm), len(pos)))

    def update_mesh_device(self, index: int, d_pos_ptr: int, d_nrm_ptr: int, nverts: int, stream: int = 0) -> None:
        """srt_pt_update_mesh_device: the same from two device arrays of nverts * 3 floats (e.g. tensor.data_ptr())."""
        self._check(self._lib, self._lib.srt_pt_update_mesh_device(self._ctx, c_void_p(stream), int(index), c_void_p(d_pos_ptr), c_void_p(d_nrm_ptr), int(nverts)))

    def refit_mesh(self, index: int, pos, nrm) -> None:
        """srt_pt_refit_mesh: new vertex positions and normals for the mesh object with this insertion index, its BVH<Triangle> kept:
        same links and primitive order, new boxes - no build (in a scene without BVHs: update_mesh)."""
        pos, nrm = _f32(pos).reshape(-1, 3), _f32(nrm).reshape(-1, 3)
        if len(pos) != len(nrm):
            raise ValueError(f"{len(pos)} positions but {len(nrm)} normals")
        self._check(self._lib, self._lib.srt_pt_refit_mesh(self._ctx, int(index), _p(pos), _p(nrm), len(pos)))

    def refit_mesh_device(self, index: int, d_pos_ptr: int, d_nrm_ptr: int, nverts: int, stream: int = 0) -> None:
        """srt_pt_refit_mesh_device: the same from two device arrays of nverts * 3 floats (e.g. tensor.data_ptr())."""
        self._check(self._lib, self._lib.srt_pt_refit_mesh_device(self._ctx, c_void_p(stream), int(index), c_void_p(d_pos_ptr), c_void_p(d_nrm_ptr), int(nverts)))

    def refit_mesh_inplace(self, index: int, pos, nrm) -> None:
        """srt_pt_refit_mesh_inplace: refit_mesh with the BVH<Object> kept as well - it takes new boxes as in repose_refit, nothing is
        built and no table of object order goes up.  Blocks.  mesh_tree_cost() / scene_tree_cost() tell when a rebuild pays."""
        pos, nrm = _f32(pos).reshape(-1, 3), _f32(nrm).reshape(-1, 3)
        if len(pos) != len(nrm):
            raise ValueError(f"{len(pos)} positions but {len(nrm)} normals")
        self._check(self._lib, self._lib.srt_pt_refit_mesh_inplace(self._ctx, int(index), _p(pos), _p(nrm), len(pos)))

    def refit_mesh_inplace_device(self, index: int, d_pos_ptr: int, d_nrm_ptr: int, nverts: int, stream: int = 0) -> None:
        """srt_pt_refit_mesh_inplace_device: the same from two device arrays of nverts * 3 floats, only enqueued on `stream`: no wait,
        no read-back, and the arrays may be overwritten behind the call.  Non-finite vertices are NOT refused (the blocking forms
        check).  The host's record settles at the next call that is not enqueue-only (dump_bvh, hit, sync, ...)."""
        self._check(self._lib, self._lib.srt_pt_refit_mesh_inplace_device(self._ctx, c_void_p(stream), int(index), c_void_p(d_pos_ptr), c_void_p(d_nrm_ptr),
                                                                          int(nverts)))

    def mesh_refit_pending(self):
        """srt_pt_mesh_refit_pending: (refit_mesh_inplace_device calls the host has not applied yet, meshes they touched); does not settle."""
        out = np.zeros(2, np.uint64)
        self._check(self._lib, self._lib.srt_pt_mesh_refit_pending(self._ctx, _p(out)))
        return int(out[0]), int(out[1])

    def mesh_tree_cost(self, index: int) -> float:
        """srt_pt_mesh_tree_cost: SAH cost of the mesh's current BVH<Triangle> - compare before and after refits to decide when to rebuild."""
        c = ctypes.c_double()
        self._check(self._lib, self._lib.srt_pt_mesh_tree_cost(self._ctx, int(index), ctypes.byref(c)))
        return float(c.value)

    def create_skin(self, index: int, bind_pos, bind_nrm, joints) -> Skin:
        """srt_pt_skin_create: Skeleton::find_joints for the mesh object with this insertion index of the committed scene, from its
        bind-pose arrays ((nverts, 3) each) and its joints (skin_joints(..)) in Skeleton::for_joints order."""
        pos, nrm = _f32(bind_pos).reshape(-1, 3), _f32(bind_nrm).reshape(-1, 3)
        if len(pos) != len(nrm):
            raise ValueError(f"{len(pos)} positions but {len(nrm)} normals")
        J = skin_joints(joints)
        h = c_void_p()
        self._check(self._lib, self._lib.srt_pt_skin_create(self._ctx, int(index), _p(pos), _p(nrm), len(pos), _p(J), len(J), ctypes.byref(h)))
        return Skin(self, h, len(pos), len(J))

    def create_timeline(self, objects, tracks) -> Timeline:
        """srt_pt_timeline_create: keys for the objects with these insertion indices of the committed scene (timeline_tracks(..) says
        how `tracks` may be given); the tables go up once."""
        idx = np.ascontiguousarray(objects, np.uint32).reshape(-1)
        off, times, values = timeline_tracks(tracks)
        if len(off) != 3 * len(idx) + 1 or len(times) != len(values) or int(off.max()) > len(times):
            raise ValueError(f"{len(idx)} objects, {len(off)} offsets up to {int(off.max())}, {len(times)} knot times, {len(values)} knot values")
        if len(times) == 0:
            times, values = np.zeros(1, np.float32), np.zeros((1, 4), np.float32)
        h = c_void_p()
        self._check(self._lib, self._lib.srt_pt_timeline_create(self._ctx, _p(idx if len(idx) else np.zeros(1, np.uint32)), len(idx), _p(off), _p(times), _p(values),
                                                                ctypes.byref(h)))
        tl = Timeline(self, h, idx)
        self._timelines = [r for r in self._timelines if r() is not None] + [weakref.ref(tl)]
        return tl

    def create_emitter(self, collide, objects, radius: float) -> Emitter:
        """srt_pt_emitter_create: an emitter over the pool `objects` (insertion indices of this context's committed scene, one per slot)
        whose particles bounce off the committed scene of the Pathtracer `collide` - the reference's Simulate scene when that holds the
        Scene_Objects only; `collide` may be this Pathtracer.  Closing either Pathtracer closes the emitter."""
        idx = np.ascontiguousarray(objects, np.uint32).reshape(-1)
        h = c_void_p()
        self._check(self._lib, self._lib.srt_pt_emitter_create(self._ctx, collide._ctx if collide is not None else None, _p(idx) if len(idx) else None, len(idx),
                                                               float(radius), ctypes.byref(h)))
        em = Emitter(self, collide, h, idx)
        for pt in {id(self): self, id(collide): collide}.values():
            pt._timelines = [r for r in pt._timelines if r() is not None] + [weakref.ref(em)]
        return em

    def update_materials(self, indices, materials) -> None:
        """srt_pt_update_materials: new values (material_records(..): the form build_scene takes) for the materials with these indices
        of the committed scene; the types stay.  No commit: 32 B per material go up."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        recs = material_records(materials)
        if len(recs) != len(idx):
            raise ValueError(f"{len(idx)} indices but {len(recs)} materials")
        self._check(self._lib, self._lib.srt_pt_update_materials(self._ctx, _p(idx), _p(recs), len(idx)))

    def update_lights(self, indices, radiance, angle_bounds, Ts) -> None:
        """srt_pt_update_lights: new radiance (n, 3), angle_bounds (n, 2) or None, and transforms (n, 16) for the delta lights with
        these indices (the order of the scene's "lights"); the types stay.  No commit: 160 B per light go up."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        rad, T = _f32(radiance).reshape(-1, 3), _f32(Ts).reshape(-1, 16)
        ab = None if angle_bounds is None else _f32(angle_bounds).reshape(-1, 2)
        if len(rad) != len(idx) or len(T) != len(idx) or (ab is not None and len(ab) != len(idx)):
            raise ValueError(f"{len(idx)} lights but {len(rad)} radiances, {len(T)} transforms")
        self._check(self._lib, self._lib.srt_pt_update_lights(self._ctx, _p(idx), _p(rad), None if ab is None else _p(ab), _p(T), len(idx)))

    def update_env_light(self, radiance) -> None:
        """srt_pt_update_env_light: a new radiance for a sphere / hemisphere environment light, in effect from the next launch."""
        rad = _f32(radiance).reshape(3)
        self._check(self._lib, self._lib.srt_pt_update_env_light(self._ctx, _p(rad)))

    def dump_shading(self, from_device: bool = False) -> dict:
        """srt_pt_dump_shading: {"materials": MATERIAL_DTYPE records as the kernels read them, "light_heads": uint32 (lights, 2) = type,
        has_trans, "lights": float32 (lights, 37) = radiance3, angle_bounds2, trans16, itrans16, "env_type", "env_radiance"} from the
        host's record or read back from the device."""
        counts, env_type, env = np.zeros(2, np.uint32), c_uint32(0), np.zeros(3, np.float32)

        def call(mats, heads, values):
            self._check(self._lib, self._lib.srt_pt_dump_shading(self._ctx, int(bool(from_device)), _p(counts), _p(mats) if len(mats) else None, len(mats),
                                                                 _p(heads) if len(heads) else None, _p(values) if len(heads) else None, len(heads),
                                                                 ctypes.byref(env_type), _p(env)))

        call(np.zeros(0, MATERIAL_DTYPE), np.zeros((0, 2), np.uint32), np.zeros((0, 37), np.float32))
        mats, heads, values = np.zeros(int(counts[0]), MATERIAL_DTYPE), np.zeros((int(counts[1]), 2), np.uint32), np.zeros((int(counts[1]), 37), np.float32)
        call(mats, heads, values)
        return {"materials": mats, "light_heads": heads, "lights": values, "env_type": int(env_type.value), "env_radiance": env}

    def create_shading_timeline(self, materials, lights, env, tracks) -> ShadingTimeline:
        """srt_pt_shading_timeline_create: keys for the materials and delta lights with these indices of the committed scene and, with
        env, for its environment light (shading_tracks(..) says how `tracks` may be given); the tables go up once."""
        mats, lts = np.ascontiguousarray(materials, np.uint32).reshape(-1), np.ascontiguousarray(lights, np.uint32).reshape(-1)
        off, times, values = shading_tracks(tracks)
        want = 6 * len(mats) + 6 * len(lts) + (2 if env else 0) + 1
        if len(off) != want or len(times) != len(values) or int(off.max()) > len(times):
            raise ValueError(f"{len(mats)} materials, {len(lts)} lights, env {bool(env)}: {want} offsets expected, {len(off)} given up to {int(off.max())}, "
                             f"{len(times)} knot times, {len(values)} knot values")
        if len(times) == 0:
            times, values = np.zeros(1, np.float32), np.zeros((1, 4), np.float32)
        h = c_void_p()
        self._check(self._lib, self._lib.srt_pt_shading_timeline_create(self._ctx, _p(mats) if len(mats) else None, len(mats), _p(lts) if len(lts) else None, len(lts),
                                                                        int(bool(env)), _p(off), _p(times), _p(values), ctypes.byref(h)))
        tl = ShadingTimeline(self, h, mats, lts, env)
        self._timelines = [r for r in self._timelines if r() is not None] + [weakref.ref(tl)]
        return tl

    def math_hypot(self, x, y):
        """srt_pt_math_hypot: the kernels' hypotf on the device."""
        x, y = _f32(x).reshape(-1), _f32(y).reshape(-1)
        out = np.zeros(len(x), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_hypot(self._ctx, _p(x), _p(y), len(x), _p(out)))
        return out

    def scene_counts(self) -> dict:
        """srt_pt_scene_counts: what the scene stores, the BVH<Triangle> builds so far and the bytes uploaded, and srt_pt_refit_count's
        refits (SCENE_COUNT_NAMES)."""
        out = np.zeros(8, np.uint64)
        self._check(self._lib, self._lib.srt_pt_scene_counts(self._ctx, _p(out)))
        refits = c_uint64()
        self._check(self._lib, self._lib.srt_pt_refit_count(self._ctx, ctypes.byref(refits)))
        return dict(zip(SCENE_COUNT_NAMES, [int(v) for v in out] + [int(refits.value)]))

    def set_camera(self, camera: dict) -> None:
        iv = _f32(camera["iview"])
        self._check(self._lib, self._lib.srt_pt_set_camera(self._ctx, _p(iv), float(camera["vfov"]), float(camera["ar"])))

    def begin_render(self, scene, camera: dict | None = None, add_samples: bool = False, samples_per_epoch: int | None = None) -> None:
        d = scene.description if isinstance(scene, Scene) else scene
        spe = samples_per_epoch or max(1, self.n_samples // (self.n_threads * 10))
        self.total_epochs = self.n_samples // spe + (1 if self.n_samples % spe else 0)
        self.completed_epochs = 0
        if not add_samples:
            self.accumulator[...] = 0
            self.accumulator_samples = 0
            self._sample_cursor = 0
            self.build_scene(d)
        self.set_camera(camera or d["camera"])
        s = 0
        while s < self.n_samples:
            n = min(spe, self.n_samples - s)
            epoch = self.render_epoch(self.seed, self._sample_cursor, n)
            self.accumulate(epoch)
            self._sample_cursor += n
            self.completed_epochs += 1
            s += n

    def accumulate(self, sample: np.ndarray) -> None:
        """rays/pathtracer.cpp:195-207 on the host copy (the device form is srt_pt_accumulate_device)."""
        self.accumulator_samples += 1
        inv = np.float32(1.0) / np.float32(self.accumulator_samples)
        self.accumulator += ((sample - self.accumulator).astype(np.float32) * inv).astype(np.float32)

    def in_progress(self) -> bool:
        return self.completed_epochs < self.total_epochs

    def progress(self) -> float:
        return self.completed_epochs / self.total_epochs if self.total_epochs else 0.0

    def get_output(self) -> np.ndarray:
        return self.accumulator

    def cancel(self) -> None:
        self.completed_epochs = self.total_epochs = 0

    # -- C-ABI steps ---------------------------------------------------------------------------------
    def set_tiling(self, tile_w: int, tile_h: int, rank: int, world: int) -> None:
        self._check(self._lib, self._lib.srt_pt_set_tiling(self._ctx, tile_w, tile_h, rank, world))

    def tile_info(self):
        a, b, c = c_uint32(), c_uint32(), c_uint32()
        self._check(self._lib, self._lib.srt_pt_tile_info(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def render_epoch(self, seed: int, sample_base: int, samples: int, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((self.out_h, self.out_w, 3), np.float32)
        st = self._lib.srt_pt_render_epoch(self._ctx, seed, sample_base, samples, _p(out))
        if st == SRT_CANCELLED:
            raise SrtCancelled()
        self._check(self._lib, st)
        return out

    def render_epoch_device(self, stream: int, seed: int, sample_base: int, samples: int, d_tiles_out: int) -> None:
        st = self._lib.srt_pt_render_epoch_device(self._ctx, c_void_p(stream), seed, sample_base, samples, c_void_p(d_tiles_out))
        if st == SRT_CANCELLED:
            raise SrtCancelled()
        self._check(self._lib, st)

    # -- Pathtracer::cancel / Pathtracer::log_ray on the C ABI ------------------------------------------
    def cancel_device(self) -> None:
        """srt_pt_cancel: may be called from another thread while render_epoch runs."""
        self._check(self._lib, self._lib.srt_pt_cancel(self._ctx))

    def cancel_requested(self) -> bool:
        return bool(self._lib.srt_pt_cancel_requested(self._ctx))

    def clear_cancel(self) -> None:
        self._check(self._lib, self._lib.srt_pt_clear_cancel(self._ctx))

    def set_ray_log(self, capacity: int) -> None:
        self._check(self._lib, self._lib.srt_pt_set_ray_log(self._ctx, int(capacity)))

    def read_ray_log(self, stream: int | None = None):
        """(rays as a LOGGED_RAY_DTYPE array in log order, dropped): what Pathtracer::log_ray received since the last read."""
        n, dropped = c_size_t(), c_uint64()
        if stream is None:
            self._check(self._lib, self._lib.srt_pt_read_ray_log(self._ctx, None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        else:
            self._check(self._lib, self._lib.srt_pt_read_ray_log_stream(self._ctx, c_void_p(stream), None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        out = np.zeros(n.value, LOGGED_RAY_DTYPE)
        got = c_size_t()
        if stream is None:
            self._check(self._lib, self._lib.srt_pt_read_ray_log(self._ctx, _p(out) if n.value else None, n.value, ctypes.byref(got), ctypes.byref(dropped)))
        else:
            self._check(self._lib, self._lib.srt_pt_read_ray_log_stream(self._ctx, c_void_p(stream), _p(out) if n.value else None, n.value,
                                                                        ctypes.byref(got), ctypes.byref(dropped)))
        return out[:got.value], int(dropped.value)

    def untile_device(self, stream: int, d_gathered: int, d_image: int) -> None:
        self._check(self._lib, self._lib.srt_pt_untile_device(self._ctx, c_void_p(stream), c_void_p(d_gathered), c_void_p(d_image)))

    def accumulate_device(self, stream: int, d_acc: int, d_epoch: int, nfloats: int, k: int) -> None:
        self._check(self._lib, self._lib.srt_pt_accumulate_device(self._ctx, c_void_p(stream), c_void_p(d_acc), c_void_p(d_epoch), nfloats, k))

    # -- launches decoupled from the reference's epochs (include/srt_pt.h) -----------------------------------
    def max_samples_per_launch(self) -> int:
        m = c_uint32()
        self._check(self._lib, self._lib.srt_pt_max_samples_per_launch(self._ctx, ctypes.byref(m)))
        return int(m.value)

    def accumulator_floats(self) -> int:
        """Floats of the device accumulator a fold keeps (8 per pixel slot of this rank's tiles: running mean, epoch in progress)."""
        n = c_size_t()
        self._check(self._lib, self._lib.srt_pt_accumulator_floats(self._ctx, ctypes.byref(n)))
        return int(n.value)

    def render_samples_device(self, stream: int, seed: int, base: int, n: int) -> None:
        """One launch of n samples per pixel into `stream`'s sample buffer (srt_pt_fold_epochs_device folds it). No wait."""
        st = self._lib.srt_pt_render_samples_device(self._ctx, c_void_p(stream), seed, base, n)
        if st == SRT_CANCELLED:
            raise SrtCancelled()
        self._check(self._lib, st)

    def fold_epochs_device(self, stream: int, spe: int, position: int, total: int, first_k: int, d_acc: int) -> None:
        """do_trace's epoch means and accumulate's running mean over the last launch on `stream`, into the device accumulator d_acc."""
        self._check(self._lib, self._lib.srt_pt_fold_epochs_device(self._ctx, c_void_p(stream), spe, position, total, first_k, c_void_p(d_acc)))

    def accumulator_tiles_device(self, stream: int, d_acc: int, d_tiles: int) -> None:
        """The running mean in d_acc as tile radiance (the layout of render_epoch_device)."""
        self._check(self._lib, self._lib.srt_pt_accumulator_tiles_device(self._ctx, c_void_p(stream), c_void_p(d_acc), c_void_p(d_tiles)))

    def set_stream_slots(self, slots: int) -> None:
        """Paths in flight per launch of the streamed forms (0 = default); the image does not depend on it."""
        self._check(self._lib, self._lib.srt_pt_set_stream_slots(self._ctx, int(slots)))

    def set_bvh_builder(self, device: bool, min_primitives: int = 16384) -> None:
        """Where build_scene runs BVH::build: on the GPU for primitive sets of at least `min_primitives`, else on the host."""
        self._check(self._lib, self._lib.srt_pt_set_bvh_builder(self._ctx, int(bool(device)), int(min_primitives)))

    def set_kernel(self, mode: int) -> None:
        """0 auto, 1 lane per pixel, 2 wave-uniform sweeps, 3 the same with section stamps, 4 lane per sample,
        5 persistent waves with the flattened per-lane walk, 6 streamed form: logic + ray-cast kernels (include/srt_pt.h)."""
        self._check(self._lib, self._lib.srt_pt_set_kernel(self._ctx, int(mode)))

    def section_cycles(self, reset: bool = False) -> dict:
        out = np.zeros(8, np.uint64)
        self._check(self._lib, self._lib.srt_pt_section_cycles(self._ctx, _p(out), int(reset)))
        names = ("refill", "top_down", "leaf_objects", "combine", "finish_direct", "shade", "terminate")
        return dict(zip(names, (int(v) for v in out)))

    def kernel_time(self, enable: bool = True):
        """(total_ms, launches) of the dominant kernel since the previous call (HIP events on the launch stream,
        recorded inside the library); then switches recording on/off."""
        ms, n = ctypes.c_double(), c_uint64()
        self._check(self._lib, self._lib.srt_pt_kernel_time(self._ctx, int(enable), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def stream_times(self, enable: bool = True):
        """({"logic_ms", "compact_ms", "cast_ms", "probe_ms"}, generations) of the streamed forms since the previous call; then
        recording on/off.  logic_ms is the resolve kernel where a generation's logic is split in two (probe_ms is 0 otherwise)."""
        ms = np.zeros(4, np.float64)
        g = c_uint64()
        self._check(self._lib, self._lib.srt_pt_stream_times(self._ctx, int(enable), _p(ms), ctypes.byref(g)))
        return {"logic_ms": float(ms[0]), "compact_ms": float(ms[1]), "cast_ms": float(ms[2]), "probe_ms": float(ms[3])}, int(g.value)

    def stream_counters(self, reset: bool = False) -> dict:
        """Streamed forms: entries queued to the ray-cast kernel and alive path-slot generations since the last reset, and the bytes per unit."""
        out = np.zeros(4, np.uint64)
        self._check(self._lib, self._lib.srt_pt_stream_counters(self._ctx, _p(out), int(reset)))
        return {"entries_queued": int(out[0]), "alive_slot_generations": int(out[1]), "bytes_per_alive_slot_generation": int(out[2]),
                "bytes_per_queued_entry": int(out[3])}

    def kernel_form(self) -> int:
        """Form render_epoch takes for the committed scene: 0 / 1 persistent sweeps (1: inline mesh walks), 2 flattened walk,
        3 streamed, 4 streamed sweeps, -1 lane per sample, -2 lane per pixel; -3 while set_normal_colors is on."""
        f = c_int()
        self._check(self._lib, self._lib.srt_pt_kernel_form(self._ctx, ctypes.byref(f)))
        return int(f.value)

    def ray_count(self, reset: bool = False):
        """(rays, camera_samples) traced by render_epoch* since the last reset (synchronizes the device)."""
        r, c = c_uint64(), c_uint64()
        self._check(self._lib, self._lib.srt_pt_ray_count(self._ctx, ctypes.byref(r), ctypes.byref(c), int(reset)))
        return r.value, c.value

    def trace_samples(self, seed: int, xs, ys, ss):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        rgb = np.zeros((len(xs), 3), np.float32)
        draws = np.zeros(len(xs), np.uint32)
        rays = np.zeros(len(xs), np.uint32)
        self._check(self._lib, self._lib.srt_pt_trace_samples(self._ctx, seed, _p(xs), _p(ys), _p(ss), len(xs), _p(rgb), _p(draws), _p(rays)))
        return rgb, draws, rays

    def counters(self) -> dict:
        out = np.zeros(8, np.uint64)
        self._check(self._lib, self._lib.srt_pt_counters(self._ctx, _p(out)))
        return dict(zip(COUNTER_NAMES, (int(v) for v in out)))

    def hit(self, org, dirs, bounds) -> np.ndarray:
        org, dirs, bounds = _f32(org), _f32(dirs), _f32(bounds)
        out = np.zeros((len(org), 9), np.float32)
        self._check(self._lib, self._lib.srt_pt_hit(self._ctx, _p(org), _p(dirs), _p(bounds), len(org), _p(out)))
        return out

    def hit_device(self, d_org_ptr: int, d_dirs_ptr: int, d_bounds_ptr: int, n: int, d_out9_ptr: int = 0, d_ids_ptr: int = 0, d_hit_ptr: int = 0,
                   stream: int = 0) -> None:
        """srt_pt_hit_device: scene.hit for n rays in device memory ((n, 3), (n, 3) float32 and (n, 2) float32 or 0 for {0, inf}), only
        enqueued on `stream`: no wait, nothing comes back to the host, the live device scene is read.  Outputs (each optional, not all
        three 0): (n, 9) float32 records as hit() returns them, (n, 2) uint32 {object insertion index, triangle's place in the mesh's
        primitive order}, (n,) uint8 hit flags."""
        self._check(self._lib, self._lib.srt_pt_hit_device(self._ctx, c_void_p(stream), c_void_p(d_org_ptr), c_void_p(d_dirs_ptr), c_void_p(d_bounds_ptr),
                                                           int(n), c_void_p(d_out9_ptr), c_void_p(d_ids_ptr), c_void_p(d_hit_ptr)))

    def hit_tensors(self, org, dirs, bounds=None, ids: bool = False, flags: bool = False):
        """hit_device for float32 CUDA tensors on the context's device ((n, 3), (n, 3), optionally (n, 2)), enqueued on torch's
        current stream.  Returns the (n, 9) records, then the (n, 2) int32 ids and the (n,) uint8 flags where asked for (a tuple
        then) - without synchronising: they are ordered behind the query on that stream."""
        import torch

        n = int(org.shape[0])
        for name, t, cols in (("org", org, 3), ("dirs", dirs, 3), ("bounds", bounds, 2)):
            if t is None:
                continue
            if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (n, cols) or not t.is_contiguous() or t.device != org.device:
                raise ValueError(f"hit_tensors: {name} must be a contiguous float32 CUDA tensor of shape ({n}, {cols}) on {org.device}")
        with torch.cuda.device(org.device):
            out = torch.empty((n, 9), dtype=torch.float32, device=org.device)
            d_ids = torch.empty((n, 2), dtype=torch.int32, device=org.device) if ids else None   # (the words of the uint32 pairs; -1: none)
            d_flags = torch.empty((n,), dtype=torch.uint8, device=org.device) if flags else None
            self.hit_device(org.data_ptr(), dirs.data_ptr(), bounds.data_ptr() if bounds is not None else 0, n, out.data_ptr(),
                            d_ids.data_ptr() if ids else 0, d_flags.data_ptr() if flags else 0, stream=torch.cuda.current_stream().cuda_stream)
        res = (out,) + ((d_ids,) if ids else ()) + ((d_flags,) if flags else ())
        return res[0] if len(res) == 1 else res

    def hit_device_paths(self):
        """srt_pt_hit_device_paths: hit_device calls so far through (the ray-cast kernel, the nested per-lane walk, the flattened one)."""
        out = np.zeros(3, np.uint64)
        self._check(self._lib, self._lib.srt_pt_hit_device_paths(self._ctx, _p(out)))
        return tuple(int(v) for v in out)

    def particles_step(self, pos, vel, age, dt: float, radius: float):
        """Scene_Particles::Particle::update for every particle (scene/particles.cpp:134-138): returns (pos, vel, age, alive)."""
        pos, vel, age = _f32(pos).copy(), _f32(vel).copy(), _f32(age).copy()
        alive = np.zeros(len(age), np.uint8)
        self._check(self._lib, self._lib.srt_pt_particles_step(self._ctx, _p(pos), _p(vel), _p(age), len(age), float(dt), float(radius), _p(alive)))
        return pos, vel, age, alive

    def particles_step_device(self, d_pos_ptr: int, d_vel_ptr: int, d_age_ptr: int, n: int, dt: float, radius: float, d_alive_ptr: int, stream: int = 0) -> None:
        """srt_pt_particles_step_device: the same in place on device arrays ((n, 3), (n, 3), (n,) float32 and (n,) uint8); only
        enqueued on `stream`."""
        self._check(self._lib, self._lib.srt_pt_particles_step_device(self._ctx, c_void_p(stream), c_void_p(d_pos_ptr), c_void_p(d_vel_ptr), c_void_p(d_age_ptr),
                                                                      int(n), float(dt), float(radius), c_void_p(d_alive_ptr)))

    def dump_bvh(self, which: int, cap: int = 1 << 22):
        boxes = np.zeros((cap, 6), np.float32)
        links = np.zeros((cap, 4), np.uint32)
        order = np.zeros(cap * 4, np.uint32)
        n = self._lib.srt_pt_dump_bvh(self._ctx, which, _p(boxes), _p(links), cap, _p(order))
        if n < 0:
            raise self._SrtError(int(n), self._lib.srt_last_error().decode())
        return boxes[:n].copy(), links[:n].copy(), order

    def math_acos(self, x):
        x = _f32(x)
        out = np.zeros(len(x), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_acos(self._ctx, _p(x), len(x), _p(out)))
        return out

    def math_atan2(self, y, x):
        y, x = _f32(y), _f32(x)
        out = np.zeros(len(y), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_atan2(self._ctx, _p(y), _p(x), len(y), _p(out)))
        return out

    def set_elision(self, on: bool) -> None:
        """Let the wave kernel skip the provably dead BSDF-sampled direct ray (include/srt_pt.h); images stay bit-identical."""
        self._check(self._lib, self._lib.srt_pt_set_elision(self._ctx, int(bool(on))))

    def set_normal_colors(self, on: bool) -> None:
        """The reference's debug_data.normal_colors: every render call takes the first-hit kernel and a sample is
        Spectrum::direction(normal) of the camera ray's hit (include/srt_pt.h).  Takes effect at the next launch."""
        self._check(self._lib, self._lib.srt_pt_set_normal_colors(self._ctx, int(bool(on))))

    ENV_SAMPLING = ("uniform", "image")

    def set_env_sampling(self, mode: str) -> None:
        """srt_pt_set_env_sampling: "uniform" (the default) or "image" - Env_Map's importance sampler, Samplers::Sphere::Image of the
        reference bit for bit, quirks included (include/srt_pt.h).  Takes effect at the next launch; a launch with "image" and an
        environment that is no map is refused."""
        if mode not in self.ENV_SAMPLING:
            raise ValueError(f"env sampling mode {mode!r}: one of {self.ENV_SAMPLING}")
        self._check(self._lib, self._lib.srt_pt_set_env_sampling(self._ctx, self.ENV_SAMPLING.index(mode)))

    def env_sampling(self) -> str:
        mode = c_uint32(0)
        self._check(self._lib, self._lib.srt_pt_env_sampling(self._ctx, ctypes.byref(mode)))
        return self.ENV_SAMPLING[mode.value]

    def math_sin_unit(self, x):
        """srt_pt_math_sin_unit: the kernels' double sin of floats in [0, 1], as float64."""
        x = _f32(x)
        out = np.zeros(len(x), np.float64)
        self._check(self._lib, self._lib.srt_pt_math_sin_unit(self._ctx, _p(x), len(x), _p(out)))
        return out

    def dump_env_sampler(self, from_device: bool = False) -> dict:
        """srt_pt_dump_env_sampler: {"w", "h", "total", "cdf", "pdf" (h * w each), "sin_theta", "cos_theta" (h + 1), "cos_phi",
        "sin_phi" (w)} of the environment map's Samplers::Sphere::Image, from the host's or the device's tables."""
        dims, total = np.zeros(2, np.uint32), ctypes.c_float(0)
        self._check(self._lib, self._lib.srt_pt_dump_env_sampler(self._ctx, int(from_device), _p(dims), ctypes.byref(total), None, None, 0, None, 0))
        w, h = int(dims[0]), int(dims[1])
        cdf, pdf, trig = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32), np.zeros(2 * (h + 1) + 2 * w, np.float64)
        self._check(self._lib, self._lib.srt_pt_dump_env_sampler(self._ctx, int(from_device), _p(dims), ctypes.byref(total), _p(cdf), _p(pdf),
                                                                  w * h, _p(trig), len(trig)))
        return {"w": w, "h": h, "total": np.float32(total.value), "cdf": cdf, "pdf": pdf, "sin_theta": trig[:h + 1].copy(),
                "cos_theta": trig[h + 1:2 * h + 2].copy(), "cos_phi": trig[2 * h + 2:2 * h + 2 + w].copy(), "sin_phi": trig[2 * h + 2 + w:].copy()}

    def env_sampler_probe(self, u=(), dirs=()):
        """srt_pt_env_sampler_probe: (index, direction (n, 3)) of sample() for each draw u, and pdf() of each direction, by a kernel."""
        u = _f32(u).reshape(-1)
        dirs = np.ascontiguousarray(_f32(dirs).reshape(-1, 3))
        index, out, pdf = np.zeros(len(u), np.uint32), np.zeros((len(u), 3), np.float32), np.zeros(len(dirs), np.float32)
        self._check(self._lib, self._lib.srt_pt_env_sampler_probe(self._ctx, _p(u), len(u), _p(index), _p(out), _p(dirs), len(dirs), _p(pdf)))
        return index, out, pdf

    def set_dynamic_lights(self, on: bool) -> None:
        """srt_pt_set_dynamic_lights: repose / update_mesh / refit_mesh / create_skin (and their device forms) accept area lights and
        keep the light tables what a fresh commit would make them.  Off by default; before or after build_scene."""
        self._check(self._lib, self._lib.srt_pt_set_dynamic_lights(self._ctx, int(bool(on))))

    def dump_lights(self, from_device: bool = False) -> dict:
        """srt_pt_dump_lights: {"heads": uint32 (lights, 4) = has_trans, first light triangle, triangle count, insertion index;
        "mats": float32 (lights, 4, 16) = trans, itrans, pdfT, pdfiT; "tris": float32 (light triangles, 31) = v0 v1 v2 (four floats
        each), area_term, p0 e1 e2, n0 n1 n2} from the host's mirror or read back from the device."""
        def call(heads, mats, nl, tris, nt):
            n = self._lib.srt_pt_dump_lights(self._ctx, int(bool(from_device)), _p(heads) if nl else None, _p(mats) if nl else None, nl,
                                             _p(tris) if nt else None, nt)
            if n < 0:
                raise self._SrtError(int(n), self._lib.srt_last_error().decode())
            return int(n)

        nl = call(None, None, 0, None, 0)
        heads, mats = np.zeros((nl, 4), np.uint32), np.zeros((nl, 4, 16), np.float32)
        call(heads, mats, nl, None, 0)
        nt = int(heads[:, 2].sum())
        tris = np.zeros((nt, 31), np.float32)
        call(heads, mats, nl, tris, nt)
        return {"heads": heads, "mats": mats, "tris": tris}

    def rays_elided(self, reset: bool = False) -> int:
        n = c_uint64(0)
        self._check(self._lib, self._lib.srt_pt_rays_elided(self._ctx, ctypes.byref(n), int(reset)))
        return int(n.value)

    def tonemap(self, rgb, exposure: float = 1.0) -> np.ndarray:
        """HDR_Image::tonemap_to: (h, w, 3) float radiance -> (h, w, 4) uint8 sRGB, rows flipped for display."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w = rgb.shape[:2]
        out = np.zeros((h, w, 4), np.uint8)
        self._check(self._lib, self._lib.srt_pt_tonemap(self._ctx, _p(rgb), w, h, float(exposure), _p(out)))
        return out

    def tonemap_device(self, d_rgb_ptr: int, w: int, h: int, exposure: float, d_rgba_ptr: int, stream: int = 0) -> None:
        self._check(self._lib, self._lib.srt_pt_tonemap_device(self._ctx, c_void_p(stream), d_rgb_ptr, w, h, float(exposure), d_rgba_ptr))

    def math_exp(self, x):
        x = _f32(x)
        out = np.zeros(len(x), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_exp(self._ctx, _p(x), len(x), _p(out)))
        return out

    def math_pow(self, x, y):
        x, y = _f32(x), _f32(y)
        out = np.zeros(len(x), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_pow(self._ctx, _p(x), _p(y), len(x), _p(out)))
        return out

    def math_div_sqrt(self, num0, num1, num2, den, x, shared_c2=False):
        """(num0/den, num1/den, num2/den, sqrt(x)) through the wave kernel's div3x3 / sqrt3; len % 3 == 0."""
        planes = np.ascontiguousarray(np.stack([_f32(num0), _f32(num1), _f32(num2), _f32(den), _f32(x)]))
        n3 = planes.shape[1]
        assert n3 % 3 == 0
        out = np.zeros((4, n3), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_div_sqrt(self._ctx, _p(planes), n3 // 3, int(bool(shared_c2)), _p(out)))
        return out[0], out[1], out[2], out[3]

    def math_tri_verdict(self, tri, org, dirs, bounds):
        """The wave kernel's batch Triangle::hit (tri_hitN<3>) and the plain tri_hit on n (triangle, origin, three rays) sets.
        tri (n, 9) = p0, e1, e2; org (n, 3); dirs (n, 3, 3); bounds (n, 3, 2) = dist_bounds of each ray.  Returns
        (batch, plain, ambiguous_waves): two dicts of (n, 3) arrays {"hit": bool, "t", "dist"} and the number of waves (64
        consecutive sets) in which some lane was ambiguous, so that the wave computed u and v after all."""
        tri, org, dirs, bounds = _f32(tri).reshape(-1, 9), _f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 9), _f32(bounds).reshape(-1, 3, 2)
        n = len(tri)
        assert len(org) == n and len(dirs) == n and len(bounds) == n and n > 0
        planes = np.ascontiguousarray(np.concatenate([tri, org, dirs, bounds[:, :, 0], bounds[:, :, 1]], axis=1).T)
        out = np.zeros((19, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_tri_verdict(self._ctx, _p(planes), n, _p(out)))
        form = lambda b: {"hit": out[b:b + 9:3].T != 0, "t": out[b + 1:b + 9:3].T.copy(), "dist": out[b + 2:b + 9:3].T.copy()}
        return form(0), form(9), int(np.count_nonzero(out[18, ::64]))

    def math_leaf_fold(self, tris, ntri, org, dirs, bounds):
        """The leaf fold of the wave kernel's mesh branch (leaf_foldN<3>) and the plain ordered fold over tri_hit on W waves of 64
        lanes, one leaf per wave.  tris (W, 12, 9) = p0, e1, e2 of up to twelve triangles; ntri (W,) in 1..12; org (W, 64, 3);
        dirs (W, 64, 3, 3); bounds (W, 64, 3, 2) = dist_bounds of each ray.  Returns (leaf, plain, fell_back): two dicts of
        (W, 64, 3) arrays {"hit": bool, "tri": uint32, "t", "dist"} and per wave whether it folded the leaf the long way."""
        tris, ntri = _f32(tris).reshape(-1, 12, 3, 3), np.ascontiguousarray(ntri, np.uint32).reshape(-1)
        W = len(ntri)
        org, dirs, bounds = _f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 9), _f32(bounds).reshape(-1, 3, 2)
        n = 64 * W
        assert len(tris) == W and len(org) == n and len(dirs) == n and len(bounds) == n and W > 0
        head = np.zeros((W, 148), np.float32)
        head[:, 0] = ntri.view(np.float32)
        padded = np.zeros((W, 12, 3, 4), np.float32)
        padded[..., :3] = tris
        head[:, 4:] = padded.reshape(W, 144)
        planes = np.concatenate([org, dirs, bounds[:, :, 0], bounds[:, :, 1]], axis=1).T
        buf = np.ascontiguousarray(np.concatenate([head.ravel(), planes.ravel()]), np.float32)
        out = np.zeros((25, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_leaf_fold(self._ctx, _p(buf), n, _p(out)))
        res = out[:24].reshape(3, 8, W, 64).transpose(1, 2, 3, 0)                 # (field, wave, lane, ray)
        form = lambda b: {"hit": res[b] != 0, "tri": res[b + 1].view(np.uint32).copy(), "t": res[b + 2].copy(), "dist": res[b + 3].copy()}
        return form(0), form(4), out[24].reshape(W, 64)[:, 0] != 0

    def math_sphere_batch(self, radius, org, dirs, bounds):
        """The wave kernel's batch Sphere::hit (sphere_hitN<3> and the distance step of object_testN's sphere branch)
        and the plain sphere_hit on n (radius, origin, three rays) sets.  radius (n,); org (n, 3); dirs (n, 3, 3); bounds (n, 3, 2) =
        dist_bounds of each ray.  Returns (batch, plain, delta, tangent): two dicts of (n, 3) arrays {"hit": bool, "t", "dist"}, the
        plain form's delta (n, 3), and per set whether its wave (64 consecutive sets) computed the tangent root."""
        radius, org, dirs, bounds = _f32(radius).reshape(-1, 1), _f32(org).reshape(-1, 3), _f32(dirs).reshape(-1, 9), _f32(bounds).reshape(-1, 3, 2)
        n = len(radius)
        assert len(org) == n and len(dirs) == n and len(bounds) == n and n > 0
        planes = np.ascontiguousarray(np.concatenate([radius, org, dirs, bounds[:, :, 0], bounds[:, :, 1]], axis=1).T)
        out = np.zeros((22, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_sphere_batch(self._ctx, _p(planes), n, _p(out)))
        form = lambda b: {"hit": out[b:b + 9:3].T != 0, "t": out[b + 1:b + 9:3].T.copy(), "dist": out[b + 2:b + 9:3].T.copy()}
        return form(0), form(9), out[18:21].T.copy(), out[21] != 0

    def math_box_sweep(self, box, org, inv, times):
        """BBox::hit of the sweeps (box_hit_inv) and of the per-lane traversals (box_hit_rec) on n sets.  box (n, 6) = min, max;
        org (n, 3); inv (n, 3) = reciprocal direction; times (n, 2).  Returns two dicts of (n,) arrays {"hit": bool, "tx", "ty"}."""
        box, org, inv, times = _f32(box).reshape(-1, 6), _f32(org).reshape(-1, 3), _f32(inv).reshape(-1, 3), _f32(times).reshape(-1, 2)
        n = len(box)
        assert len(org) == n and len(inv) == n and len(times) == n and n > 0
        planes = np.ascontiguousarray(np.concatenate([box, org, inv, times], axis=1).T)
        out = np.zeros((6, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_box_sweep(self._ctx, _p(planes), n, _p(out)))
        form = lambda b: {"hit": out[b] != 0, "tx": out[b + 1].copy(), "ty": out[b + 2].copy()}
        return form(0), form(3)

    def math_point_affine(self, mats, points):
        """Mat4 * Vec3 of the wave kernel's leaf section (mat_point_affine) and the plain mat_point on W waves of 64 lanes, one matrix
        per wave.  mats (W, 16) as Mat4::data; points (W * 64, 3).  Returns (affine (n, 3), plain (n, 3), per wave whether w was not
        computed)."""
        mats, points = _f32(mats).reshape(-1, 16), _f32(points).reshape(-1, 3)
        W, n = len(mats), len(points)
        assert n == 64 * W and W > 0
        buf = np.ascontiguousarray(np.concatenate([mats.ravel(), points.T.ravel()]), np.float32)
        out = np.zeros((7, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_point_affine(self._ctx, _p(buf), n, _p(out)))
        return out[0:3].T.copy(), out[3:6].T.copy(), out[6].reshape(W, 64)[:, 0] != 0

    def math_topdown_minmax(self, records, rays):
        """The top-down sweep with the min / max step behind its guard and through the old step alone, on W waves of 64 lanes with one
        seven-node tree each.  records (W, 7, 16) uint32 = WaveInterior words; rays (W * 64, 10) = origin, reciprocal direction, the
        root's times, dist_bounds.  Returns (guarded (n, 7, 6) uint32, old (n, 7, 6) uint32 - per node {flags, cur_far_t.x, left times
        x, y, right times x, y} as bits -, per wave whether it took the min / max step)."""
        records = np.ascontiguousarray(records, np.uint32).reshape(-1, 7, 16)
        rays = _f32(rays).reshape(-1, 10)
        W, n = len(records), len(rays)
        assert n == 64 * W and W > 0
        buf = np.ascontiguousarray(np.concatenate([records.ravel().view(np.float32), rays.T.ravel()]), np.float32)
        out = np.zeros((85, n), np.float32)
        self._check(self._lib, self._lib.srt_pt_math_topdown_minmax(self._ctx, _p(buf), n, _p(out)))
        bits = out[:84].view(np.uint32)
        form = lambda b: np.ascontiguousarray(bits[b:b + 42].reshape(7, 6, n).transpose(2, 0, 1))
        took = out[84].reshape(W, 64) != 0
        assert (took == took[:, :1]).all()
        return form(0), form(42), took[:, 0]

    def math_cos_sin(self, x):
        x = _f32(x)
        c, s = np.zeros_like(x), np.zeros_like(x)
        self._check(self._lib, self._lib.srt_pt_math_cos_sin(self._ctx, _p(x), len(x), _p(c), _p(s)))
        return c, s

    def math_sincos2(self, x):
        """(cos, sin) through srt_sincosf2; math_cos_sin goes through the single-function forms."""
        x = _f32(x)
        c, s = np.zeros_like(x), np.zeros_like(x)
        self._check(self._lib, self._lib.srt_pt_math_sincos2(self._ctx, _p(x), len(x), _p(c), _p(s)))
        return c, s

    def sync(self) -> None:
        self._check(self._lib, self._lib.srt_pt_sync(self._ctx))


class PathtracerGroup:
    """srt_pt_create_multi: one render sharded by image tile over several devices inside one process (include/srt_pt.h).
    members[r] is a Pathtracer over rank r's context (scene / camera / kernel calls are made on every member)."""

    def __init__(self, devices):
        from . import SrtError, _check, load_library

        self._SrtError, self._check = SrtError, _check
        self._lib = load_library()
        self._g = c_void_p()
        self.devices = [int(d) for d in devices]
        devs = (c_int * len(devices))(*self.devices)
        _check(self._lib, self._lib.srt_pt_create_multi(devs, len(devices), ctypes.byref(self._g)))
        self.members = [Pathtracer(_borrowed_ctx=self._lib.srt_pt_group_context(self._g, r)) for r in range(len(devices))]
        self.out_w = self.out_h = 0

    def uses_rccl(self) -> bool:
        return bool(self._lib.srt_pt_group_uses_rccl(self._g))

    def set_params(self, w: int, h: int, pixel_samples: int, depth: int, use_bvh: bool) -> None:
        for m in self.members:
            m.out_w, m.out_h, m.n_samples, m.max_depth, m.scene_use_bvh = int(w), int(h), int(pixel_samples), int(depth), bool(use_bvh)
        self.out_w, self.out_h = int(w), int(h)
        self._check(self._lib, self._lib.srt_pt_group_set_params(self._g, int(w), int(h), int(depth)))

    def build_scene(self, scene) -> None:
        for m in self.members:
            m.build_scene(scene)

    def repose(self, indices, Ts) -> None:
        for m in self.members:
            m.repose(indices, Ts)

    def repose_device(self, indices, d_trans_ptrs, stream: int = 0) -> None:
        """srt_pt_repose_device on every rank: one device pointer per rank, each on its rank's device (ranks that share a device may
        share the array)."""
        for m, ptr in zip(self.members, _one_per_rank(d_trans_ptrs, len(self.members))):
            m.repose_device(indices, ptr, stream)

    def repose_refit(self, indices, Ts) -> None:
        for m in self.members:
            m.repose_refit(indices, Ts)

    def repose_refit_device(self, indices, d_trans_ptrs, stream: int = 0) -> None:
        """srt_pt_repose_refit_device on every rank: one device pointer per rank, as repose_device.  The group's lanes render on
        streams of their own, which nothing orders behind `stream`: each member is settled (srt_pt_sync) before this returns, so the
        group form waits for the refit.  A caller that wants the enqueue-only loop drives the members and their streams itself."""
        for m, ptr in zip(self.members, _one_per_rank(d_trans_ptrs, len(self.members))):
            m.repose_refit_device(indices, ptr, stream)
        _settle(self.members)

    def set_active(self, indices, flags) -> None:
        """srt_pt_group_set_active: srt_pt_set_active on every rank."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        f = np.ascontiguousarray(flags, np.uint8).reshape(-1)
        if len(f) != len(idx):
            raise ValueError(f"{len(idx)} objects but {len(f)} flags")
        self._check(self._lib, self._lib.srt_pt_group_set_active(self._g, _p(idx), _p(f), len(idx)))

    def set_active_device(self, indices, d_active_ptrs, stream: int = 0) -> None:
        """srt_pt_group_set_active_device: one device pointer per rank, as repose_refit_device takes d_trans_ptrs; every member is
        settled before this returns (the group's lanes render on streams of their own)."""
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        ptrs = _one_per_rank(d_active_ptrs, len(self.members))
        arr =(c_void_p * len(ptrs))(*[c_void_p(int(p)) for p in ptrs])
        self._check(self._lib, self._lib.srt_pt_group_set_active_device(self._g, c_void_p(stream), _p(idx), arr, len(idx)))

    def update_mesh(self, index: int, pos, nrm) -> None:
        for m in self.members:
            m.update_mesh(index, pos, nrm)

    def refit_mesh(self, index: int, pos, nrm) -> None:
        for m in self.members:
            m.refit_mesh(index, pos, nrm)

    def refit_mesh_inplace(self, index: int, pos, nrm) -> None:
        for m in self.members:
            m.refit_mesh_inplace(index, pos, nrm)

    def refit_mesh_inplace_device(self, index: int, d_pos_ptrs, d_nrm_ptrs, nverts: int, stream: int = 0) -> None:
        """srt_pt_refit_mesh_inplace_device on every rank: one pair of device pointers per rank, as repose_refit_device takes
        d_trans_ptrs.  The group's lanes render on streams of their own, which nothing orders behind `stream`: every member is settled
        (srt_pt_sync) before this returns, as set_active_device does and for the same reason."""
        pp, nn = list(d_pos_ptrs), list(d_nrm_ptrs)
        if len(pp) != len(self.members) or len(nn) != len(self.members):
            raise ValueError(f"{len(self.members)} ranks but {len(pp)} position and {len(nn)} normal arrays")
        for m, p, n in zip(self.members, pp, nn):
            m.refit_mesh_inplace_device(index, p, n, nverts, stream)
        _settle(self.members)

    def create_skin(self, index: int, bind_pos, bind_nrm, joints) -> SkinGroup:
        """One skin per rank; SkinGroup.pose poses each rank, as update_mesh updates each."""
        return SkinGroup(_handle_per_rank(lambda m: m.create_skin(index, bind_pos, bind_nrm, joints), self.members))

    def create_timeline(self, objects, tracks) -> TimelineGroup:
        """One timeline per rank; TimelineGroup.repose_refit / repose give every rank the same t."""
        return TimelineGroup(_handle_per_rank(lambda m: m.create_timeline(objects, tracks), self.members))

    def create_emitter(self, collide_group, objects, radius: float) -> EmitterGroup:
        """One emitter per rank over the rank's own context (srt_pt_group_context) and the same rank of `collide_group` (which may be
        this group): a forwarder, with no group entry points in C."""
        if len(collide_group.members) != len(self.members):
            raise ValueError(f"a collide group of {len(collide_group.members)} ranks for a group of {len(self.members)}")
        return EmitterGroup(_handle_per_rank(lambda m, c: m.create_emitter(c, objects, radius), self.members, collide_group.members))

    def update_materials(self, indices, materials) -> None:
        for m in self.members:
            m.update_materials(indices, materials)

    def update_lights(self, indices, radiance, angle_bounds, Ts) -> None:
        for m in self.members:
            m.update_lights(indices, radiance, angle_bounds, Ts)

    def update_env_light(self, radiance) -> None:
        for m in self.members:
            m.update_env_light(radiance)

    def dump_shading(self, from_device: bool = False) -> list:
        """Every member's Pathtracer.dump_shading(), by rank."""
        return [m.dump_shading(from_device) for m in self.members]

    def create_shading_timeline(self, materials, lights, env, tracks) -> ShadingTimelineGroup:
        """One shading timeline per rank; ShadingTimelineGroup.update / apply give every rank the same t."""
        return ShadingTimelineGroup(_handle_per_rank(lambda m: m.create_shading_timeline(materials, lights, env, tracks), self.members))

    def scene_counts(self) -> list:
        """Every member's Pathtracer.scene_counts(), by rank (the scene is replicated)."""
        return [m.scene_counts() for m in self.members]

    def set_camera(self, camera) -> None:
        for m in self.members:
            m.set_camera(camera)

    def set_kernel(self, mode: int) -> None:
        for m in self.members:
            m.set_kernel(mode)

    def set_elision(self, on: bool) -> None:
        for m in self.members:
            m.set_elision(on)

    def set_env_sampling(self, mode: str) -> None:
        """srt_pt_group_set_env_sampling: Pathtracer.set_env_sampling on every member."""
        if mode not in Pathtracer.ENV_SAMPLING:
            raise ValueError(f"env sampling mode {mode!r}: one of {Pathtracer.ENV_SAMPLING}")
        self._check(self._lib, self._lib.srt_pt_group_set_env_sampling(self._g, Pathtracer.ENV_SAMPLING.index(mode)))

    def set_normal_colors(self, on: bool) -> None:
        """srt_pt_group_set_normal_colors: the normal-colors debug view on every member."""
        self._check(self._lib, self._lib.srt_pt_group_set_normal_colors(self._g, int(bool(on))))

    def set_dynamic_lights(self, on: bool) -> None:
        """srt_pt_group_set_dynamic_lights: area lights in repose / update_mesh / refit_mesh / create_skin on every member."""
        self._check(self._lib, self._lib.srt_pt_group_set_dynamic_lights(self._g, int(bool(on))))

    def render_epoch(self, seed: int, sample_base: int, samples: int) -> np.ndarray:
        out = np.zeros((self.out_h, self.out_w, 3), np.float32)
        self._check(self._lib, self._lib.srt_pt_group_render_epoch(self._g, seed, sample_base, samples, _p(out)))
        return out

    def render_epoch_device(self, seed: int, sample_base: int, samples: int):
        """Enqueue one epoch on every rank + the gather; returns (device pointer of the image on rank 0, its stream). No wait."""
        d, s = c_void_p(), c_void_p()
        self._check(self._lib, self._lib.srt_pt_group_render_epoch_device(self._g, seed, sample_base, samples, ctypes.byref(d), ctypes.byref(s)))
        return d.value, s.value

    def render_epoch_lane(self, lane: int, seed: int, sample_base: int, samples: int):
        """As render_epoch_device on lane `lane` (its own streams and buffers): epochs on different lanes overlap."""
        d, s = c_void_p(), c_void_p()
        st = self._lib.srt_pt_group_render_epoch_lane(self._g, int(lane), seed, sample_base, samples, ctypes.byref(d), ctypes.byref(s))
        if st == SRT_CANCELLED:
            raise SrtCancelled()
        self._check(self._lib, st)
        return d.value, s.value

    # -- a render with the accumulator on the devices (what the drop-in class renders with) ----------------------------
    def max_samples_per_launch(self) -> int:
        m = c_uint32()
        self._check(self._lib, self._lib.srt_pt_group_max_samples_per_launch(self._g, ctypes.byref(m)))
        return int(m.value)

    def reset_accumulator(self) -> None:
        self._check(self._lib, self._lib.srt_pt_group_reset_accumulator(self._g))

    def render_samples(self, lane: int, seed: int, base: int, n: int) -> None:
        """One launch of n samples per pixel on every rank, on lane `lane`. No wait."""
        st = self._lib.srt_pt_group_render_samples(self._g, int(lane), seed, base, n)
        if st == SRT_CANCELLED:
            raise SrtCancelled()
        self._check(self._lib, st)

    def wait_lane(self, lane: int) -> None:
        self._check(self._lib, self._lib.srt_pt_group_wait_lane(self._g, int(lane)))

    def fold(self, lane: int, spe: int, position: int, total: int, first_k: int) -> None:
        """Fold the launch last rendered on `lane` into every rank's accumulator (call in launch order)."""
        self._check(self._lib, self._lib.srt_pt_group_fold(self._g, int(lane), spe, position, total, first_k))

    def accumulator_image(self) -> np.ndarray:
        """The running mean gathered to rank 0 and copied to the host: (h, w, 3) float32, row 0 = bottom (waits for it)."""
        d, s = c_void_p(), c_void_p()
        self._check(self._lib, self._lib.srt_pt_group_accumulator_image(self._g, ctypes.byref(d), ctypes.byref(s)))
        out = np.zeros((self.out_h, self.out_w, 3), np.float32)
        L = self._lib                                   # the HIP runtime the library is linked to (dlsym searches its dependencies)
        if L.hipSetDevice(self.devices[0]) != 0 or L.hipMemcpyAsync(_p(out), d, out.nbytes, _HIP_MEMCPY_D2H, s) != 0 or L.hipStreamSynchronize(s) != 0:
            raise self._SrtError(-3, "srt_pt_group_accumulator_image: copy to the host failed")
        return out

    def cancel_requested(self) -> bool:
        return bool(self._lib.srt_pt_group_cancel_requested(self._g))

    def cancel_device(self) -> None:
        self._check(self._lib, self._lib.srt_pt_group_cancel(self._g))

    def clear_cancel(self) -> None:
        self._check(self._lib, self._lib.srt_pt_group_clear_cancel(self._g))

    def set_ray_log(self, capacity: int) -> None:
        self._check(self._lib, self._lib.srt_pt_group_set_ray_log(self._g, int(capacity)))

    def read_ray_log(self, lane: int = 0):
        n, dropped = c_size_t(), c_uint64()
        self._check(self._lib, self._lib.srt_pt_group_read_ray_log(self._g, int(lane), None, 0, ctypes.byref(n), ctypes.byref(dropped)))
        out = np.zeros(n.value, LOGGED_RAY_DTYPE)
        got = c_size_t()
        self._check(self._lib, self._lib.srt_pt_group_read_ray_log(self._g, int(lane), _p(out) if n.value else None, n.value, ctypes.byref(got),
                                                                     ctypes.byref(dropped)))
        return out[:got.value], int(dropped.value)

    def gather_time(self, enable: bool = True):
        """(total ms, epochs) of the exchange step (gather + un-tiling, incl. waiting for the slowest rank) since the previous call."""
        ms, n = ctypes.c_double(), c_uint64()
        self._check(self._lib, self._lib.srt_pt_group_gather_time(self._g, int(enable), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def ray_count(self, reset: bool = False):
        r = [m.ray_count(reset) for m in self.members]
        return sum(x[0] for x in r), sum(x[1] for x in r)

    def close(self) -> None:
        if self._g:
            for m in self.members:
                m.close()
            self._lib.srt_pt_group_destroy(self._g)
            self._g = c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
