"""CPU: srt_pt_repose_device on the host side.  The device functions of pt_pose.h compiled for the host (through
tests/host_emu/pose_host.cpp) against mat_inverse / mat_ne_identity / Box::transform / mat_mul of pt_scene.cpp as bit patterns;
the ABI on a host-only context; and a sanitized stand-alone program over prepare_repose_supplied, the scene layer's repose with
the per-object values supplied by the caller."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _repose_device_cases as RC

INVALID, UNSUPPORTED, STATE = -1, -4, -5          # SRT_ERR_* (include/srt_raster.h)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def test_device_functions_on_the_host():
    """pose_inverse / pose_ne_identity / pose_box / pose_object over every matrix of matrix_cases() with every box of box_cases()."""
    lib = RC.pose_lib()
    boxes = RC.box_cases()
    seen = np.zeros(4, np.uint32)
    total = np.zeros(4, np.uint64)
    for name, mats in RC.matrix_cases().items():
        mats = np.ascontiguousarray(mats, np.float32)
        assert lib.pose_emu_mismatches(H.P(mats), len(mats), H.P(boxes), len(boxes), H.P(seen)) == 0, name
        if name == "singular":
            assert seen[0] == 2 and seen[1] >= 1            # 0 / 0 and x / 0: the NaNs and the infinities are there, and where the host's are
        if name == "NaN":
            assert seen[0] == 1 and seen[2] == 0            # a NaN entry: has_trans
        if name in ("identity", "identity with -0"):
            assert seen[2] == 1                             # -0.0f equals 0.0f: no transform
        total += seen
    assert len(RC.matrix_cases()["cbox_particles"]) == 74 and len(RC.matrix_cases()["random"]) >= 300
    assert total[3] > 0                                     # posed bounds that are -0 occurred: their sign was compared


def test_translate_scale_on_the_host():
    """pose_translate_scale and the numpy restatement against mat_mul(translate, scale): zero signs included."""
    lib = RC.pose_lib()
    rng = np.random.default_rng(5)
    pos = np.concatenate([np.array([[0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.25, -0.0, -1.5], [1e-40, -1e-40, 3.0]], np.float32),
                          (rng.random((200, 3), np.float32) - np.float32(0.5)) * np.float32(3.0)]).astype(np.float32)
    for scale in (0.03, 1.0, -0.5, -0.0, 0.0):
        assert lib.pose_ts_mismatches(H.P(pos), len(pos), ctypes.c_float(scale)) == 0, scale
        want = np.zeros((len(pos), 16), np.float32)
        lib.pose_ts_reference(H.P(pos), len(pos), ctypes.c_float(scale), H.P(want))
        got = RC.translate_scale_product(pos, scale)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), scale
    # the product is not the matrix written down directly: -0 positions and negative scales give other zero signs
    direct = np.array([RC.translate_scale(p, -0.5) for p in pos], np.float32)
    assert not np.array_equal(direct.view(np.uint32), RC.translate_scale_product(pos, -0.5).view(np.uint32))
    assert np.array_equal(direct, RC.translate_scale_product(pos, -0.5))


def refusal_scene():
    """Objects: 0-4 walls, 5 sphere, 6 blob, 7 area light, 8 instance of 6."""
    return IC.sweeps_scene()


def test_abi_on_a_host_only_context(srt):
    """Both symbols, their documented signatures and the Python methods; on a host-only context srt_pt_repose_device refuses what
    srt_pt_repose refuses, with its status and its message, and a valid call is SRT_ERR_UNSUPPORTED; the scene stays as it was."""
    lib = srt.load_library()
    assert hasattr(lib, "srt_pt_repose_device") and hasattr(lib, "srt_pt_particle_transforms_device")
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    assert "int srt_pt_repose_device(srt_pt* pt, void* stream, const uint32_t* objects, const float* d_trans, uint32_t n);" in header
    assert ("int srt_pt_particle_transforms_device(srt_pt* pt, void* stream, const float* d_pos, uint32_t n, float scale, float* d_trans_out);") in header
    assert lib.srt_pt_repose_device.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    for cls, names in ((srt.Pathtracer, ("repose_device", "particle_transforms_device")), (srt.PathtracerGroup, ("repose_device",))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    S = refusal_scene()
    nobj = len(S["objects"])
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    T = np.array([IC.translate(S["objects"][8]["T"], (0.1, 0.0, 0.0)), IC.translate(S["objects"][5]["T"], (0.0, 0.1, 0.0))], np.float32)
    fake = ctypes.c_void_p(T.ctypes.data)                  # never read: a host-only context enqueues nothing
    ok = np.array([8, 5], np.uint32)
    assert lib.srt_pt_repose_device(pt._ctx, None, H.P(ok), fake, 2) == STATE and b"before srt_pt_scene_commit" in lib.srt_last_error()
    pt.build_scene(S)
    first = IC.all_dumps(pt, nobj)
    counts = pt.scene_counts()

    def message(status):
        return status, lib.srt_last_error().decode().split(": ", 1)[1]

    assert lib.srt_pt_repose_device(None, None, H.P(ok), fake, 2) == INVALID
    assert lib.srt_pt_repose_device(pt._ctx, None, None, fake, 2) == INVALID and lib.srt_pt_repose_device(pt._ctx, None, H.P(ok), None, 2) == INVALID
    assert message(lib.srt_pt_repose(pt._ctx, H.P(ok), None, 2)) == message(lib.srt_pt_repose_device(pt._ctx, None, H.P(ok), None, 2))
    for what, bad in (("an area light", [8, 7]), ("a duplicate", [8, 8]), ("out of range", [nobj, 5])):
        bad = np.array(bad, np.uint32)
        host = message(lib.srt_pt_repose(pt._ctx, H.P(bad), H.P(T), 2))
        dev = message(lib.srt_pt_repose_device(pt._ctx, None, H.P(bad), fake, 2))
        assert host == dev and dev[0] == INVALID, what
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts, what
    assert lib.srt_pt_repose_device(pt._ctx, None, H.P(ok), fake, 2) == UNSUPPORTED and b"host-only" in lib.srt_last_error()
    with pytest.raises(srt.SrtError, match="host-only") as e:
        pt.repose_device(ok, T.ctypes.data)
    assert e.value.status == UNSUPPORTED
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts
    with pytest.raises(srt.SrtError):                      # the transforms kernel needs a device
        pt.particle_transforms_device(T.ctypes.data, 1, 0.03, T.ctypes.data)
    # srt_pt_repose itself is what it was: the repose a fresh commit of the new poses gives
    pt.repose(ok, T)
    fresh = srt.Pathtracer(device=-1)
    fresh.set_params(8, 8, 1, 8, True)
    fresh.build_scene(IC.with_poses(S, ok, T))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj)) and not IC.dumps_equal(IC.all_dumps(pt, nobj), first)
    fresh.close()
    pt.close()


def test_sanitized_supplied_repose(tmp_path):
    """tests/host_emu/repose_device_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: prepare_repose_supplied on
    the 74-object particle scene and repose_case's list against prepare_repose, refused lists - built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once on the CPU."""
    S = IC.particles_shared()[0]
    idx, Ts = IC.repose_case(S)
    assert len(S["objects"]) == 74 and len(idx) == 12
    scene_file = str(tmp_path / "particles.scene")
    RC.write_scene_file(scene_file, S, idx, Ts)
    H.run_sanitized_main(tmp_path, "repose_device_sanitized_main.cpp", args=[scene_file], expect="repose_device_sanitized: ok (74 objects, 12 listed)")
