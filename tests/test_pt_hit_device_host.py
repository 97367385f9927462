"""CPU: srt_pt_hit_device on a host-only context (device = -1) - the entry point validates before it looks for a device, so every
refusal of include/srt_pt.h is reachable here: status and message; a valid call is SRT_ERR_UNSUPPORTED after validating, a call of
no rays SRT_OK.  (What it computes: tests/test_pt_hit_device_gpu.py.)"""
import os

import numpy as np
import pytest

import _harness as H
from _cases import pt_scene, random_rays

INVALID, STATE, UNSUPPORTED, OK = -1, -5, -4, 0


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def rays():
    org, d, b = random_rays(3, 16)
    out9, ids, flags = np.zeros((16, 9), np.float32), np.zeros((16, 2), np.uint32), np.zeros(16, np.uint8)
    return [np.ascontiguousarray(a) for a in (org, d, b, out9, ids, flags)]


def host_pt(srt):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    pt.build_scene(pt_scene("cbox"))
    return pt


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    assert lib.srt_pt_hit_device is not None and lib.srt_pt_hit_device_paths is not None
    for name in ("hit_device", "hit_tensors", "hit_device_paths"):
        assert callable(getattr(srt.Pathtracer, name)), name
    assert not hasattr(srt.PathtracerGroup, "hit_device")        # no group form: a caller addresses group.members[r]
    assert "srt_pt_hit_device(" in open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    assert "srt_pt_hit_device_paths(" in open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()


def test_refusals(srt, rays):
    org, d, b, out9, ids, flags = (a.ctypes.data for a in rays)
    pt = host_pt(srt)
    L = pt._lib
    message = lambda: L.srt_last_error().decode()
    assert L.srt_pt_hit_device(None, None, org, d, b, 16, out9, ids, flags) == INVALID and "NULL context" in message()
    for o, dd in ((None, d), (org, None), (None, None)):
        with pytest.raises(srt.SrtError, match="NULL origins or directions") as e:
            pt.hit_device(o or 0, dd or 0, b, 16, out9, ids, flags)
        assert e.value.status == INVALID and "srt_pt_hit_device:" in str(e.value)
    with pytest.raises(srt.SrtError, match="no output") as e:
        pt.hit_device(org, d, b, 16)
    assert e.value.status == INVALID
    with pytest.raises(srt.SrtError, match="no output") as e:   # (whatever n is)
        pt.hit_device(org, d, b, 0)
    assert e.value.status == INVALID
    with pytest.raises(srt.SrtError, match="too many rays") as e:
        pt.hit_device(org, d, b, 0x80000000, out9)
    assert e.value.status == UNSUPPORTED
    # a valid call - every combination of outputs, bounds or none - validates and only then finds no device
    for outs in ((out9, 0, 0), (0, ids, 0), (0, 0, flags), (out9, ids, flags)):
        for bounds in (b, 0):
            with pytest.raises(srt.SrtError, match="host-only") as e:
                pt.hit_device(org, d, bounds, 16, *outs)
            assert e.value.status == UNSUPPORTED and "srt_pt_hit_device:" in str(e.value)
    assert all(not a.any() for a in rays[3:]), "a refused call wrote to its outputs"
    # no rays: SRT_OK, with or without pointers to rays
    assert L.srt_pt_hit_device(pt._ctx, None, None, None, None, 0, out9, None, None) == OK
    pt.hit_device(org, d, b, 0, 0, 0, flags)
    assert pt.hit_device_paths() == (0, 0, 0)
    assert L.srt_pt_hit_device_paths(pt._ctx, None) == INVALID and L.srt_pt_hit_device_paths(None, out9) == INVALID
    pt.close()


def test_no_committed_scene(srt, rays):
    org, d, b, out9, ids, flags = (a.ctypes.data for a in rays)
    empty = srt.Pathtracer(device=-1)
    for n in (16, 0):
        with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
            empty.hit_device(org, d, b, n, out9)
        assert e.value.status == STATE
    empty.close()
