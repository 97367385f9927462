"""CPU: the device traversal headers (pt_trace.h nested walk, pt_flat.h flattened walk) compiled for the host and run over scenes
whose objects share triangle and BVH<Triangle> ranges (srt_pt_add_instance).  S against S' = the same scene made of copies:
hit flag, distance bits and object slot of every ray must agree; the triangle index is a storage address and may differ, so it
is compared relative to the object's first triangle through the oracle's hit record instead (position, normal, material)."""
import ctypes

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
from _cases import random_rays, unnormalised_rays


def emu_lib():
    lib = ctypes.CDLL(H.build_host_lib("instances_flat_host", ["instances_flat_host.cpp"], scene_layer=True))
    lib.emu_create.restype = ctypes.c_void_p
    return lib


class EmuInstances(H.EmuPT):
    def __init__(self, scene, use_bvh=True):
        self.lib = emu_lib()
        self.h_ = ctypes.c_void_p(self.lib.emu_create())
        self.use_bvh = use_bvh
        self.feed(scene)

    def feed(self, scene):
        for m in scene["materials"]:
            self._add_material(int(m["type"]), H._f32(m["a"]), H._f32(m["b"]), float(m["ior"]))
        for o in scene["objects"]:
            T = H._f32(o["T"])
            if o["kind"] == "mesh":
                self._add_mesh(H._f32(o["pos"]), H._f32(o["nrm"]), np.ascontiguousarray(o["idx"], np.uint32), T, int(o["material"]), bool(o["is_light"]))
            elif o["kind"] == "instance":
                assert self.lib.emu_add_instance(self.h_, int(o["of"]), H.P(T), int(o["material"])) == 0
            else:
                self._add_sphere(float(o["radius"]), T, int(o["material"]))
        self._commit()


def rays():
    o1, d1, b1 = random_rays(21, 3000)
    o2, d2, b2 = unnormalised_rays(22, 1000)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([b1, b2])


@pytest.mark.parametrize("which,use_bvh", [("particles", True), ("particles", False), ("sweeps", True), ("sweeps", False)])
def test_walks_on_shared_ranges(which, use_bvh):
    S = IC.particles_shared()[0] if which == "particles" else IC.sweeps_scene()
    S1 = IC.expand(S)
    org, d, b = rays()
    a, c = EmuInstances(S, use_bvh), EmuInstances(S1, use_bvh)
    flat = len(S["objects"]) <= 31                       # the flattened walk packs the object slot into five bits
    na, fa = a.hit(org, d, b)
    nc, fc = c.hit(org, d, b)
    assert np.count_nonzero(na[:, 0]) > 1000                 # (sanity: the oracle has 1253 of the 4000 rays hit the particle scene)
    assert np.array_equal(na[:, :3], nc[:, :3])           # hit, distance bits, object slot
    if flat and use_bvh:
        assert np.array_equal(fa[:, :3], fc[:, :3]) and np.array_equal(fa, na)
        for slot in (1, 2):                              # the other batch slots of flat_trace3
            assert np.array_equal(a.hit(org, d, b, slot)[1], na)
    # and against the oracle on S': same hits at the same distances
    want = H.OraclePT(S1, 8, 8, 4, use_bvh).hit(org, d, b)
    assert np.array_equal(na[:, 0] != 0, want[:, 0] != 0)
    assert np.array_equal(na[:, 1][want[:, 0] != 0], np.ascontiguousarray(want[:, 1]).view(np.uint32)[want[:, 0] != 0])
    a.close(); c.close()
