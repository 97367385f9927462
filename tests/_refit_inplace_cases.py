"""Scenes, expectations and the host emulation of the in-place refit tests (test_pt_refit_inplace_host.py,
test_pt_refit_inplace_gpu.py).

srt_pt_refit_mesh_inplace keeps a mesh's BVH<Triangle> AND the BVH<Object> and gives both new boxes, so the refitted scene is not
the scene a fresh commit of the new vertices builds: the oracle, which only builds, walks other trees.  What such a scene must
compute is defined by the host definition (prepare_mesh_refit_inplace / apply_mesh_refit_inplace, pt_scene.cpp) walked by the
device headers compiled for the host (tests/host_emu/refit_inplace_flat_host.cpp): EmuInplace below."""
import ctypes

import numpy as np

import _harness as H
import _repose_refit_cases as PR
from _cases import random_rays
from _refit_cases import DEPTH, HT, RAYS, SEED, SPP, W, bits_equal, every_sample, epoch_of  # noqa: F401

# Seed of random_rays() for the closest-hit comparison with the oracle.  The in-place form walks another BVH<Object> than the one the
# refit tests' RAY_SEED = 3 was chosen for; checked on the CPU (test_pt_refit_inplace_host.py::test_closest_hits_equal_the_oracle):
# with seed 3 the emulation's closest hits after D1, D2 and D3 on the blob scene, the two-mesh scene and the scene with instances
# equal the oracle's on a fresh commit of the new vertices on every one of the 2048 rays, so the seed stays.  Exceptions allowed: 0.
RAY_SEED = 3
TIES_CAP = 0


def emu_lib():
    lib = ctypes.CDLL(H.build_host_lib("refit_inplace_flat_host", ["refit_inplace_flat_host.cpp"], scene_layer=True))
    lib.emu_refit_create.restype = ctypes.c_void_p
    lib.emu_dump_top.restype = ctypes.c_long
    lib.emu_dump_top.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.emu_top_cost.restype = ctypes.c_double
    lib.emu_top_cost.argtypes = [ctypes.c_void_p]
    return lib


class EmuInplace(PR.EmuTop):
    """The scene layer's build, then host in-place refits (and top-level refits, reposes, refits with a rebuilt BVH<Object>, active
    flags), walked by the device headers on the CPU."""

    def __init__(self, scene, w=W, h=HT, depth=DEPTH):
        self.lib = emu_lib()                                  # (a superset of EmuTop's library: the same feeding, two more calls)
        self.h_ = ctypes.c_void_p(self.lib.emu_refit_create())
        self.use_bvh = True
        self.nobj = len(scene["objects"])
        assert not any(o.get("light_mesh") is not None for o in scene["objects"]) and int((scene.get("env") or {"type": 0})["type"]) != 3
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
        for l in scene.get("lights", []):
            self.lib.emu_add_light(self.h_, int(l["type"]), H.P(H._f32(l["radiance"])), H.P(H._f32(l.get("angle_bounds", (0.0, 0.0)))), H.P(H._f32(l["T"])))
        if scene.get("env"):
            self.lib.emu_set_env(self.h_, int(scene["env"]["type"]), H.P(H._f32(scene["env"]["radiance"])))
        cam = scene["camera"]
        self.lib.emu_set_camera(self.h_, H.P(H._f32(cam["iview"])), ctypes.c_float(float(cam["vfov"])), ctypes.c_float(float(cam["ar"])), w, h, depth)

    def refit_inplace(self, index, pos, nrm):
        pos, nrm = H._f32(pos), H._f32(nrm)
        return self.lib.emu_refit_inplace(self.h_, int(index), H.P(pos), H.P(nrm), len(pos))

    def set_active(self, idx, flags):
        idx, flags = np.ascontiguousarray(idx, np.uint32).reshape(-1), np.ascontiguousarray(flags, np.uint8).reshape(-1)
        return self.lib.emu_set_active(self.h_, H.P(idx), H.P(flags), len(idx))


def apply_steps(target, steps):
    """steps: ("inplace", index, pos, nrm) | ("repose_refit", idx, Ts) | ("refit", index, pos, nrm) | ("active", idx, flags) on an
    EmuInplace; the same names are the host forms of a Pathtracer (host_forms below)."""
    for step in steps:
        kind, args = step[0], step[1:]
        r = {"inplace": target.refit_inplace, "repose_refit": target.repose_refit, "refit": target.refit, "active": target.set_active}[kind](*args)
        assert r in (0, None), step[0]


def expectation(scene, steps, w=W, h=HT, depth=DEPTH, spp=SPP, samples=True, ray_seed=RAY_SEED):
    """What a context must compute after `steps` on `scene`: every sample, the epoch image, the hit records of both walks, the
    dumped top-level tree and its cost."""
    e = EmuInplace(scene, w, h, depth)
    apply_steps(e, steps)
    org, d, b = random_rays(ray_seed, RAYS)
    out = {"hits": e.hit9(org, d, b), "dump": e.dump_top(), "cost": e.cost()}
    if samples:
        out["samples"] = e.trace_samples(SEED, *every_sample(w, h, spp))
        out["epoch"] = epoch_of(out["samples"][0], w, h, spp)
    e.close()
    return out


def host_forms(pt, steps):
    """The same steps through a Pathtracer's blocking host forms."""
    for step in steps:
        kind, args = step[0], step[1:]
        {"inplace": pt.refit_mesh_inplace, "repose_refit": pt.repose_refit, "refit": pt.refit_mesh, "active": pt.set_active}[kind](*args)


def family_of(scene, index):
    return [index] + [k for k, o in enumerate(scene["objects"]) if o["kind"] == "instance" and int(o["of"]) == index]


def scene_with(scene, index, pos):
    """The description with mesh `index` given new positions (for local_boxes_numpy)."""
    out = dict(scene)
    out["objects"] = list(scene["objects"])
    out["objects"][index] = dict(scene["objects"][index], pos=np.ascontiguousarray(pos, np.float32))
    return out


def expected_top_boxes(scene, index, pos, links, order, active=None):
    """top_boxes_numpy over the posed boxes of local_boxes_numpy with the mesh's new vertices - BBox() for an inactive object."""
    posed = PR.posed_boxes_numpy(PR.local_boxes_numpy(scene_with(scene, index, pos)), PR.transforms_of(scene))
    if active is not None:
        big = np.float32(np.finfo(np.float32).max)
        posed = np.where(np.asarray(active, bool)[:, None], posed, np.array([big, big, big, -big, -big, -big], np.float32))
    return PR.top_boxes_numpy(links, order, posed)
