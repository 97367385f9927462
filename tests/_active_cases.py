"""Scenes, expectations and the host emulation of the active-flag tests (test_pt_active_host.py, test_pt_active_gpu.py).

srt_pt_set_active hides objects behind empty boxes and keeps the BVH<Object> of the commit, so a scene with hidden objects is NOT
the scene a fresh commit without them builds: the oracle, which only builds, walks another tree.  What such a scene must compute is
defined by the host definition (check_active_list / apply_set_active / mask_top, pt_scene.cpp) walked by the device headers compiled
for the host (tests/host_emu/active_flat_host.cpp): EmuActive below.  The boxes themselves are top_boxes_numpy of
_repose_refit_cases fed with masked posed boxes (masked)."""
import ctypes

import numpy as np

import _harness as H
import _instance_cases as IC
import _repose_refit_cases as C
from _cases import random_rays
from _repose_refit_cases import RAY_SEED, RAYS, SEED, bits_equal, every_sample, epoch_of  # noqa: F401

W, HT, DEPTH, SPP = 32, 24, 6, 3

# Seed of hidden(): chosen on the CPU so that the emulation's closest hits with a third of the particles hidden equal the oracle's
# on a fresh commit of the scene without them on every one of the 2048 random_rays (closest hits do not depend on the tree except
# at exact ties).  Seeds 0 .. 7 were tried in order; the mismatching rays the emulation itself shows for this seed: 0.
MASK_SEED = 0
TIES_CAP = 0


def emu_lib():
    lib = ctypes.CDLL(H.build_host_lib("active_flat_host", ["active_flat_host.cpp"], scene_layer=True))
    lib.emu_refit_create.restype = ctypes.c_void_p
    lib.emu_dump_top.restype = ctypes.c_long
    lib.emu_dump_top.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.emu_top_cost.restype = ctypes.c_double
    lib.emu_top_cost.argtypes = [ctypes.c_void_p]
    lib.emu_get_active.restype = ctypes.c_long
    lib.emu_get_active.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


class EmuActive(C.EmuTop):
    """The scene layer's build, then host set_active calls (and refits, reposes), walked by the device headers on the CPU."""

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

    def set_active(self, idx, flags):
        idx, flags = np.ascontiguousarray(idx, np.uint32).reshape(-1), np.ascontiguousarray(flags, np.uint8).reshape(-1)
        assert len(idx) == len(flags)
        return self.lib.emu_set_active(self.h_, H.P(idx), H.P(flags), len(idx))

    def active(self):
        out = np.zeros(self.nobj, np.uint8)
        assert self.lib.emu_get_active(self.h_, out.ctypes.data, self.nobj) == self.nobj
        return out


def expectation(scene, steps, w=W, h=HT, depth=DEPTH, spp=SPP, samples=True):
    """What a context must compute after `steps` on `scene` - ("active", indices, flags) or ("refit", indices, Ts), in order: every
    sample, the epoch image, the hit records of both walks, the dumped top-level tree, its cost and the table."""
    e = EmuActive(scene, w, h, depth)
    for kind, idx, val in steps:
        assert (e.set_active(idx, val) if kind == "active" else e.repose_refit(idx, val)) == 0
    org, d, b = random_rays(RAY_SEED, RAYS)
    out = {"hits": e.hit9(org, d, b), "dump": e.dump_top(), "cost": e.cost(), "active": e.active()}
    if samples:
        out["samples"] = e.trace_samples(SEED, *every_sample(w, h, spp))
        out["epoch"] = epoch_of(out["samples"][0], w, h, spp)
    e.close()
    return out


def hidden(seed=MASK_SEED, count=IC.PARTICLE_COUNT // 3):
    """A seeded third of the particles (insertion indices, ascending)."""
    return np.sort(np.random.default_rng(seed).choice(C.particle_indices(), count, replace=False)).astype(np.uint32)


def flags_of(nobj, off):
    a = np.ones(nobj, np.uint8)
    a[np.asarray(off, np.int64)] = 0
    return a


def masked(posed, active):
    """E: the posed boxes (nobj, 6) with BBox() - min = +FLT_MAX, max = -FLT_MAX - in the place of every inactive object's."""
    big = np.float32(np.finfo(np.float32).max)
    out = np.array(posed, np.float32, copy=True)
    out[np.asarray(active) == 0] = [big, big, big, -big, -big, -big]
    return out


def posed_of(scene, idx=(), Ts=()):
    T = C.transforms_of(scene)
    if len(idx):
        T[np.asarray(idx, np.int64)] = np.ascontiguousarray(Ts, np.float32).reshape(-1, 16)
    return C.posed_boxes_numpy(C.local_boxes_numpy(scene), T)


def expected_boxes(scene, active, links, order, idx=(), Ts=()):
    """The node boxes of the definition: top_boxes_numpy over the masked posed boxes."""
    return C.top_boxes_numpy(links, order, masked(posed_of(scene, idx, Ts), active))


def posed_from_leaves(boxes, links, order, nobj):
    """The posed box of every object read off a tree with every object active: a leaf holds one object and its box is that object's."""
    out = np.zeros((nobj, 6), np.float32)
    for k in range(len(links)):
        start, size, l, r = (int(v) for v in links[k])
        if l == r and size == 1:
            out[int(order[start]) - 1] = boxes[k]
    return out


def tree_cost_numpy(boxes, links):
    """tree_cost with the empty-node rule: a node with mn > mx on any axis contributes 0, an empty root gives 0."""
    b = np.asarray(boxes, np.float64)
    empty = np.any(b[:, :3] > b[:, 3:], axis=1)
    if empty[0]:
        return 0.0
    e = b[:, 3:] - b[:, :3]
    sa = np.where(empty, 0.0, 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]))
    leaf = links[:, 2] == links[:, 3]
    w = np.where(leaf, links[:, 1].astype(np.float64), 1.0)
    return float(np.sum(w * (sa / sa[0])))


def without(scene, off):
    """The description a fresh commit is given when the objects `off` do not exist: instances expanded (a hidden source's instances
    stay), the hidden objects left out."""
    out = IC.expand(scene)
    gone = {int(i) for i in off}
    out["objects"] = [o for k, o in enumerate(out["objects"]) if k not in gone]
    return out


def values_equal(a, b):
    """Equality as values (a zero bound that occurs as +0 and as -0 follows the fold's order)."""
    return np.array_equal(np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32))


def mismatches(got, want):
    return int(np.sum(np.any(np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32), axis=1)))


pool_scene = C.pool_scene
one_object_scene = C.one_object_scene
particle_indices = C.particle_indices
