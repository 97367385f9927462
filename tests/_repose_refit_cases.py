"""Scenes, expectations and the host emulation of the top-level refit tests (test_pt_repose_refit_host.py,
test_pt_repose_refit_gpu.py).

srt_pt_repose_refit keeps the BVH<Object> and gives it new boxes, so the refitted scene is NOT the scene a fresh commit of the new
poses builds: the oracle, which only builds, walks another tree.  What a refitted scene must compute is defined by the host
refit (prepare_top_refit / apply_top_refit, pt_scene.cpp) walked by the device headers compiled for the host
(tests/host_emu/repose_refit_flat_host.cpp): EmuTop below.  The boxes themselves are restated in numpy from a dump's links and
order (top_boxes_numpy)."""
import ctypes

import numpy as np

import _harness as H
import _instance_cases as IC
import _refit_cases as RF
from _cases import random_rays
from _refit_cases import DEPTH, HT, RAY_SEED, RAYS, SEED, SPP, W, bits_equal, every_sample, epoch_of  # noqa: F401

# Seed of scatter(): chosen on the CPU so that the emulation's closest hits after the refit equal the oracle's on a fresh commit of
# the same poses on every one of the 2048 random_rays (closest hits do not depend on the tree except at exact ties); the
# mismatching rays the emulation itself shows for this seed: 0.
POSE_SEED = 1
TIES_CAP = 0


def emu_lib():
    lib = ctypes.CDLL(H.build_host_lib("repose_refit_flat_host", ["repose_refit_flat_host.cpp"], scene_layer=True))
    lib.emu_refit_create.restype = ctypes.c_void_p
    lib.emu_dump_top.restype = ctypes.c_long
    lib.emu_dump_top.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.emu_top_cost.restype = ctypes.c_double
    lib.emu_top_cost.argtypes = [ctypes.c_void_p]
    return lib


class EmuTop(RF.EmuRefit):
    """The scene layer's build, then host top-level refits (and reposes), walked by the device headers on the CPU."""

    def __init__(self, scene, w=W, h=HT, depth=DEPTH):
        self.lib = emu_lib()                                  # (a superset of EmuRefit's library: the same feeding, one more call)
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

    def repose_refit(self, idx, Ts):
        idx, Ts = np.ascontiguousarray(idx, np.uint32).reshape(-1), H._f32(Ts).reshape(-1, 16)
        return self.lib.emu_repose_refit(self.h_, H.P(idx), H.P(Ts), len(idx))

    def repose(self, idx, Ts):
        idx, Ts = np.ascontiguousarray(idx, np.uint32).reshape(-1), H._f32(Ts).reshape(-1, 16)
        return self.lib.emu_repose(self.h_, H.P(idx), H.P(Ts), len(idx))

    def dump_top(self):
        cap = 2 * self.nobj + 2
        boxes, links, order = np.zeros((cap, 6), np.float32), np.zeros((cap, 4), np.uint32), np.zeros(self.nobj, np.uint32)
        n = self.lib.emu_dump_top(self.h_, boxes.ctypes.data, links.ctypes.data, cap, order.ctypes.data)
        return boxes[:n], links[:n], order

    def cost(self):
        return float(self.lib.emu_top_cost(self.h_))


def expectation(scene, refits, w=W, h=HT, depth=DEPTH, spp=SPP, samples=True):
    """What a context must compute after `refits` = [(indices, Ts), ..] (host top-level refits) on `scene`: every sample, the
    epoch image, the hit records of both walks, the dumped top-level tree and its cost."""
    e = EmuTop(scene, w, h, depth)
    for idx, Ts in refits:
        assert e.repose_refit(idx, Ts) == 0
    org, d, b = random_rays(RAY_SEED, RAYS)
    out = {"hits": e.hit9(org, d, b), "dump": e.dump_top(), "cost": e.cost()}
    if samples:
        out["samples"] = e.trace_samples(SEED, *every_sample(w, h, spp))
        out["epoch"] = epoch_of(out["samples"][0], w, h, spp)
    e.close()
    return out


def local_boxes_numpy(scene):
    """(nobj, 6) float32: the object-space box Object::bbox poses - a mesh's is the fold of Triangle::bbox over its triangles (a
    flat axis: max = min + 1.0f), an instance's its source's, a sphere's +-radius."""
    out = np.zeros((len(scene["objects"]), 6), np.float32)
    for k, o in enumerate(scene["objects"]):
        if o["kind"] == "sphere":
            r = np.float32(o["radius"])
            out[k] = [-r, -r, -r, r, r, r]
        elif o["kind"] == "instance":
            out[k] = out[int(o["of"])]
        else:
            pos = np.ascontiguousarray(o["pos"], np.float32).reshape(-1, 3)
            tri = pos[np.ascontiguousarray(o["idx"], np.uint32).reshape(-1, 3)]
            lo, hi = tri.min(axis=1), tri.max(axis=1)
            hi = np.where(lo >= hi, (lo + np.float32(1.0)).astype(np.float32), hi)
            out[k, :3], out[k, 3:] = lo.min(axis=0), hi.max(axis=0)
    return out


def posed_boxes_numpy(local, Ts):
    """BBox::transform in float32 in the operation order of pose_box (pt_pose.h) / Box::transform (pt_scene.cpp), one rounding per
    operation; an object whose transform equals the identity (as values) keeps its object-space box (Object::bbox)."""
    local, Ts = np.ascontiguousarray(local, np.float32), np.ascontiguousarray(Ts, np.float32).reshape(-1, 16)
    amin, amax = local[:, :3].copy(), local[:, 3:].copy()
    mn = Ts[:, 12:15].copy()
    mx = Ts[:, 12:15].copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                a = (Ts[:, 4 * j + i] * amin[:, j]).astype(np.float32)
                b = (Ts[:, 4 * j + i] * amax[:, j]).astype(np.float32)
                less = a < b
                mn[:, i] = (mn[:, i] + np.where(less, a, b)).astype(np.float32)
                mx[:, i] = (mx[:, i] + np.where(less, b, a)).astype(np.float32)
    has_trans = np.any(Ts != np.eye(4, dtype=np.float32).reshape(16), axis=1)
    return np.where(has_trans[:, None], np.concatenate([mn, mx], axis=1), local)


def top_boxes_numpy(links, order, posed):
    """The refitted boxes restated: links (n, 4) = {start, size, l, r} of the dumped BVH<Object>, order = the 1-based id of every
    slot, posed (nobj, 6) by insertion index.  A leaf's box is the std::min / std::max fold from BBox() of its objects' boxes
    (b < mn ? b : mn - a NaN bound is never taken), an interior node's the same fold of its left and then its right child's."""
    big = np.float32(np.finfo(np.float32).max)
    n = len(links)
    boxes = np.zeros((n, 6), np.float32)

    def enclose(box, other):
        with np.errstate(invalid="ignore"):
            box[:3] = np.where(other[:3] < box[:3], other[:3], box[:3])
            box[3:] = np.where(box[3:] < other[3:], other[3:], box[3:])

    for k in range(n - 1, -1, -1):
        start, size, l, r = (int(v) for v in links[k])
        b = np.array([big, big, big, -big, -big, -big], np.float32)
        if l == r:
            for s in range(start, start + size):
                enclose(b, posed[int(order[s]) - 1])
        else:
            assert l > k and r > k
            enclose(b, boxes[l])
            enclose(b, boxes[r])
        boxes[k] = b
    return boxes


def transforms_of(scene):
    return np.array([o["T"] for o in scene["objects"]], np.float32).reshape(-1, 16)


def expected_top_boxes(scene, idx, Ts, links, order):
    T = transforms_of(scene)
    T[np.asarray(idx, np.int64)] = np.ascontiguousarray(Ts, np.float32).reshape(-1, 16)
    return top_boxes_numpy(links, order, posed_boxes_numpy(local_boxes_numpy(scene), T))


def bits_equal_nan(a, b):
    """Bit equality, with every NaN equal to every NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def particle_indices():
    return np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + IC.PARTICLE_COUNT, dtype=np.uint32)


def scatter(scene, idx, seed=POSE_SEED, spread=0.25):
    """The objects `idx` of the scene moved by a seeded offset of at most spread / 2 per axis: (idx, Ts)."""
    rng = np.random.default_rng(seed)
    idx = np.ascontiguousarray(idx, np.uint32)
    return idx, np.array([IC.translate(scene["objects"][int(i)]["T"], (rng.random(3) - 0.5) * spread) for i in idx], np.float32)


def sweeps_case(S):
    """The rotated, non-uniformly scaled instance (the last object) and one wall of IC.sweeps_scene(), moved."""
    n = len(S["objects"])
    T_inst = IC.translate(S["objects"][n - 1]["T"], (0.3, -0.15, 0.25))
    T_inst[0] *= np.float32(1.25)
    T_wall = IC.translate(S["objects"][1]["T"], (0.0, 0.0, -0.125))
    return np.array([n - 1, 1], np.uint32), np.array([T_inst, T_wall], np.float32)


POOL = 1200


def pool_scene(n=POOL):
    """A pool of n - 1 instances of a 12-triangle cube (and the cube itself) on a jittered grid inside the box of IC.sweeps_scene(),
    whose materials and camera it keeps: a BVH<Object> with levels of more than 256 interior nodes."""
    base = IC.sweeps_scene()
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32).reshape(-1)
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    rng = np.random.default_rng(5)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    cells = np.array([[x, y, z] for x in range(side) for y in range(side) for z in range(side)], np.float32)[:n]
    centres = ((cells + 0.5 + (rng.random((n, 3)).astype(np.float32) - 0.5) * 0.6) / side * 1.6 - 0.8).astype(np.float32)
    objs = []
    for k in range(n):
        T = np.eye(4, dtype=np.float32).reshape(16).copy()
        T[0] = T[5] = T[10] = np.float32(0.02)
        T[12:15] = centres[k] + np.array([0.0, 1.0, 0.0], np.float32)
        objs.append({"kind": "mesh", "pos": v, "nrm": nrm, "idx": idx, "T": T, "material": 0, "is_light": False} if k == 0 else
                    {"kind": "instance", "of": 0, "T": T, "material": 0})
    out = dict(base)
    out["objects"] = objs
    out["name"] = f"pool of {n} cubes"
    return out


def widest_level(links):
    """The largest number of interior nodes on one level of a dumped tree."""
    level = np.zeros(len(links), np.int64)
    for k in range(len(links)):
        l, r = int(links[k][2]), int(links[k][3])
        if l != r:
            level[l] = level[r] = level[k] + 1
    interior = links[:, 2] != links[:, 3]
    return int(np.bincount(level[interior]).max()) if interior.any() else 0


def one_object_scene():
    """IC.sweeps_scene() reduced to its blob: the root of the BVH<Object> is a leaf - no interior record, no level."""
    base = IC.sweeps_scene()
    out = dict(base)
    out["objects"] = [base["objects"][6]]
    return out
