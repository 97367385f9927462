"""Scenes, expectations and the host emulation of the refit tests (test_pt_refit_host.py, test_pt_refit_emu_host.py,
test_pt_refit_gpu.py).

A refit keeps a mesh's BVH<Triangle> and gives it new boxes, so the refitted scene is NOT the scene a fresh commit of the new
vertices builds: the oracle, which only builds, walks another tree.  What a refitted scene must compute is defined by the host
refit (refit_boxes / apply_mesh_refit, pt_scene.cpp) walked by the device headers compiled for the host
(tests/host_emu/refit_flat_host.cpp): EmuRefit below."""
import ctypes

import numpy as np

import _harness as H
import _instance_cases as IC
import _update_cases as UC
from _cases import random_rays

W = HT = 64
DEPTH, SPP, SEED = 8, 4, 9
RAY_SEED, RAYS = 3, 2048


DEEP = (32, 32, 5, 2)            # w, h, depth, spp of the deep-tree case
DEEP_MESH = 23                   # the chain of pt_scene("deep_both")


def deep_moved(scene):
    """The chain's vertices moved by a seeded offset of at most 5e-4 per coordinate (seed 0: the reference's build of the moved
    chain still nests 48; with seed 1 it nests deeper and the oracle refuses the commit - a refit does not care)."""
    p, n = UC.original(scene, DEEP_MESH)
    return (p + (np.random.default_rng(0).random(p.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(1e-3)).astype(np.float32), n


def emu_lib():
    lib = ctypes.CDLL(H.build_host_lib("refit_flat_host", ["refit_flat_host.cpp"], scene_layer=True))
    lib.emu_refit_create.restype = ctypes.c_void_p
    return lib


class EmuRefit(H.EmuPT):
    """The scene layer's build, then host refits, walked by the device headers on the CPU."""

    def __init__(self, scene, w=W, h=HT, depth=DEPTH):
        self.lib = emu_lib()
        self.h_ = ctypes.c_void_p(self.lib.emu_refit_create())
        self.use_bvh = True
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

    def refit(self, index, pos, nrm):
        pos, nrm = H._f32(pos), H._f32(nrm)
        return self.lib.emu_refit(self.h_, int(index), H.P(pos), H.P(nrm), len(pos))

    def trace_samples(self, seed, xs, ys, ss, normals=False):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        rgb, draws, rays = np.zeros((len(xs), 3), np.float32), np.zeros(len(xs), np.uint32), np.zeros(len(xs), np.uint32)
        self.lib.emu_trace_samples(self.h_, ctypes.c_uint64(seed), H.P(xs), H.P(ys), H.P(ss), ctypes.c_size_t(len(xs)), int(normals), H.P(rgb), H.P(draws), H.P(rays))
        return rgb, draws, rays

    def close(self):
        self.lib.emu_refit_destroy(self.h_)

    def hit9(self, org, dirs, bounds):
        """(nested, flat): srt_pt_hit's nine floats per ray from the nested walk and from the flattened walk."""
        org, dirs, bounds = H._f32(org), H._f32(dirs), H._f32(bounds)
        a, b = np.zeros((len(org), 9), np.float32), np.zeros((len(org), 9), np.float32)
        self.lib.emu_hit9(self.h_, H.P(org), H.P(dirs), H.P(bounds), ctypes.c_size_t(len(org)), H.P(a), H.P(b))
        return a, b


def every_sample(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32), ss.reshape(-1).astype(np.uint32)


def epoch_of(rgb, w, h, spp):
    """do_trace's epoch mean from per-sample radiance in every_sample order: valid samples summed in sample order, times 1 / count
    (pt_epoch_kernel, rays/pathtracer.cpp:250-280)."""
    s = np.ascontiguousarray(rgb, np.float32).reshape(h, w, spp, 3)
    acc = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros((h, w), np.uint32)
    for k in range(spp):
        ok = np.all(np.isfinite(s[:, :, k]), axis=2)      # Spectrum::valid
        acc = np.where(ok[..., None], (acc + s[:, :, k]).astype(np.float32), acc)
        cnt += ok
    inv = (np.float32(1.0) / np.maximum(cnt, 1).astype(np.float32)).astype(np.float32)
    return np.where(cnt[..., None] > 0, (acc * inv[..., None]).astype(np.float32), acc)


def expectation(scene, refits, w=W, h=HT, depth=DEPTH, spp=SPP, normals=False):
    """What a context must compute after `refits` = [(index, pos, nrm), ..] on `scene`: every sample, the epoch image, the hit
    records of both walks."""
    e = EmuRefit(scene, w, h, depth)
    for index, p, n in refits:
        assert e.refit(index, p, n) == 0
    org, d, b = random_rays(RAY_SEED, RAYS)
    samples = e.trace_samples(SEED, *every_sample(w, h, spp))
    out = {"samples": samples, "epoch": epoch_of(samples[0], w, h, spp), "hits": e.hit9(org, d, b)}
    if normals:
        out["normals"] = e.trace_samples(SEED, *every_sample(w, h, spp), normals=True)
    e.close()
    return out


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def refit_boxes_numpy(links, order_tris, pos, idx):
    """The refitted boxes restated: links (n, 4) = {start, size, l, r} of a dumped tree, order_tris = the triangle index of every
    primitive slot.  A leaf's box is the min / max fold of its triangles' Triangle::bbox (a flat axis: max = min + 1.0f), an
    interior node's the enclose of its children's (children lie behind their parent)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    tri = pos[np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)]            # (ntri, 3 corners, 3)
    lo, hi = tri.min(axis=1), tri.max(axis=1)
    hi = np.where(lo >= hi, (lo + np.float32(1.0)).astype(np.float32), hi)
    n = len(links)
    boxes = np.zeros((n, 6), np.float32)
    for k in range(n - 1, -1, -1):
        start, size, l, r = (int(v) for v in links[k])
        if l == r:
            t = order_tris[start:start + size]
            boxes[k, :3], boxes[k, 3:] = lo[t].min(axis=0), hi[t].max(axis=0)
        else:
            assert l > k and r > k
            boxes[k, :3], boxes[k, 3:] = np.minimum(boxes[l, :3], boxes[r, :3]), np.maximum(boxes[l, 3:], boxes[r, 3:])
    return boxes


def tree_cost_numpy(boxes, links):
    b = np.asarray(boxes, np.float64)
    e = b[:, 3:] - b[:, :3]
    sa = 2.0 * (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])
    leaf = links[:, 2] == links[:, 3]
    w = np.where(leaf, links[:, 1].astype(np.float64), 1.0)
    return float(np.sum(w * sa / sa[0]))


def slot_of(pt_or_dump, index, nobj=None):
    """The object slot of insertion index `index` in a TLAS dump's order (1-based ids)."""
    order = pt_or_dump[2] if isinstance(pt_or_dump, tuple) else pt_or_dump.dump_bvh(-1)[2]
    n = nobj if nobj is not None else len(order)
    return [k for k in range(n) if order[k] == index + 1][0]


def refusal_scene():
    """Objects: 0-4 walls, 5 sphere, 6 blob, 7 area light, 8 instance of 6, 9 emissive sphere."""
    S = IC.sweeps_scene()
    light = S["objects"][7]
    S["objects"].append({"kind": "sphere", "radius": 0.05, "T": IC.translate(np.eye(4, dtype=np.float32).reshape(16), (0.3, 0.8, 0.3)), "material": 7,
                         "light_mesh": {"pos": light["pos"], "nrm": light["nrm"], "idx": light["idx"]}})
    return S


def refused_arguments(S):
    """(what, index, pos, nrm, nverts or None for len(pos)) of refusal_scene(): every argument srt_pt_update_mesh refuses."""
    p, n = UC.deformations()["D1"]
    lp, ln = UC.original(S, 7)
    return [("out of range", len(S["objects"]), p, n, None), ("a sphere", 5, p, n, None), ("a sphere light", 9, lp, ln, None),
            ("an instance", 8, p, n, None), ("an area light", 7, lp, ln, None), ("another vertex count", 6, p[:-3], n[:-3], None),
            ("a vertex too many", 6, p, n, len(p) + 1)]
