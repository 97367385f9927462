"""Scenes, poses, deformations and the host module of the dynamic-light tests (test_pt_lights_host.py, test_pt_lights_gpu.py):
srt_pt_set_dynamic_lights lets repose / update_mesh / refit_mesh / create_skin take area lights.  The oracle and a fresh commit,
which know nothing of it, are given IC.with_poses(..) / scenes.with_vertices(..) of the description."""
import ctypes

import numpy as np

import _harness as H
import _instance_cases as IC
import _update_cases as UC

F = np.float32
CBOX_LIGHT = 7                   # the Cornell box's emissive quad (two triangles)
BLOB_LIGHT_TRIS = 125            # more than one wave of 64 lanes, and a partial last one


def lights_lib():
    lib = ctypes.CDLL(H.build_host_lib("lights_host", ["lights_host.cpp"]))
    lib.upd_create.restype = ctypes.c_void_p
    lib.upd_clone.restype = ctypes.c_void_p
    lib.upd_error.restype = ctypes.c_char_p
    lib.lit_emu_mismatches.restype = ctypes.c_long
    return lib


def colmajor(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16), F)


def poses(T):
    """The three poses a light with committed transform T is taken through: a translation of T, a rotation about y by 30 degrees
    times scale (0.7, 1, 1.3) in front of T, the identity.  From any committed pose and back to it, has_trans goes 1 -> 0 (into the
    identity) and 0 -> 1 (out of it, or into the translation when T is the identity itself).
    (The Cornell box's own quad under the identity lies on the floor with the floor's centre: the reference's BVH<Object> build does
    not terminate on that description, a fresh commit refuses it and so does the repose - scenes committed with BVHs take the quad
    through the first two poses and see the refusal at the third; the blob, the sphere light and list scenes take all three.)"""
    T = np.ascontiguousarray(T, F).reshape(16)
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    A = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]]) @ np.diag([0.7, 1.0, 1.3, 1.0])
    M = A @ T.astype(np.float64).reshape(4, 4).T
    return {"translation": IC.translate(T, (0.1, -0.15, 0.05)), "rotation * scale": colmajor(M), "identity": np.eye(4, dtype=F).reshape(16)}


def blob_light_arrays(seed=5, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """(pos, nrm, idx) of blob_mesh(2, seed) without its last three faces - 125 triangles - flat shaded."""
    scenes = IC.scenes_module()
    v, f = scenes.blob_mesh(2, seed)
    v = (v * np.asarray(scale, F) + np.asarray(shift, F)).astype(F)
    return scenes.flat_mesh(v, f[:BLOB_LIGHT_TRIS])


def blob_light_deformations():
    base = blob_light_arrays()
    out = {"D1": blob_light_arrays(seed=9), "D2": blob_light_arrays(scale=(1.3, 0.8, 1.0)), "D3": blob_light_arrays(shift=(0.0625, 0.0, 0.0))}
    for name, (p, n, i) in out.items():
        assert np.array_equal(i, base[2]) and p.shape == base[0].shape, name
    return {k: (p, n) for k, (p, n, _) in out.items()}


BLOB_LIGHT = 8


def blob_light_scene():
    """The Cornell box plus an emissive 125-triangle blob (object 8) under a transform of its own: a light that deforms."""
    s = IC.scenes_module().cornell_box("cbox")
    s = dict(s, objects=list(s["objects"]))
    p, n, i = blob_light_arrays()
    T = np.array([[0.8, 0, 0, -0.25], [0, 1.1, 0, 0.55], [0, 0, 0.7, -0.1], [0, 0, 0, 1]], F)
    assert len(s["objects"]) == BLOB_LIGHT
    s["objects"].append({"kind": "mesh", "pos": p, "nrm": n, "idx": i, "T": colmajor(T), "material": 7, "is_light": True})
    s["name"] = "cbox+lightblob125"
    return s


def three_light_scene():
    """sweeps_scene() plus an emissive sphere (object 9) and a second emissive quad (object 10): lights 0 (object 7), 1 and 2."""
    S = IC.sweeps_scene()
    light = S["objects"][CBOX_LIGHT]
    I = np.eye(4, dtype=F).reshape(16)
    S["objects"].append({"kind": "sphere", "radius": 0.05, "T": IC.translate(I, (0.3, 0.8, 0.3)), "material": 7,
                         "light_mesh": {"pos": light["pos"], "nrm": light["nrm"], "idx": light["idx"]}})
    T = np.array([[0.3, 0, 0, -0.45], [0, 0.3, 0, 0.35], [0, 0, 0.3, 0.25], [0, 0, 0, 1]], F)
    S["objects"].append(dict(light, T=colmajor(T @ np.asarray(light["T"], F).reshape(4, 4).T)))
    S["name"] = "cbox+blob512+instance+3lights"
    return S


class LightScene(UC.HostScene):
    """A BuiltScene behind tests/host_emu/lights_host.cpp: UC.HostScene's calls (the module includes update_host.cpp) plus the
    switch, refit, the light comparisons and the light dump."""

    def __init__(self, scene=None, use_bvh=True, dynamic=False, _handle=None, may_fail=False):
        """may_fail: a description whose build the scene layer refuses leaves .failed set to the message instead of asserting."""
        self.failed = None
        self.lib = L = lights_lib()
        self.use_bvh = use_bvh
        if _handle is not None:
            self.h_ = ctypes.c_void_p(_handle)
            return
        self.h_ = ctypes.c_void_p(L.upd_create())
        for m in scene["materials"]:
            L.upd_add_material(self.h_, int(m["type"]), H.P(H._f32(m["a"])), H.P(H._f32(m["b"])), ctypes.c_float(float(m["ior"])))
        for o in scene["objects"]:
            T = H._f32(o["T"])
            mesh = o if o["kind"] == "mesh" else o.get("light_mesh")
            if mesh is not None:
                pos, nrm, idx = H._f32(mesh["pos"]), H._f32(mesh["nrm"]), np.ascontiguousarray(mesh["idx"], np.uint32)
            if o["kind"] == "mesh":
                L.upd_add_mesh(self.h_, H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx), H.P(T), int(o["material"]), int(bool(o["is_light"])))
            elif o["kind"] == "instance":
                L.upd_add_instance(self.h_, int(o["of"]), H.P(T), int(o["material"]))
            elif mesh is not None:
                L.upd_add_sphere_light(self.h_, ctypes.c_float(float(o["radius"])), H.P(T), int(o["material"]), H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx))
            else:
                L.upd_add_sphere(self.h_, ctypes.c_float(float(o["radius"])), H.P(T), int(o["material"]))
        L.lit_set_dynamic(self.h_, int(dynamic))
        rc = L.upd_commit(self.h_, int(use_bvh))
        if rc != 0 and may_fail:
            self.failed = L.upd_error(self.h_).decode()
            return
        assert rc == 0, L.upd_error(self.h_).decode()
        assert bool(L.lit_get_dynamic(self.h_)) == bool(dynamic)              # a commit keeps the switch

    def clone(self):
        return LightScene(use_bvh=self.use_bvh, _handle=self.lib.upd_clone(self.h_))

    def set_dynamic(self, on):
        self.lib.lit_set_dynamic(self.h_, int(bool(on)))

    def refit(self, index, pos, nrm, nverts=None):
        pos, nrm = H._f32(pos), H._f32(nrm)
        return self.lib.lit_refit(self.h_, int(index), H.P(pos), H.P(nrm), len(pos) if nverts is None else int(nverts))

    def same_computed(self, other):
        return bool(self.lib.lit_same_computed(self.h_, other.h_))

    def same_but_trees(self, other):
        return bool(self.lib.lit_same_but_trees(self.h_, other.h_))

    def identical(self, other):
        return bool(self.lib.lit_identical(self.h_, other.h_))

    def dump_lights(self):
        nl, nt = self.lib.lit_light_count(self.h_), self.lib.lit_light_tri_count(self.h_)
        heads, mats, tris = np.zeros((nl, 4), np.uint32), np.zeros((nl, 4, 16), F), np.zeros((nt, 31), F)
        self.lib.lit_dump(self.h_, H.P(heads), H.P(mats), H.P(tris))
        return {"heads": heads, "mats": mats, "tris": tris}


def lights_equal(a, b):
    """Two dump_lights() results, bit for bit."""
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in ("heads", "mats", "tris"))


def light_rows(d, light):
    """The rows of one light in a dump: (head, matrices, its triangles)."""
    first, n = int(d["heads"][light, 1]), int(d["heads"][light, 2])
    return d["heads"][light].copy(), d["mats"][light].view(np.uint32).copy(), d["tris"][first:first + n].view(np.uint32).copy()


def rows_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))
