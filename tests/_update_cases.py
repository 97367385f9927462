"""Deformations, scenes and the host module of the mesh-update tests (test_pt_update_host.py, test_pt_update_gpu.py).

A deformation is a (pos, nrm) pair for a mesh of the scene: same vertex count, same index buffer.  The oracle and a fresh commit,
which know nothing of updates, are given scenes.with_vertices(S, index, pos, nrm).

Node counts of the BVH<Triangle> of cornell_with_mesh(3) object 6 (blob_mesh(3, seed 7), 512 triangles) under the deformations,
from the oracle's dumps (test_pt_update_host.py::test_deformations_exercise_both_storage_paths asserts them):
    original 315, D1 323, D2 325, D3 315
D1 and D2 change the node count (the ranges stored behind the mesh move); D3, a translation, keeps it."""
import ctypes

import numpy as np

import _harness as H
import _instance_cases as IC

BLOB_OBJECT = 6
NODES = {"original": 315, "D1": 323, "D2": 325, "D3": 315}


def blob_arrays(n_subdiv, seed=7, scale=(1.0, 1.0, 1.0), shift=(0.0, 0.0, 0.0)):
    """(pos, nrm, idx) of blob_mesh(n_subdiv, seed) scaled and shifted, flat shaded as cornell_with_mesh does."""
    scenes = IC.scenes_module()
    v, f = scenes.blob_mesh(n_subdiv, seed)
    v = (v * np.asarray(scale, np.float32) + np.asarray(shift, np.float32)).astype(np.float32)
    return scenes.flat_mesh(v, f) if len(f) <= 4096 else scenes._flat_mesh_fast(v, f)


def deformations(n_subdiv=3):
    """{"D1": (pos, nrm), ..} for blob_mesh(n_subdiv); every one has the faces - and so, after flat_mesh, the idx - of seed 7."""
    base = blob_arrays(n_subdiv)
    out = {"D1": blob_arrays(n_subdiv, seed=11), "D2": blob_arrays(n_subdiv, scale=(1.3, 0.8, 1.0)), "D3": blob_arrays(n_subdiv, shift=(0.0625, 0.0, 0.0))}
    for name, (p, n, i) in out.items():
        assert np.array_equal(i, base[2]) and p.shape == base[0].shape, name
    return {k: (p, n) for k, (p, n, _) in out.items()}


def original(scene, index):
    o = scene["objects"][index]
    return np.ascontiguousarray(o["pos"], np.float32), np.ascontiguousarray(o["nrm"], np.float32)


def blob_scene():
    return IC.scenes_module().cornell_with_mesh(3, "glass")


def two_mesh_scene():
    """cbox+blob512 plus blob_mesh(2, seed 5) (128 triangles) under a transform of its own: objects 6 and 8 are meshes that can be
    updated, with a real BVH<Triangle> each."""
    scenes = IC.scenes_module()
    s = blob_scene()
    v, f = scenes.blob_mesh(2, seed=5)
    p, n, i = scenes.flat_mesh(v, f)
    T = np.array([[0.8, 0, 0, -0.25], [0, 1.1, 0, 0.55], [0, 0, 0.7, -0.1], [0, 0, 0, 1]], np.float32)
    s["objects"].append({"kind": "mesh", "pos": p, "nrm": n, "idx": i, "T": np.ascontiguousarray(T.T.reshape(16)), "material": 5, "is_light": False})
    s["name"] = "cbox+blob512+blob128"
    return s


def small_blob_deformation():
    p, n, _ = blob_arrays(2, seed=9, scale=(1.2, 0.9, 1.1))
    return p, n


def flat_chain_scene():
    """The Cornell box with a mesh of deep_over's vertex count and index buffer (53 triangles, three vertices each) laid out side by
    side - a shallow tree - in place of the glass sphere, and the chain geometry of deep_over itself as the deformation whose
    BVH<Triangle> nests 49 deep."""
    from _cases import DEEP_CHAIN_TRIANGLES, chain_mesh, pt_scene

    deep = pt_scene("deep_over")
    n = DEEP_CHAIN_TRIANGLES["deep_over"]
    k = np.arange(n, dtype=np.float32)
    tri = np.array([[0, 0, 0], [0.08, 0, 0], [0, 0.08, 0.02]], np.float32)
    # (placed off the box's centre: an object whose centre coincides with the walls' makes the BVH<Object> build non-terminating)
    v = (tri[None] + np.stack([0.1 * (k % 8) - 0.5, 0.1 * (k // 8) - 0.2, 0.01 * k - 0.1], 1)[:, None, :]).reshape(-1, 3).astype(np.float32)
    scenes = IC.scenes_module()
    p, nr, ix = scenes.flat_mesh(v, chain_mesh(n)[1])
    chain = deep["objects"][6]
    assert np.array_equal(ix, chain["idx"])
    s = dict(deep)
    s["objects"] = list(deep["objects"])
    s["objects"][6] = dict(chain, pos=p, nrm=nr)
    s["name"] = "cbox+flatchain53"
    return s, (np.ascontiguousarray(chain["pos"], np.float32), np.ascontiguousarray(chain["nrm"], np.float32))


def one_point(scene, index):
    """Every vertex of the mesh at one point: the reference's BVH<Triangle> build does not terminate."""
    p, n = original(scene, index)
    return np.full_like(p, 0.125), n


def update_lib():
    lib = ctypes.CDLL(H.build_host_lib("update_host", ["update_host.cpp"]))
    lib.upd_create.restype = ctypes.c_void_p
    lib.upd_clone.restype = ctypes.c_void_p
    lib.upd_error.restype = ctypes.c_char_p
    lib.upd_emu_mismatches.restype = ctypes.c_long
    return lib


class HostScene(H._SceneFeeder):
    """A BuiltScene of the scene layer (pt_scene.cpp) behind tests/host_emu/update_host.cpp."""

    def __init__(self, scene=None, use_bvh=True, _handle=None):
        self.lib = update_lib()
        self.use_bvh = use_bvh
        if _handle is not None:
            self.h_ = ctypes.c_void_p(_handle)
            return
        self.h_ = ctypes.c_void_p(self.lib.upd_create())
        for m in scene["materials"]:
            self.lib.upd_add_material(self.h_, int(m["type"]), H.P(H._f32(m["a"])), H.P(H._f32(m["b"])), ctypes.c_float(float(m["ior"])))
        for o in scene["objects"]:
            T = H._f32(o["T"])
            if o["kind"] == "mesh":
                pos, nrm, idx = H._f32(o["pos"]), H._f32(o["nrm"]), np.ascontiguousarray(o["idx"], np.uint32)
                self.lib.upd_add_mesh(self.h_, H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx), H.P(T), int(o["material"]), int(bool(o["is_light"])))
            elif o["kind"] == "instance":
                self.lib.upd_add_instance(self.h_, int(o["of"]), H.P(T), int(o["material"]))
            elif o.get("light_mesh") is not None:
                lm = o["light_mesh"]
                pos, nrm, idx = H._f32(lm["pos"]), H._f32(lm["nrm"]), np.ascontiguousarray(lm["idx"], np.uint32)
                self.lib.upd_add_sphere_light(self.h_, ctypes.c_float(float(o["radius"])), H.P(T), int(o["material"]), H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx))
            else:
                self.lib.upd_add_sphere(self.h_, ctypes.c_float(float(o["radius"])), H.P(T), int(o["material"]))
        rc = self.lib.upd_commit(self.h_, int(use_bvh))
        assert rc == 0, self.lib.upd_error(self.h_).decode()

    def clone(self):
        return HostScene(use_bvh=self.use_bvh, _handle=self.lib.upd_clone(self.h_))

    def update(self, index, pos, nrm, nverts=None):
        """0 applied, 1 refused argument, 2 unsupported (srt_pt_update_mesh's INVALID / UNSUPPORTED)."""
        pos, nrm = H._f32(pos), H._f32(nrm)
        return self.lib.upd_update(self.h_, int(index), H.P(pos), H.P(nrm), len(pos) if nverts is None else int(nverts))

    def repose(self, indices, Ts):
        idx, T = np.ascontiguousarray(indices, np.uint32), H._f32(Ts).reshape(-1, 16)
        return self.lib.upd_repose(self.h_, H.P(idx), H.P(T), len(idx))

    def error(self):
        return self.lib.upd_error(self.h_).decode()

    def same_computed(self, other):
        return bool(self.lib.upd_same_computed(self.h_, other.h_))

    def identical(self, other):
        return bool(self.lib.upd_identical(self.h_, other.h_))

    def store(self, index):
        out = np.zeros(4, np.uint32)
        self.lib.upd_store(self.h_, int(index), H.P(out))
        return dict(zip(("nodes", "records", "node_off", "rec_base"), (int(v) for v in out)))

    def depths(self):
        out = np.zeros(2, np.uint32)
        self.lib.upd_depths(self.h_, H.P(out))
        return int(out[0]), int(out[1])

    def local_box(self, index):
        out = np.zeros(6, np.float32)
        self.lib.upd_local_box(self.h_, int(index), H.P(out))
        return out

    def close(self):
        if self.h_:
            self.lib.upd_destroy(self.h_)
            self.h_ = None
