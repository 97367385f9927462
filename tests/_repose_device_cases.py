"""Cases and helpers of the device-repose tests (test_pt_repose_device_host.py, test_pt_repose_device_gpu.py): the host module
over pt_pose.h (tests/host_emu/pose_host.cpp), the matrices and boxes the device functions are compared on, the numpy
restatement of translate * scale, and the scene file the sanitized stand-alone program reads."""
import ctypes
import struct

import numpy as np

import _harness as H
import _instance_cases as IC
from _cases import pt_scene

PARTICLE_SCALE = np.float32(0.03)          # pt_scene("cbox_particles"): Mat4::translate(p.pos) * Mat4::scale(0.03)


def pose_lib():
    lib = ctypes.CDLL(H.build_host_lib("pose_host", ["pose_host.cpp"]))
    lib.pose_emu_mismatches.restype = ctypes.c_long
    lib.pose_ts_mismatches.restype = ctypes.c_long
    lib.pose_ts_mismatches.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float]
    lib.pose_ts_reference.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p]
    return lib


def identity():
    return np.eye(4, dtype=np.float32).reshape(16)


def translate_scale(pos, scale):
    """Column-major translate(pos) * scale(scale), written down directly (not through the product)."""
    T = identity()
    T[0] = T[5] = T[10] = np.float32(scale)
    T[12:15] = np.asarray(pos, np.float32)
    return T


def matrix_cases():
    """{name: (k, 16) float32} - the matrices the device functions are held to the host functions on."""
    rng = np.random.default_rng(2024)
    neg_zero = identity()
    neg_zero[[1, 2, 4, 6, 8, 9, 12, 13, 14]] = np.float32(-0.0)
    sweeps = IC.sweeps_scene()["objects"][-1]["T"]
    particles = np.array([o["T"] for o in pt_scene("cbox_particles")["objects"]], np.float32)
    denormal = identity()
    denormal[0], denormal[5], denormal[12], denormal[6] = np.float32(1e-39), np.float32(3e-41), np.float32(-2e-40), np.float32(1e-44)
    singular = identity()
    singular[10] = np.float32(0.0)                        # det 0
    singular2 = np.ones(16, np.float32)                   # every cofactor 0 as well: 0 / 0
    nan = translate_scale((0.1, 0.2, 0.3), 0.5)
    nan[5] = np.float32(np.nan)
    mirrored = translate_scale((-0.0, -0.0, -0.0), -2.0)
    mirrored[[1, 2, 4, 6, 8, 9]] = np.float32(-0.0)         # bounds of the unit box that come out as -0: their sign is compared too
    random = (rng.random((300, 16), np.float32) - np.float32(0.5)) * np.float32(4.0)
    affine = random[:150].copy()
    affine[:, [3, 7, 11]] = 0.0
    affine[:, 15] = 1.0
    return {"identity": identity()[None], "identity with -0": neg_zero[None], "translate * scale": translate_scale((0.25, -0.5, 0.125), 0.03)[None],
            "rotated, non-uniform scale": np.asarray(sweeps, np.float32).reshape(1, 16), "cbox_particles": particles, "denormal": denormal[None],
            "mirrored at -0": mirrored[None], "singular": np.stack([singular, singular2]), "NaN": nan[None], "random": random, "random affine": affine}


def box_cases():
    """The unit box, a box with a flat axis widened by +1 (Triangle::bbox), the empty BBox()."""
    big = np.float32(np.finfo(np.float32).max)
    return np.array([[0, 0, 0, 1, 1, 1], [-0.5, 0.25, -0.5, 0.5, 1.25, 0.5], [big, big, big, -big, -big, -big]], np.float32)


def translate_scale_product(pos, scale):
    """Mat4::translate(pos_k) * Mat4::scale(Vec3{scale}) for every row of pos as Mat4::operator* forms it (mat_mul(translate, scale)
    of pt_scene.cpp): out[i][j] = sum over k, accumulated from 0.0f in order, of S[i][k] * T[k][j] - in float32, one rounding per
    operation.  (n, 16) float32, column-major."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    T = np.tile(identity(), (n, 1))
    T[:, 12:15] = pos
    S = np.tile(identity(), (n, 1))
    S[:, 0] = S[:, 5] = S[:, 10] = np.float32(scale)
    out = np.zeros((n, 16), np.float32)
    for i in range(4):
        for j in range(4):
            acc = np.zeros(n, np.float32)
            for k in range(4):
                acc = (acc + (S[:, 4 * i + k] * T[:, 4 * k + j]).astype(np.float32)).astype(np.float32)
            out[:, 4 * i + j] = acc
    return out


def particle_positions(S):
    """(60, 3): where the particles of the shared particle scene are."""
    return np.array([S["objects"][IC.PARTICLE_FIRST + k]["T"][12:15] for k in range(IC.PARTICLE_COUNT)], np.float32)


def write_scene_file(path, scene, indices, Ts):
    """The file tests/host_emu/repose_device_sanitized_main.cpp reads: materials, objects, the repose list (its header comment)."""
    out = []
    u32 = lambda *v: out.append(struct.pack("<%dI" % len(v), *[int(x) for x in v]))
    f32 = lambda a: out.append(np.ascontiguousarray(a, np.float32).reshape(-1).astype("<f4").tobytes())
    u32(len(scene["materials"]))
    for m in scene["materials"]:
        u32(m["type"]); f32(m["a"]); f32(m["b"]); f32([m["ior"]])
    u32(len(scene["objects"]))
    for o in scene["objects"]:
        mesh = o if o["kind"] == "mesh" else o.get("light_mesh")
        kind = {"mesh": 0, "sphere": 1, "instance": 2}[o["kind"]]
        is_light = bool(o.get("is_light")) or (kind == 1 and mesh is not None)
        u32(kind, int(is_light), o["material"], o.get("of", 0))
        f32([o.get("radius", 0.0)]); f32(o["T"])
        if mesh is None:
            u32(0, 0)
        else:
            pos, idx = H._f32(mesh["pos"]).reshape(-1, 3), np.ascontiguousarray(mesh["idx"], np.uint32).reshape(-1)
            u32(len(pos), len(idx)); f32(pos); f32(mesh["nrm"])
            out.append(idx.astype("<u4").tobytes())
    idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
    u32(len(idx))
    out.append(idx.astype("<u4").tobytes())
    f32(np.ascontiguousarray(Ts, np.float32).reshape(len(idx), 16))
    with open(path, "wb") as f:
        f.write(b"".join(out))
