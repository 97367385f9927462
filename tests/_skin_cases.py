"""Rigs and meshes of the skinning tests (test_pt_skin_host.py, test_pt_skin_gpu.py, tests/golden/make_skin_golden.py).

RIGS are what make_skin_golden.py runs through the reference (its own Skeleton, in its own Skeleton::for_joints order) and
records as tests/golden/skin_<name>.npz.  Everything else here is generated: joint matrices built in float64 and rounded to
float32 - any float32 matrices are valid inputs; the expected values for them come from _skin_expected.py."""
import os

import numpy as np

import _harness as H
import _skin_expected as E

F = np.float32


def blob_object_mesh():
    """(pos, nrm, idx) of object 6 of cbox+blob512 (_update_cases.blob_scene()), in object space."""
    import _update_cases as UC

    o = UC.blob_scene()["objects"][UC.BLOB_OBJECT]
    return np.ascontiguousarray(o["pos"], F), np.ascontiguousarray(o["nrm"], F), np.ascontiguousarray(o["idx"], np.uint32)


def small_blob_mesh():
    import _update_cases as UC

    return UC.blob_arrays(2, seed=5)


# name -> mesh, joints in the caller's order (parent, extent, radius), base, and the poses (Euler angles in degrees per joint)
def rigs():
    return {
        "blob_chain3": {"mesh": blob_object_mesh, "parent": [-1, 0, 1], "extent": [[0, 0.09, 0]] * 3, "radius": [0.16, 0.15, 0.16], "base": [0.01, -0.14, 0.0],
                        "poses": [[[0, 0, 12], [10, 0, -20], [0, 15, 25]], [[5, 30, -8], [-12, 0, 14], [20, -10, 0]]]},
        "blob128_tree5": {"mesh": small_blob_mesh, "parent": [-1, 0, 0, 2, -1], "extent": [[0, 0.4, 0], [0.3, 0.2, 0], [-0.3, 0.25, 0.1], [0, 0.3, 0.2], [0.1, -0.5, 0]],
                          "radius": [0.9, 0.6, 0.7, 0.5, 0.8], "base": [0.05, -0.3, 0.02], "poses": [[[10, 0, 20], [0, 40, 0], [-15, 5, 30], [25, 0, -10], [0, 0, 45]]]},
    }


def load_fixture(name):
    g = np.load(os.path.join(H.GOLDEN, f"skin_{name}.npz"))
    joints = np.zeros(len(g["radius"]), E.JOINT_DTYPE)
    joints["bind"], joints["extent"], joints["radius"] = g["bind"], g["extent"], g["radius"]
    return g, joints


# ---- generated rigs ----
def _translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def _euler(deg):
    x, y, z = np.radians(np.asarray(deg, np.float64))
    rx = np.array([[1, 0, 0, 0], [0, np.cos(x), -np.sin(x), 0], [0, np.sin(x), np.cos(x), 0], [0, 0, 0, 1]])
    ry = np.array([[np.cos(y), 0, np.sin(y), 0], [0, 1, 0, 0], [-np.sin(y), 0, np.cos(y), 0], [0, 0, 0, 1]])
    rz = np.array([[np.cos(z), -np.sin(z), 0, 0], [np.sin(z), np.cos(z), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return rz @ ry @ rx


def _data(m):
    return np.ascontiguousarray(m.T.reshape(16), F)          # Mat4::data: column-major


def chain(base, extents, radii):
    """A chain of joints, each the child of the one before: JOINT_DTYPE records with bind = translate(base + the extents in front)."""
    joints = np.zeros(len(extents), E.JOINT_DTYPE)
    at = np.asarray(base, np.float64)
    for k, e in enumerate(extents):
        joints[k] = (_data(_translate(at)), np.asarray(e, F), F(radii[k]))
        at = at + np.asarray(e, np.float64)
    return joints


def chain_posed(base, extents, angles):
    """joint_to_posed of the chain's joints under Euler angles (degrees) per joint: (njoints, 16)."""
    out, m = [], _translate(base)
    for k, e in enumerate(extents):
        m = m @ _euler(angles[k])
        out.append(_data(m))
        m = m @ _translate(e)
    return np.stack(out)


def blob_chain():
    """The three-joint chain through cbox+blob512's blob that pose() is tested with, and two sets of angles."""
    base, extents = [0.0, -0.13, 0.01], [[0, 0.09, 0]] * 3
    joints = chain(base, extents, [0.15, 0.16, 0.15])
    poses = [chain_posed(base, extents, a) for a in ([[0, 0, 10], [8, 0, -15], [0, 12, 20]], [[4, 25, -6], [-10, 0, 12], [15, -8, 0]])]
    return joints, poses


def edge_mesh(nverts, njoints, seed=1):
    """nverts vertices, njoints joints, with the cases a skinning kernel can get wrong placed at fixed vertices when there is room:
    joint 0 is the bone (0,1,0) from the origin with radius 0.25 (identity bind: joint space is object space).
      vertex 0: (0.25, 0.5, 0): at exactly `radius` from bone 0 - included;        vertex 1: one ulp further out - excluded;
      vertex 2: behind the start (dot <= 0: closest returns start);                vertex 3: beside the bone (returns proj);
      vertex 4: past the end (returns end);                                        vertex 5: far from every joint (keeps its position).
    The last joint, when there are at least three, has zero extent (closest returns start for every vertex); the joints in
    between are a fan around the origin with radii up to 0.9, so that the random vertices have up to njoints influences.
    Triangles: vertex v names triangles (v, v+1, v+2) for every second v - most vertices are shared by several - the very last
    vertex is named by none, and one triangle is degenerate (three times the same vertex: unit() of a zero cross is NaN)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.6, 0.6, (nverts, 3)).astype(F)
    fixed = np.array([[0.25, 0.5, 0], [np.nextafter(F(0.25), F(1)), 0.5, 0], [0.1, -0.125, 0.05], [0.125, 0.25, -0.0625], [0.0625, 1.125, 0.125], [40, 40, 40]], F)
    pos[:min(nverts, len(fixed))] = fixed[:nverts]
    nrm = rng.normal(size=(nverts, 3)).astype(F)
    joints = np.zeros(njoints, E.JOINT_DTYPE)
    angles = []
    for j in range(njoints):
        if j == 0:
            joints[j] = (_data(np.eye(4)), F([0, 1, 0]), F(0.25))
        elif j == njoints - 1 and njoints >= 3:
            joints[j] = (_data(_translate([0.1, 0.1, -0.1])), F([0, 0, 0]), F(0.7))
        else:
            a = 2.0 * np.pi * j / njoints
            joints[j] = (_data(_translate([0.2 * np.cos(a), -0.1, 0.2 * np.sin(a)]) @ _euler([7 * j, 0, 11 * j])), F([0.3 * np.cos(a), 0.2, 0.3 * np.sin(a)]), F(0.3 + 0.6 * (j % 5) / 4))
        angles.append([13 * j % 50, -7 * j % 40, 5 * j % 60])
    posed = np.stack([_data(_translate([0.02 * j, 0.01, -0.01 * j]) @ _euler(angles[j])) for j in range(njoints)])
    tris = [[v, v + 1, v + 2] for v in range(0, nverts - 3, 2)]
    if nverts >= 4:
        tris.insert(len(tris) // 2, [2, 2, 2])
    idx = np.array(tris if tris else [[0, 0, 0]], np.uint32).reshape(-1)
    return pos, nrm, idx, joints, posed


def single_mesh_scene(pos, nrm, idx):
    """A scene with one Lambertian mesh and a camera: what a skin of an edge mesh is bound to."""
    scenes = __import__("_instance_cases").scenes_module()
    s = scenes.cornell_with_mesh(1, "glass")
    keep = dict(s)
    mesh = [o for o in s["objects"] if o["kind"] == "mesh" and not o.get("is_light")][0]
    keep["objects"] = [dict(mesh, pos=np.ascontiguousarray(pos, F), nrm=np.ascontiguousarray(nrm, F), idx=np.ascontiguousarray(idx, np.uint32))]
    return keep
