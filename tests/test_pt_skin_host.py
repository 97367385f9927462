"""CPU: skinning (srt_pt_skin_*) without a device.  The numpy restatement tests/_skin_expected.py against results recorded from the
reference (tests/golden/skin_*.npz); the per-vertex device functions of pt_skin.h compiled for the host - plain and with
AddressSanitizer / UndefinedBehaviorSanitizer, as a stand-alone program - against the same recordings; and the ABI: the symbols,
the header, and every entry point's argument validation on a host-only context, which has no skinning (there is no CPU path)."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _skin_cases as SC
import _skin_expected as E
import _update_cases as UC
from test_pt_update_host import refusal_scene

INVALID, UNSUPPORTED, STATE = -1, -4, -5
RIGS = sorted(SC.rigs())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.mark.parametrize("name", RIGS)
def test_restatement_equals_the_reference(name):
    g, joints = SC.load_fixture(name)
    ex = E.expected(g["pos"], g["nrm"], g["idx"], joints, list(g["posed"]))
    assert np.array_equal(ex["off"], g["off"]) and np.array_equal(ex["jidx"], g["jidx"])
    assert len(g["jidx"]) > 0 and np.diff(g["off"]).max() >= 3              # lists long enough for the order of the sums to show
    for k, (p, n) in enumerate(ex["frames"]):
        assert not np.isnan(g["smooth_pos"][k]).any()
        assert np.array_equal(bits(p), bits(g["smooth_pos"][k])) and np.array_equal(bits(p), bits(g["flat_pos"][k])), (name, k)
        assert np.array_equal(bits(g["smooth_nrm"][k]), bits(g["nrm"])), (name, k)         # skin leaves the normals alone
        assert np.array_equal(bits(n), bits(g["flat_nrm"][k])), (name, k)
        assert not np.array_equal(bits(p), bits(g["pos"]))


def test_restatement_matrix_routines():
    """mat4_mul takes the operands the way Mat4::operator* does (a * b applies b first), and the inverse undoes a translation exactly."""
    t = SC._data(SC._translate([1, 2, 3]))
    s = SC._data(np.diag([2.0, 4.0, 8.0, 1.0]))
    p = np.array([[1, 1, 1]], np.float32)
    assert np.array_equal(E.mat_point(E.mat4_mul(t, s), p), [[3, 6, 11]])       # scale, then translate
    assert np.array_equal(E.mat_point(E.mat4_mul(s, t), p), [[4, 12, 32]])
    assert np.array_equal(E.mat_point(E.mat4_inverse(t), p), [[0, -1, -2]])


def fixture_blob(name, path):
    g, joints = SC.load_fixture(name)
    nv, nj = len(g["pos"]), len(joints)
    with open(path, "wb") as f:
        f.write(np.array([nv, len(g["idx"]), nj, len(g["posed"])], np.uint32).tobytes())
        for a in (g["pos"], g["nrm"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
        f.write(np.ascontiguousarray(g["idx"], np.uint32).tobytes())
        f.write(np.concatenate([g["bind"].reshape(nj, 16), g["extent"].reshape(nj, 3), g["radius"].reshape(nj, 1)], axis=1).astype(np.float32).tobytes())
        f.write(np.ascontiguousarray(g["off"], np.uint32).tobytes())
        f.write(np.ascontiguousarray(g["jidx"], np.uint32).tobytes())
        for k in range(len(g["posed"])):
            for a in (g["posed"][k], g["smooth_pos"][k], g["flat_nrm"][k]):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_device_functions_on_the_host(tmp_path, sanitized):
    """tests/host_emu/skin_host.cpp over both fixtures: the map, the positions and the flat normals, bit for bit."""
    for name in RIGS:
        blob = str(tmp_path / f"{name}.bin")
        fixture_blob(name, blob)
        H.run_sanitized_main(tmp_path, "skin_host.cpp", scene_layer=False, args=[blob], flags=H.SANITIZE if sanitized else ("-O2",))


def test_abi_and_validation_on_a_host_only_context(srt):
    lib = srt.load_library()
    names = ("create", "destroy", "counts", "map", "vertices_device", "vertices", "pose")
    assert all(hasattr(lib, "srt_pt_skin_" + n) for n in names)
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for decl in ("int srt_pt_skin_create(srt_pt* pt, uint32_t object, const float* bind_positions, const float* bind_normals, uint32_t nverts,",
                 "int srt_pt_skin_map(srt_pt_skin* skin, uint32_t* offsets, uint32_t* joints, float* weights, uint32_t cap);",
                 "int srt_pt_skin_vertices_device(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals, float* d_positions_out, float* d_normals_out);",
                 "int srt_pt_skin_pose(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);", "int srt_pt_skin_destroy(srt_pt_skin* skin);"):
        assert decl in header, decl
    assert srt.SKIN_JOINT_DTYPE.itemsize == 80 and E.JOINT_DTYPE == srt.SKIN_JOINT_DTYPE        # srt_pt_skin_joint: 16 + 3 + 1 floats
    for cls, methods in ((srt.Pathtracer, ("create_skin",)), (srt.PathtracerGroup, ("create_skin",)), (srt.Skin, ("map", "vertices", "pose", "close")),
                         (srt.SkinGroup, ("pose", "close"))):
        assert all(callable(getattr(cls, m, None)) for m in methods)

    S = refusal_scene(UC.IC.scenes_module())           # 0-4 walls, 5 sphere, 6 blob, 7 area light, 8 instance of 6, 9 emissive sphere
    p, n = UC.original(S, 6)
    lp, ln = UC.original(S, 7)
    joints, poses = SC.blob_chain()
    J = srt.skin_joints(joints)
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    h = ctypes.c_void_p()

    def create(ctx, index, pos, nrm, nverts, jp, nj, out=h):
        return lib.srt_pt_skin_create(ctx, index, H.P(pos) if pos is not None else None, H.P(nrm) if nrm is not None else None, nverts,
                                      H.P(jp) if jp is not None else None, nj, ctypes.byref(out) if out is not None else None)

    assert create(pt._ctx, 6, p, n, len(p), J, len(J)) == STATE                       # before commit
    pt.build_scene(S)
    assert create(None, 6, p, n, len(p), J, len(J)) == INVALID
    assert create(pt._ctx, 6, None, n, len(p), J, len(J)) == INVALID and create(pt._ctx, 6, p, None, len(p), J, len(J)) == INVALID
    assert create(pt._ctx, 6, p, n, len(p), None, len(J)) == INVALID and create(pt._ctx, 6, p, n, len(p), J, len(J), out=None) == INVALID
    for what, index, pp, nn, nverts in (("out of range", len(S["objects"]), p, n, len(p)), ("a sphere", 5, p, n, len(p)), ("a sphere light", 9, lp, ln, len(lp)),
                                        ("an instance", 8, p, n, len(p)), ("an area light", 7, lp, ln, len(lp)), ("another vertex count", 6, p[:-3], n[:-3], len(p) - 3),
                                        ("a vertex too many", 6, p, n, len(p) + 1)):
        assert create(pt._ctx, index, pp, nn, nverts, J, len(J)) == INVALID, what
        assert not h.value
    assert create(pt._ctx, 8, p, n, len(p), J, len(J)) == INVALID and "object 6" in lib.srt_last_error().decode()     # names the instance's source
    assert create(pt._ctx, 6, p, n, len(p), J, 0) == INVALID
    many = np.zeros(4097, srt.SKIN_JOINT_DTYPE)
    assert create(pt._ctx, 6, p, n, len(p), many, len(many)) == UNSUPPORTED               # the limit of the header
    assert create(pt._ctx, 6, p, n, len(p), J, len(J)) == UNSUPPORTED and not h.value      # valid arguments: host-only has no skinning
    with pytest.raises(srt.SrtError, match="host-only") as e:
        pt.create_skin(6, p, n, joints)
    assert e.value.status == UNSUPPORTED
    # a NULL skin is refused by every call that needs one; destroy takes it
    posed = np.ascontiguousarray(poses[0], np.float32)
    off, ji, w, out = np.zeros(len(p) + 1, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.float32), np.zeros((len(p), 3), np.float32)
    assert lib.srt_pt_skin_map(None, H.P(off), H.P(ji), H.P(w), 4) == INVALID
    assert lib.srt_pt_skin_counts(None, H.P(ji)) == INVALID
    assert lib.srt_pt_skin_vertices(None, H.P(posed), 0, H.P(out), H.P(out)) == INVALID
    assert lib.srt_pt_skin_vertices_device(None, None, H.P(posed), 0, H.P(out), H.P(out)) == INVALID
    assert lib.srt_pt_skin_pose(None, None, H.P(posed), 0) == INVALID
    assert lib.srt_pt_skin_destroy(None) == 0
    pt.close()
