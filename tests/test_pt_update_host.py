"""CPU: srt_pt_update_mesh on the host side.  The scene layer's prepare_mesh_update / apply_mesh_update (through
tests/host_emu/update_host.cpp) against a fresh build_scene of scenes.with_vertices(S, ..) - bit-equal in everything a kernel
computes from; refusals that leave the scene byte for byte as it was; the per-triangle device functions (pt_mesh_update.h)
compiled for the host against triangle_box / append_triangles; a sanitized stand-alone program; and the ABI."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _update_cases as UC

INVALID, UNSUPPORTED, STATE = -1, -4, -5          # SRT_ERR_* (include/srt_raster.h)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def blob_slot(dumps, index):
    return [k for k in range(len(dumps) - 1) if dumps[0][2][k] == index + 1][0]


def test_deformations_exercise_both_storage_paths(scenes):
    """The oracle's BVH<Triangle> of cornell_with_mesh(3) object 6 under D1..D3: at least one deformation changes the node count
    (ranges behind the mesh are re-packed) and at least one keeps it (the mesh's ranges are rewritten in place)."""
    S = UC.blob_scene()
    counts = {}
    for name, arrays in [("original", UC.original(S, UC.BLOB_OBJECT))] + list(UC.deformations().items()):
        o = H.OraclePT(scenes.with_vertices(S, UC.BLOB_OBJECT, *arrays), 8, 8, 4, True)
        dumps = IC.all_dumps(o, len(S["objects"]))
        counts[name] = len(dumps[1 + blob_slot(dumps, UC.BLOB_OBJECT)][0])
    assert counts == UC.NODES
    assert any(counts[d] != counts["original"] for d in ("D1", "D2", "D3")) and any(counts[d] == counts["original"] for d in ("D1", "D2", "D3"))


def scene_cases():
    return {"blob": (UC.blob_scene, UC.BLOB_OBJECT, 3), "sweeps": (IC.sweeps_scene, 6, 3), "two_meshes": (UC.two_mesh_scene, UC.BLOB_OBJECT, 3)}


@pytest.mark.parametrize("which", ["blob", "sweeps", "two_meshes"])
@pytest.mark.parametrize("use_bvh", [True, False])
def test_update_equals_fresh_build(scenes, which, use_bvh):
    """D1, D2, D3 in turn on one scene, each against a fresh build of the same description; then back to the original arrays."""
    make, index, subdiv = scene_cases()[which]
    S = make()
    first = UC.HostScene(S, use_bvh)
    hs = first.clone()
    for name, (p, n) in UC.deformations(subdiv).items():
        assert hs.update(index, p, n) == 0, hs.error()
        fresh = UC.HostScene(scenes.with_vertices(S, index, p, n), use_bvh)
        assert hs.same_computed(fresh), (which, use_bvh, name)
        if use_bvh and which != "two_meshes":
            assert hs.store(index)["nodes"] == UC.NODES[name]
        for k, o in enumerate(S["objects"]):
            if o["kind"] == "instance" and o["of"] == index:       # the instance follows: the source's new root box and ranges
                assert np.array_equal(hs.local_box(k).view(np.uint32), hs.local_box(index).view(np.uint32)) and hs.store(k) == hs.store(index)
        fresh.close()
    assert hs.update(index, *UC.original(S, index)) == 0
    assert hs.same_computed(first)
    hs.close(); first.close()


@pytest.mark.parametrize("use_bvh", [True, False])
def test_two_meshes_in_both_storage_orders(scenes, use_bvh):
    """Each of two meshes updated in turn: the updated range lies once in front of and once behind the other one, whose stored
    nodes, records and triangles keep their content."""
    S = UC.two_mesh_scene()
    hs = UC.HostScene(S, use_bvh)
    if use_bvh:
        assert hs.store(6)["node_off"] != hs.store(8)["node_off"]
    p6, n6 = UC.deformations()["D1"]
    p8, n8 = UC.small_blob_deformation()
    assert hs.update(6, p6, n6) == 0
    S1 = scenes.with_vertices(S, 6, p6, n6)
    f1 = UC.HostScene(S1, use_bvh)
    assert hs.same_computed(f1)
    assert hs.update(8, p8, n8) == 0
    S2 = scenes.with_vertices(S1, 8, p8, n8)
    f2 = UC.HostScene(S2, use_bvh)
    assert hs.same_computed(f2) and not hs.same_computed(f1)
    for x in (hs, f1, f2):
        x.close()


@pytest.mark.parametrize("use_bvh", [True, False])
def test_particle_scene_source(scenes, use_bvh):
    """Object 8 of the shared particle scene (32 triangles) is the source of 59 instances: 60 object boxes move."""
    S = IC.particles_shared()[0]
    src = IC.PARTICLE_FIRST
    p, n = UC.original(S, src)
    p2 = (p * np.array([1.4, 0.7, 1.1], np.float32) + np.array([0.01, 0.0, -0.02], np.float32)).astype(np.float32)
    first = UC.HostScene(S, use_bvh)
    hs = first.clone()
    boxes = [hs.local_box(k).copy() for k in range(src, src + IC.PARTICLE_COUNT)]
    assert hs.update(src, p2, n) == 0
    fresh = UC.HostScene(scenes.with_vertices(S, src, p2, n), use_bvh)
    assert hs.same_computed(fresh)
    assert all(not np.array_equal(hs.local_box(src + k), boxes[k]) for k in range(IC.PARTICLE_COUNT))
    # update, repose of the same objects, update back, repose back: the original scene
    idx, Ts = IC.repose_case(S)
    assert hs.repose(idx, Ts) == 0
    moved = UC.HostScene(IC.with_poses(scenes.with_vertices(S, src, p2, n), idx, Ts), use_bvh)
    assert hs.same_computed(moved)
    assert hs.update(src, p, n) == 0
    assert hs.repose(idx, np.array([S["objects"][i]["T"] for i in idx], np.float32)) == 0
    assert hs.same_computed(first)
    for x in (first, hs, fresh, moved):
        x.close()


def test_update_repose_update_sweeps(scenes):
    S = IC.sweeps_scene()
    n_obj = len(S["objects"])
    p, n = UC.deformations()["D2"]
    T = IC.translate(S["objects"][n_obj - 1]["T"], (0.5, -0.25, 0.3))
    first = UC.HostScene(S)
    hs = first.clone()
    assert hs.update(6, p, n) == 0 and hs.repose([n_obj - 1], [T]) == 0
    want = UC.HostScene(IC.with_poses(scenes.with_vertices(S, 6, p, n), [n_obj - 1], [T]))
    assert hs.same_computed(want)
    assert hs.update(6, *UC.original(S, 6)) == 0 and hs.repose([n_obj - 1], [S["objects"][n_obj - 1]["T"]]) == 0
    assert hs.same_computed(first)
    for x in (first, hs, want):
        x.close()


def refusal_scene(scenes):
    """Objects: 0-4 walls, 5 sphere, 6 blob, 7 area light, 8 instance of 6, 9 emissive sphere."""
    S = IC.sweeps_scene()
    light = S["objects"][7]
    S["objects"].append({"kind": "sphere", "radius": 0.05, "T": IC.translate(np.eye(4, dtype=np.float32).reshape(16), (0.3, 0.8, 0.3)), "material": 7,
                         "light_mesh": {"pos": light["pos"], "nrm": light["nrm"], "idx": light["idx"]}})
    return S


def refused_arguments(S):
    p, n = UC.deformations()["D1"]
    lp, ln = UC.original(S, 7)
    return [("out of range", len(S["objects"]), p, n, None), ("a sphere", 5, p, n, None), ("a sphere light", 9, lp, ln, None),
            ("an instance", 8, p, n, None), ("an area light", 7, lp, ln, None), ("another vertex count", 6, p[:-3], n[:-3], None),
            ("a vertex too many", 6, p, n, len(p) + 1)]


@pytest.mark.parametrize("use_bvh", [True, False])
def test_scene_layer_refusals_leave_the_scene_identical(scenes, use_bvh):
    S = refusal_scene(scenes)
    hs = UC.HostScene(S, use_bvh)
    before = hs.clone()
    for what, index, p, n, nverts in refused_arguments(S):
        assert hs.update(index, p, n, nverts) == 1, what
        assert hs.identical(before), what
    assert hs.update(8, *UC.deformations()["D1"]) == 1 and "object 6" in hs.error()        # the message names the instance's source
    if use_bvh:
        assert hs.update(6, *UC.one_point(S, 6)) == 2 and "does not terminate" in hs.error()
        assert hs.identical(before)
    hs.close(); before.close()


def test_deep_chain_is_refused(scenes):
    """A deformation onto deep_over's chain (BVH<Triangle> nesting 49 > 48): unsupported, the scene stays."""
    S, (cp, cn) = UC.flat_chain_scene()
    hs = UC.HostScene(S)
    before = hs.clone()
    assert hs.depths()[1] < 48
    assert hs.update(6, cp, cn) == 2 and hs.identical(before)
    hs.close(); before.close()


def host_pt(srt, scene, use_bvh=True):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, use_bvh)
    pt.build_scene(scene)
    return pt


def test_abi_update_on_a_host_only_context(srt, scenes):
    """The two symbols with the documented signatures, the Python methods, and srt_pt_update_mesh end to end on a host-only
    context: dumps and counts against a fresh commit and the oracle, every refusal's status, the scene left as it was."""
    lib = srt.load_library()
    assert hasattr(lib, "srt_pt_update_mesh") and hasattr(lib, "srt_pt_update_mesh_device")
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    assert "int srt_pt_update_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);" in header
    assert ("int srt_pt_update_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, "
            "uint32_t nverts);") in header
    assert lib.srt_pt_update_mesh.argtypes == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    for cls, names in ((srt.Pathtracer, ("update_mesh", "update_mesh_device")), (srt.PathtracerGroup, ("update_mesh",))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    S = refusal_scene(scenes)
    nobj = len(S["objects"])
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    p, n = UC.deformations()["D1"]
    assert lib.srt_pt_update_mesh(pt._ctx, 6, H.P(p), H.P(n), len(p)) == STATE        # before commit
    pt.build_scene(S)
    first = IC.all_dumps(pt, nobj)
    counts = pt.scene_counts()
    assert lib.srt_pt_update_mesh(None, 6, H.P(p), H.P(n), len(p)) == INVALID
    assert lib.srt_pt_update_mesh(pt._ctx, 6, None, H.P(n), len(p)) == INVALID and lib.srt_pt_update_mesh(pt._ctx, 6, H.P(p), None, len(p)) == INVALID
    for what, index, pp, nn, nverts in refused_arguments(S):
        pp, nn = np.ascontiguousarray(pp, np.float32), np.ascontiguousarray(nn, np.float32)
        assert lib.srt_pt_update_mesh(pt._ctx, index, H.P(pp), H.P(nn), len(pp) if nverts is None else nverts) == INVALID, what
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts, what
    with pytest.raises(srt.SrtError, match="object 6"):
        pt.update_mesh(8, p, n)
    with pytest.raises(srt.SrtError, match="does not terminate") as e:
        pt.update_mesh(6, *UC.one_point(S, 6))
    assert e.value.status == UNSUPPORTED and IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts
    # the update itself: the trees of a fresh commit and of the oracle, one more build, the same storage totals where the node count is kept
    for name in ("D1", "D3"):
        p, n = UC.deformations()[name]
        pt.update_mesh(6, p, n)
        desc = scenes.with_vertices(S, 6, p, n)
        fresh = host_pt(srt, desc)
        got = IC.all_dumps(pt, nobj)
        assert IC.dumps_equal(got, IC.all_dumps(fresh, nobj)) and not IC.dumps_equal(got, first)
        assert IC.dumps_equal(got, IC.all_dumps(H.OraclePT(IC.expand(desc), 8, 8, 8, True), nobj))       # (the oracle knows no instances)
        after, want = pt.scene_counts(), fresh.scene_counts()
        assert {k: v for k, v in after.items() if k != "blas_builds"} == {k: v for k, v in want.items() if k != "blas_builds"}
        fresh.close()
    assert pt.scene_counts()["blas_builds"] == counts["blas_builds"] + 2
    pt.update_mesh(6, *UC.original(S, 6))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first)
    # the deep chain through the ABI
    S2, (cp, cn) = UC.flat_chain_scene()
    pt.build_scene(S2)
    before = IC.all_dumps(pt, 8)
    with pytest.raises(srt.SrtError, match="too deep") as e:
        pt.update_mesh(6, cp, cn)
    assert e.value.status == UNSUPPORTED and IC.dumps_equal(IC.all_dumps(pt, 8), before)
    # list mode: nothing is built
    lst = host_pt(srt, S, use_bvh=False)
    c0 = lst.scene_counts()
    lst.update_mesh(6, p, n)
    assert lst.scene_counts() == c0 and c0["blas_builds"] == 0
    lst.close()
    pt.close()


def test_with_vertices(scenes):
    S = IC.sweeps_scene()
    p, n = UC.deformations()["D1"]
    out = scenes.with_vertices(S, 6, p, n)
    assert out is not S and out["objects"][6] is not S["objects"][6] and np.array_equal(out["objects"][6]["pos"], p)
    assert np.array_equal(S["objects"][6]["pos"], UC.original(S, 6)[0])                # the input is not modified
    assert all(a is b for k, (a, b) in enumerate(zip(out["objects"], S["objects"])) if k != 6)
    assert out["objects"][6]["idx"] is S["objects"][6]["idx"] and out["objects"][8]["of"] == 6
    for bad in (lambda: scenes.with_vertices(S, 5, p, n), lambda: scenes.with_vertices(S, 8, p, n), lambda: scenes.with_vertices(S, 6, p[:-1], n[:-1])):
        with pytest.raises(ValueError):
            bad()


def test_device_functions_on_the_host():
    """mesh_triangle_box / mesh_triangle_record over every triangle of D1, in index order and in a BVH's primitive order, and over
    triangles with zero and negative-zero coordinates (the sign of a zero bound is part of the device builder's contract)."""
    lib = UC.update_lib()
    p, n = UC.deformations()["D1"]
    idx = np.arange(len(p), dtype=np.uint32)
    ntri = len(idx) // 3
    zeros = np.zeros(2, np.uint32)
    assert lib.upd_emu_mismatches(H.P(p), H.P(n), len(p), H.P(idx), ntri, None, H.P(zeros)) == 0
    order = np.random.default_rng(3).permutation(ntri).astype(np.uint32)
    assert lib.upd_emu_mismatches(H.P(p), H.P(n), len(p), H.P(idx), ntri, H.P(order), H.P(zeros)) == 0
    # signed zeros: every combination of +0 / -0 / a value on the three corners of an axis, degenerate (zero-extent) axes included
    vals = np.array([0.0, -0.0, 0.25, -0.25], np.float32)
    tri = np.array([[a, b, c] for a in vals for b in vals for c in vals], np.float32)            # 64 triangles' x coordinates
    zp = np.stack([tri, tri[:, ::-1], np.roll(tri, 1, axis=1)], axis=2).reshape(-1, 3).astype(np.float32)    # the other axes: permutations
    zn = np.tile(np.array([0.0, -0.0, 1.0], np.float32), (len(zp), 1))
    zi = np.arange(len(zp), dtype=np.uint32)
    assert lib.upd_emu_mismatches(H.P(zp), H.P(zn), len(zp), H.P(zi), len(zi) // 3, None, H.P(zeros)) == 0
    assert zeros[0] > 0 and zeros[1] > 0            # bounds of both signs of zero occur


def test_sanitized_update_repose_update(tmp_path):
    """tests/host_emu/update_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: update, repose, update, a refused
    update - built with AddressSanitizer and UndefinedBehaviorSanitizer and run once on the CPU."""
    H.run_sanitized_main(tmp_path, "update_sanitized_main.cpp")
