"""CPU: srt_pt_refit_mesh / srt_pt_mesh_tree_cost on a host-only context (device = -1), where the scene layer's refit_boxes /
prepare_mesh_refit / apply_mesh_refit (pt_scene.cpp) do all the work - the definition the device kernels are held to.  A refit
keeps links and primitive order and gives every node the exact min / max fold of its triangles' boxes, which a numpy restatement
checks with ==; refusals leave every dump and count as they were; and a sanitized stand-alone program runs the same layer."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _refit_cases as RC
import _update_cases as UC
from _cases import pt_scene

INVALID, UNSUPPORTED, STATE = -1, -4, -5          # SRT_ERR_* (include/srt_raster.h)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def host_pt(srt, scene, use_bvh=True):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, use_bvh)
    pt.build_scene(scene)
    return pt


def mesh_dump(pt, index, nobj):
    return pt.dump_bvh(RC.slot_of(pt, index, nobj))


def check_refitted(pt, S, index, before, p, n):
    """Links and order as before, boxes == the numpy restatement from the new vertices."""
    nobj = len(S["objects"])
    boxes, links, order = mesh_dump(pt, index, nobj)
    idx = np.ascontiguousarray(S["objects"][index]["idx"], np.uint32)
    assert np.array_equal(idx, np.arange(len(idx), dtype=np.uint32))       # flat-shaded: dump_bvh's order is 3 * triangle
    ntri = len(idx) // 3
    assert np.array_equal(links, before[1]) and np.array_equal(order[:ntri], before[2][:ntri])
    want = RC.refit_boxes_numpy(links, order[:ntri] // 3, p, idx)
    assert RC.bits_equal(boxes, want)
    assert np.all(boxes == want)
    return boxes, links


def test_abi(srt):
    lib = srt.load_library()
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for decl in ("int srt_pt_refit_mesh(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);",
                 "int srt_pt_refit_mesh_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts);",
                 "int srt_pt_skin_pose_refit(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);",
                 "int srt_pt_mesh_tree_cost(srt_pt* pt, uint32_t object, double* cost);"):
        assert decl in header
    for name in ("srt_pt_refit_mesh", "srt_pt_refit_mesh_device", "srt_pt_skin_pose_refit", "srt_pt_mesh_tree_cost", "srt_pt_refit_count"):
        assert hasattr(lib, name)
    for cls, names in ((srt.Pathtracer, ("refit_mesh", "refit_mesh_device", "mesh_tree_cost")), (srt.PathtracerGroup, ("refit_mesh",))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    from soft_rendering_toolsets_amd import _pt_bindings as B

    assert callable(B.Skin.pose_refit) and callable(B.SkinGroup.pose_refit)


def test_identity_refit(srt):
    S = UC.blob_scene()
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    first, counts, cost = IC.all_dumps(pt, nobj), pt.scene_counts(), pt.mesh_tree_cost(UC.BLOB_OBJECT)
    pt.refit_mesh(UC.BLOB_OBJECT, *UC.original(S, UC.BLOB_OBJECT))
    after = pt.scene_counts()
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first)
    assert after["refits"] == counts["refits"] + 1 == 1
    assert {k: v for k, v in after.items() if k != "refits"} == {k: v for k, v in counts.items() if k != "refits"}
    assert pt.mesh_tree_cost(UC.BLOB_OBJECT) == cost
    pt.close()


@pytest.mark.parametrize("which", ["blob", "two_meshes", "sweeps"])
def test_refit_to_each_deformation(srt, scenes, which):
    """D1, D2, D3 in turn on one context (sweeps: the scene with an instance of the blob, which follows)."""
    S = {"blob": UC.blob_scene, "two_meshes": UC.two_mesh_scene, "sweeps": IC.sweeps_scene}[which]()
    nobj, index = len(S["objects"]), UC.BLOB_OBJECT
    pt = host_pt(srt, S)
    before = mesh_dump(pt, index, nobj)
    others = {k: mesh_dump(pt, k, nobj) for k, o in enumerate(S["objects"]) if o["kind"] == "mesh" and k != index}
    builds = pt.scene_counts()["blas_builds"]
    for name, (p, n) in UC.deformations().items():
        pt.refit_mesh(index, p, n)
        boxes, _ = check_refitted(pt, S, index, before, p, n)
        fresh = host_pt(srt, scenes.with_vertices(S, index, p, n))
        # the BVH<Object> - boxes, links, object order - is the fresh commit's: the root box is the same fold over all triangles
        assert IC.dumps_equal([pt.dump_bvh(-1)], [fresh.dump_bvh(-1)]), name
        assert RC.bits_equal(boxes[0], mesh_dump(fresh, index, nobj)[0][0])
        for k, o in enumerate(S["objects"]):
            if o["kind"] == "instance" and o["of"] == index:       # the instance dumps the source's refitted tree
                assert IC.dumps_equal([mesh_dump(pt, k, nobj)], [mesh_dump(pt, index, nobj)])
        for k, d in others.items():                                 # no other mesh's tree is touched
            assert IC.dumps_equal([mesh_dump(pt, k, nobj)], [d]), (name, k)
        fresh.close()
    assert pt.scene_counts()["blas_builds"] == builds and pt.scene_counts()["refits"] == 3
    pt.close()


def test_second_mesh_of_two(srt, scenes):
    S = UC.two_mesh_scene()
    pt = host_pt(srt, S)
    before6, before8 = mesh_dump(pt, 6, 9), mesh_dump(pt, 8, 9)
    p, n = UC.small_blob_deformation()
    pt.refit_mesh(8, p, n)
    check_refitted(pt, S, 8, before8, p, n)
    assert IC.dumps_equal([mesh_dump(pt, 6, 9)], [before6])
    pt.close()


def test_degenerate_shapes(srt):
    # the shallow 53-triangle tree takes the chain's vertices (an update would build a tree nesting 49 and be refused)
    S, (cp, cn) = UC.flat_chain_scene()
    pt = host_pt(srt, S)
    before = mesh_dump(pt, 6, 8)
    pt.refit_mesh(6, cp, cn)
    check_refitted(pt, S, 6, before, cp, cn)
    # flat boxes: every vertex in one plane - Triangle::bbox widens the flat axis by +1.0f, and so does every node
    fp = UC.original(S, 6)[0].copy()
    fp[:, 2] = np.float32(0.25)
    pt.refit_mesh(6, fp, cn)
    boxes, _ = check_refitted(pt, S, 6, before, fp, cn)
    assert np.all(boxes[:, 2] == np.float32(0.25)) and np.all(boxes[:, 5] == np.float32(1.25))
    pt.close()
    # the deep skewed tree (48 nested interior nodes = kMaxBlasDepth)
    D = pt_scene("deep_max")
    pt = host_pt(srt, D)
    before = mesh_dump(pt, 6, len(D["objects"]))
    p, n = UC.original(D, 6)
    moved = (p + (np.random.default_rng(5).random(p.shape, dtype=np.float32) - np.float32(0.5)) * np.float32(1e-3)).astype(np.float32)
    pt.refit_mesh(6, moved, n)
    check_refitted(pt, D, 6, before, moved, n)
    pt.close()
    # a mesh of <= 4 triangles: the root is a leaf, there are no records
    P = IC.scenes_module().cornell_with_mesh(3, "glass")
    small = dict(P["objects"][6])
    small.update(pos=np.ascontiguousarray(small["pos"][:9]), nrm=np.ascontiguousarray(small["nrm"][:9]), idx=np.arange(9, dtype=np.uint32))
    P["objects"][6] = small
    pt = host_pt(srt, P)
    before = mesh_dump(pt, 6, 8)
    assert len(before[0]) == 1 and before[1][0][2] == before[1][0][3]
    counts = pt.scene_counts()
    p = (small["pos"] * np.float32(1.25)).astype(np.float32)
    pt.refit_mesh(6, p, small["nrm"])
    check_refitted(pt, P, 6, before, p, small["nrm"])
    assert pt.scene_counts()["blas_records"] == counts["blas_records"] and pt.mesh_tree_cost(6) == 3.0
    pt.close()


def test_refit_then_update_equals_a_fresh_commit(srt, scenes):
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    (p1, n1), (p2, n2) = UC.deformations()["D1"], UC.deformations()["D2"]
    pt.refit_mesh(6, p1, n1)
    pt.update_mesh(6, p2, n2)
    fresh = host_pt(srt, scenes.with_vertices(S, 6, p2, n2))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj))
    # and an update with the refitted vertices equals a fresh commit of those
    pt.refit_mesh(6, p1, n1)
    pt.update_mesh(6, p1, n1)
    fresh1 = host_pt(srt, scenes.with_vertices(S, 6, p1, n1))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh1, nobj))
    for x in (pt, fresh, fresh1):
        x.close()


def test_every_refusal_leaves_the_scene_alone(srt, scenes):
    lib = srt.load_library()
    S = RC.refusal_scene()
    nobj = len(S["objects"])
    p, n = UC.deformations()["D1"]
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    cost = ctypes.c_double()
    assert lib.srt_pt_refit_mesh(pt._ctx, 6, H.P(p), H.P(n), len(p)) == STATE        # before commit
    assert lib.srt_pt_mesh_tree_cost(pt._ctx, 6, ctypes.byref(cost)) == STATE
    pt.build_scene(S)
    first, counts = IC.all_dumps(pt, nobj), pt.scene_counts()

    def unchanged(what):
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts, what

    assert lib.srt_pt_refit_mesh(None, 6, H.P(p), H.P(n), len(p)) == INVALID
    assert lib.srt_pt_refit_mesh(pt._ctx, 6, None, H.P(n), len(p)) == INVALID and lib.srt_pt_refit_mesh(pt._ctx, 6, H.P(p), None, len(p)) == INVALID
    assert lib.srt_pt_mesh_tree_cost(pt._ctx, 6, None) == INVALID
    for what, index, pp, nn, nverts in RC.refused_arguments(S):
        pp, nn = np.ascontiguousarray(pp, np.float32), np.ascontiguousarray(nn, np.float32)
        assert lib.srt_pt_refit_mesh(pt._ctx, index, H.P(pp), H.P(nn), len(pp) if nverts is None else nverts) == INVALID, what
        unchanged(what)
    for what, index in (("out of range", nobj), ("a sphere", 5), ("a sphere light", 9), ("an instance", 8), ("an area light", 7)):
        assert lib.srt_pt_mesh_tree_cost(pt._ctx, index, ctypes.byref(cost)) == INVALID, what
    with pytest.raises(srt.SrtError, match="object 6"):                               # the message names the instance's source
        pt.refit_mesh(8, p, n)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[len(q) // 2, 1] = bad
        with pytest.raises(srt.SrtError, match="non-finite") as e:
            pt.refit_mesh(6, q, n)
        assert e.value.status == INVALID
        unchanged(bad)
    # all vertices at one point: the update's BVH<Triangle> build does not terminate, the refit builds nothing and goes through
    with pytest.raises(srt.SrtError, match="does not terminate"):
        pt.update_mesh(6, *UC.one_point(S, 6))
    unchanged("update to one point")
    pt.refit_mesh(6, *UC.one_point(S, 6))
    assert pt.scene_counts()["refits"] == counts["refits"] + 1 and pt.scene_counts()["blas_builds"] == counts["blas_builds"]
    pt.close()
    # list mode: no tree - the call does what update_mesh does, and there is no cost
    lst = host_pt(srt, S, use_bvh=False)
    c0 = lst.scene_counts()
    lst.refit_mesh(6, p, n)
    upd = host_pt(srt, S, use_bvh=False)
    upd.update_mesh(6, p, n)
    assert lst.scene_counts() == c0 == upd.scene_counts()
    with pytest.raises(srt.SrtError) as e:
        lst.mesh_tree_cost(6)
    assert e.value.status == UNSUPPORTED
    lst.close(); upd.close()


def test_top_build_failure_is_unsupported_and_changes_nothing(srt, scenes):
    """New vertices that give the blob (posed by the identity here) exactly the sphere's box: two objects with one centre, which no
    plane parts - the reference's BVH<Object> build loops forever.  Unsupported, and refused before anything is written."""
    S = UC.blob_scene()
    S["objects"][6] = dict(S["objects"][6], T=np.eye(4, dtype=np.float32).reshape(16))
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    first, counts = IC.all_dumps(pt, nobj), pt.scene_counts()
    tl = first[0]
    k = RC.slot_of(tl, 5, nobj)
    leaf = [i for i in range(len(tl[1])) if tl[1][i][2] == tl[1][i][3] and tl[1][i][0] == k and tl[1][i][1] == 1][0]
    lo, hi = tl[0][leaf][:3], tl[0][leaf][3:]
    p, n = UC.original(S, 6)
    plo, phi = p.min(axis=0), p.max(axis=0)
    q = ((p - plo) / (phi - plo) * (hi - lo) * np.float32(0.5) + lo + (hi - lo) * np.float32(0.25)).astype(np.float32)   # well inside ..
    q[0], q[1] = lo, hi                                                                                                   # .. but for two corners
    with pytest.raises(srt.SrtError, match="BVH<Object> build does not terminate") as e:
        pt.refit_mesh(6, q, n)
    assert e.value.status == UNSUPPORTED
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts
    pt.close()


def test_mesh_tree_cost(srt, scenes):
    S = UC.two_mesh_scene()
    pt = host_pt(srt, S)
    for index in (6, 8):
        boxes, links, _ = mesh_dump(pt, index, 9)
        got, want = pt.mesh_tree_cost(index), RC.tree_cost_numpy(boxes, links)
        assert abs(got - want) <= 1e-9 * want, (index, got, want)
    # the tangled blob: the step from the committed vertices to small_blob_deformation() taken TANGLE times over.  Chosen on the CPU
    # with the host code: refitted / rebuilt cost is 17.02 / 16.08 at 1, 16.39 / 14.65 at 1.5, 16.06 / 13.76 at 2, 16.58 / 13.74 at 3.
    TANGLE = 3.0
    p0, _ = UC.original(S, 8)
    p, n = UC.small_blob_deformation()
    tangled = (p0 + (p - p0) * np.float32(TANGLE)).astype(np.float32)
    pt.refit_mesh(8, tangled, n)
    boxes, links, _ = mesh_dump(pt, 8, 9)
    refitted = pt.mesh_tree_cost(8)
    assert abs(refitted - RC.tree_cost_numpy(boxes, links)) <= 1e-9 * refitted
    pt.update_mesh(8, tangled, n)
    rebuilt = pt.mesh_tree_cost(8)
    print("tree cost of the tangled blob: refitted", refitted, "rebuilt", rebuilt)
    assert refitted > rebuilt
    pt.close()


def test_sanitized_refit(tmp_path):
    """tests/host_emu/refit_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: refits, a repose, an update, the
    refusals - built with AddressSanitizer and UndefinedBehaviorSanitizer and run once on the CPU."""
    H.run_sanitized_main(tmp_path, "refit_sanitized_main.cpp")
