"""CPU: srt_pt_refit_mesh_inplace on a host-only context (device = -1), where the scene layer's prepare_mesh_refit_inplace /
apply_mesh_refit_inplace (pt_scene.cpp) do all the work - the definition the device forms are held to: new vertices for one mesh
with BOTH trees kept.  Links and orders of both trees stay, the mesh's boxes are the numpy restatement of the triangle fold, the
BVH<Object>'s the numpy restatement of the fold over the posed boxes; a rebuild of the BVH<Object> on top gives srt_pt_refit_mesh's
scene; refusals leave every dump and count as they were; the emulation's closest hits equal the oracle's on a fresh commit; and a
sanitized stand-alone program runs the same layer."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _refit_cases as RC
import _refit_inplace_cases as RI
import _repose_refit_cases as PR
import _update_cases as UC
from _cases import pt_scene, random_rays

INVALID, UNSUPPORTED, STATE = -1, -4, -5          # SRT_ERR_* (include/srt_raster.h)
SCENES = {"blob": UC.blob_scene, "two_meshes": UC.two_mesh_scene, "sweeps": IC.sweeps_scene}


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


def check_mesh(pt, S, index, before, p):
    """The mesh's tree: links and order as before, boxes == the numpy restatement from the new vertices."""
    nobj = len(S["objects"])
    boxes, links, order = mesh_dump(pt, index, nobj)
    idx = np.ascontiguousarray(S["objects"][index]["idx"], np.uint32)
    assert np.array_equal(idx, np.arange(len(idx), dtype=np.uint32))       # flat-shaded: dump_bvh's order is 3 * triangle
    ntri = len(idx) // 3
    assert np.array_equal(links, before[1]) and np.array_equal(order[:ntri], before[2][:ntri])
    want = RC.refit_boxes_numpy(links, order[:ntri] // 3, p, idx)
    assert np.all(boxes == want) and RC.bits_equal(boxes, want)
    return boxes


def check_top(pt, S, index, before_top, p, active=None):
    """The BVH<Object>: links and order as before, boxes == the numpy fold over the posed boxes."""
    boxes, links, order = pt.dump_bvh(-1)
    nobj = len(S["objects"])
    assert np.array_equal(links, before_top[1]) and np.array_equal(order[:nobj], before_top[2][:nobj])
    want = RI.expected_top_boxes(S, index, p, links, order, active)
    assert np.all(boxes == want) and RC.bits_equal(boxes, want)
    return boxes, links


def test_abi(srt):
    lib = srt.load_library()
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    debug = open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()
    for decl in ("int srt_pt_refit_mesh_inplace(srt_pt* pt, uint32_t object, const float* positions, const float* normals, uint32_t nverts);",
                 "int srt_pt_refit_mesh_inplace_device(srt_pt* pt, void* stream, uint32_t object, const float* d_positions, const float* d_normals, uint32_t nverts);",
                 "int srt_pt_skin_pose_inplace(srt_pt_skin* skin, void* stream, const float* posed, int flat_normals);",
                 "int srt_pt_skin_pose_inplace_at(srt_pt_skin* skin, void* stream, float t, int flat_normals);"):
        assert decl in header
    assert "int srt_pt_mesh_refit_pending(srt_pt* pt, uint64_t out[2]);" in debug
    for name in ("srt_pt_refit_mesh_inplace", "srt_pt_refit_mesh_inplace_device", "srt_pt_skin_pose_inplace", "srt_pt_skin_pose_inplace_at",
                 "srt_pt_mesh_refit_pending"):
        assert hasattr(lib, name)
    for cls, names in ((srt.Pathtracer, ("refit_mesh_inplace", "refit_mesh_inplace_device", "mesh_refit_pending")),
                       (srt.PathtracerGroup, ("refit_mesh_inplace", "refit_mesh_inplace_device"))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    from soft_rendering_toolsets_amd import _pt_bindings as B

    for cls in (B.Skin, B.SkinGroup):
        assert callable(cls.pose_inplace) and callable(cls.pose_inplace_at)


def test_identity_refit(srt):
    """The committed vertices give the committed boxes of both trees back, and nothing but the refit count moves."""
    S = UC.blob_scene()
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    first, counts = IC.all_dumps(pt, nobj), pt.scene_counts()
    costs = pt.mesh_tree_cost(UC.BLOB_OBJECT), pt.scene_tree_cost()
    pt.refit_mesh_inplace(UC.BLOB_OBJECT, *UC.original(S, UC.BLOB_OBJECT))
    after = pt.scene_counts()
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first)
    assert after["refits"] == counts["refits"] + 1 == 1
    assert {k: v for k, v in after.items() if k != "refits"} == {k: v for k, v in counts.items() if k != "refits"}
    assert (pt.mesh_tree_cost(UC.BLOB_OBJECT), pt.scene_tree_cost()) == costs and pt.mesh_refit_pending() == (0, 0)
    pt.close()


@pytest.mark.parametrize("which", sorted(SCENES))
def test_refit_to_each_deformation(srt, which):
    """D1, D2, D3 in turn on one context (sweeps: the scene with an instance of the blob, which follows): both trees keep links and
    orders, the boxes are the numpy folds, no other mesh is touched, nothing is built; the tree costs agree with numpy in double."""
    S = SCENES[which]()
    nobj, index = len(S["objects"]), UC.BLOB_OBJECT
    pt = host_pt(srt, S)
    before, before_top = mesh_dump(pt, index, nobj), pt.dump_bvh(-1)
    others = {k: mesh_dump(pt, k, nobj) for k, o in enumerate(S["objects"]) if o["kind"] == "mesh" and k != index}
    counts = pt.scene_counts()
    for name, (p, n) in UC.deformations().items():
        pt.refit_mesh_inplace(index, p, n)
        boxes = check_mesh(pt, S, index, before, p)
        top, links = check_top(pt, S, index, before_top, p)
        for k in RI.family_of(S, index)[1:]:                       # the instance dumps the source's refitted tree
            assert IC.dumps_equal([mesh_dump(pt, k, nobj)], [mesh_dump(pt, index, nobj)])
        for k, d in others.items():                                 # no other mesh's tree is touched
            assert IC.dumps_equal([mesh_dump(pt, k, nobj)], [d]), (name, k)
        for got, want in ((pt.mesh_tree_cost(index), RC.tree_cost_numpy(boxes, before[1])), (pt.scene_tree_cost(), RC.tree_cost_numpy(top, links))):
            assert abs(got - want) <= 1e-9 * want, (name, got, want)
    after = pt.scene_counts()
    assert after["blas_builds"] == counts["blas_builds"] and after["refits"] == counts["refits"] + 3
    assert {k: after[k] for k in ("objects", "triangles", "blas_nodes", "blas_records")} == {k: counts[k] for k in ("objects", "triangles", "blas_nodes", "blas_records")}
    pt.close()


@pytest.mark.parametrize("which", sorted(SCENES))
def test_a_repose_on_top_equals_refit_mesh(srt, which):
    """refit_mesh_inplace(V) followed by repose(family, same transforms) - the rebuild refit_mesh ends with - equals refit_mesh(V);
    and repose_refit(family, same transforms) on top of the in-place refit changes nothing."""
    S = SCENES[which]()
    nobj, index = len(S["objects"]), UC.BLOB_OBJECT
    family = RI.family_of(S, index)
    Ts = PR.transforms_of(S)[family]
    for name, (p, n) in UC.deformations().items():
        a, b = host_pt(srt, S), host_pt(srt, S)
        a.refit_mesh_inplace(index, p, n)
        kept = IC.all_dumps(a, nobj)
        a.repose_refit(family, Ts)
        assert IC.dumps_equal(IC.all_dumps(a, nobj), kept), name
        a.repose(family, Ts)
        b.refit_mesh(index, p, n)
        assert IC.dumps_equal(IC.all_dumps(a, nobj), IC.all_dumps(b, nobj)), name
        a.close(); b.close()


def test_inactive_mesh_and_instance(srt):
    """With the blob's instance and a wall switched off, then the blob itself: the masked fold and the counts the walks see stay
    right through refits; after reactivation the boxes are those of the unmasked fold."""
    S = IC.sweeps_scene()
    nobj, index = len(S["objects"]), UC.BLOB_OBJECT
    inst = RI.family_of(S, index)[1]
    (p1, n1), (p2, n2) = UC.deformations()["D1"], UC.deformations()["D2"]
    pt, plain = host_pt(srt, S), host_pt(srt, S)
    before, before_top = mesh_dump(pt, index, nobj), pt.dump_bvh(-1)
    pt.set_active([inst, 1], [0, 0])
    pt.refit_mesh_inplace(index, p1, n1)
    active = np.ones(nobj, np.uint8)
    active[[inst, 1]] = 0
    check_mesh(pt, S, index, before, p1)
    check_top(pt, S, index, before_top, p1, active)
    assert np.array_equal(pt.active(), active)
    pt.set_active([index], [0])
    active[index] = 0
    pt.refit_mesh_inplace(index, p2, n2)
    check_top(pt, S, index, before_top, p2, active)
    # the emulation agrees on what the walks see: the hidden objects are hit by no ray
    e = RI.EmuInplace(S)
    RI.apply_steps(e, [("active", [inst, 1], [0, 0]), ("inplace", index, p1, n1), ("active", [index], [0]), ("inplace", index, p2, n2)])
    assert RC.bits_equal(e.dump_top()[0], pt.dump_bvh(-1)[0])
    org, d, b = random_rays(RI.RAY_SEED, RI.RAYS)
    nested, flat = e.hit9(org, d, b)
    e.close()
    hidden = {int(S["objects"][k]["material"]) for k in (inst, index, 1)} - {int(o["material"]) for k, o in enumerate(S["objects"]) if k not in (inst, index, 1)}
    assert RC.bits_equal(nested, flat) and not (set(nested[nested[:, 0] != 0][:, 8].astype(int)) & hidden)
    pt.set_active([inst, 1, index], [1, 1, 1])
    plain.refit_mesh_inplace(index, p1, n1)
    plain.refit_mesh_inplace(index, p2, n2)
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(plain, nobj))
    check_top(pt, S, index, before_top, p2)
    pt.close(); plain.close()


def test_degenerate_shapes(srt):
    # a mesh of <= 4 triangles: the root is a leaf, there are no records
    P = IC.scenes_module().cornell_with_mesh(3, "glass")
    small = dict(P["objects"][6])
    small.update(pos=np.ascontiguousarray(small["pos"][:9]), nrm=np.ascontiguousarray(small["nrm"][:9]), idx=np.arange(9, dtype=np.uint32))
    P["objects"][6] = small
    pt = host_pt(srt, P)
    before, before_top = mesh_dump(pt, 6, 8), pt.dump_bvh(-1)
    assert len(before[0]) == 1 and before[1][0][2] == before[1][0][3]
    p = (small["pos"] * np.float32(1.25)).astype(np.float32)
    pt.refit_mesh_inplace(6, p, small["nrm"])
    check_mesh(pt, P, 6, before, p)
    check_top(pt, P, 6, before_top, p)
    pt.close()
    # the 48-level chain under a BVH<Object> nesting 24
    D = pt_scene("deep_both")
    nobj = len(D["objects"])
    pt = host_pt(srt, D)
    before, before_top = mesh_dump(pt, RC.DEEP_MESH, nobj), pt.dump_bvh(-1)
    p, n = RC.deep_moved(D)
    pt.refit_mesh_inplace(RC.DEEP_MESH, p, n)
    check_mesh(pt, D, RC.DEEP_MESH, before, p)
    check_top(pt, D, RC.DEEP_MESH, before_top, p)
    pt.close()
    # flat boxes: every vertex in one plane - Triangle::bbox widens the flat axis by +1.0f, the root box and the posed box follow
    S = UC.blob_scene()
    pt = host_pt(srt, S)
    before, before_top = mesh_dump(pt, 6, 8), pt.dump_bvh(-1)
    fp, fn = UC.original(S, 6)
    fp = fp.copy()
    fp[:, 2] = np.float32(0.25)
    pt.refit_mesh_inplace(6, fp, fn)
    boxes = check_mesh(pt, S, 6, before, fp)
    check_top(pt, S, 6, before_top, fp)
    assert np.all(boxes[:, 2] == np.float32(0.25)) and np.all(boxes[:, 5] == np.float32(1.25))
    pt.close()


def test_every_refusal_leaves_the_scene_alone(srt):
    lib = srt.load_library()
    S = RC.refusal_scene()
    nobj = len(S["objects"])
    p, n = UC.deformations()["D1"]
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    assert lib.srt_pt_refit_mesh_inplace(pt._ctx, 6, H.P(p), H.P(n), len(p)) == STATE        # before commit
    assert lib.srt_pt_refit_mesh_inplace_device(pt._ctx, None, 6, H.P(p), H.P(n), len(p)) == STATE
    pt.build_scene(S)
    first, counts = IC.all_dumps(pt, nobj), pt.scene_counts()

    def unchanged(what):
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.scene_counts() == counts and pt.mesh_refit_pending() == (0, 0), what

    assert lib.srt_pt_refit_mesh_inplace(None, 6, H.P(p), H.P(n), len(p)) == INVALID
    assert lib.srt_pt_refit_mesh_inplace(pt._ctx, 6, None, H.P(n), len(p)) == INVALID and lib.srt_pt_refit_mesh_inplace(pt._ctx, 6, H.P(p), None, len(p)) == INVALID
    assert lib.srt_pt_refit_mesh_inplace_device(None, None, 6, H.P(p), H.P(n), len(p)) == INVALID
    assert lib.srt_pt_refit_mesh_inplace_device(pt._ctx, None, 6, None, H.P(n), len(p)) == INVALID
    assert lib.srt_pt_mesh_refit_pending(pt._ctx, None) == INVALID and lib.srt_pt_mesh_refit_pending(None, None) == INVALID
    assert lib.srt_pt_skin_pose_inplace(None, None, H.P(p), 0) == INVALID and lib.srt_pt_skin_pose_inplace_at(None, None, ctypes.c_float(0.5), 0) == INVALID
    for what, index, pp, nn, nverts in RC.refused_arguments(S):
        pp, nn = np.ascontiguousarray(pp, np.float32), np.ascontiguousarray(nn, np.float32)
        nv = len(pp) if nverts is None else nverts
        assert lib.srt_pt_refit_mesh_inplace(pt._ctx, index, H.P(pp), H.P(nn), nv) == INVALID, what
        unchanged(what)
        # the device form validates first too (the pointers are never read on a host-only context) ..
        assert lib.srt_pt_refit_mesh_inplace_device(pt._ctx, None, index, H.P(pp), H.P(nn), nv) == INVALID, what
        unchanged(what)
    # .. and then refuses the host-only context
    with pytest.raises(srt.SrtError, match="host-only") as e:
        pt.refit_mesh_inplace_device(6, p.ctypes.data, n.ctypes.data, len(p))
    assert e.value.status == UNSUPPORTED
    unchanged("the device form on a host-only context")
    # the messages are refit_mesh's
    for index, pp in ((8, p), (7, UC.original(S, 7)[0]), (5, p)):
        texts = []
        for call in (lib.srt_pt_refit_mesh, lib.srt_pt_refit_mesh_inplace):
            assert call(pt._ctx, index, H.P(pp), H.P(np.ascontiguousarray(pp)), len(pp)) == INVALID
            texts.append(lib.srt_last_error().decode().split(": ", 1)[1])
        assert texts[0] == texts[1], index
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[len(q) // 2, 1] = bad
        with pytest.raises(srt.SrtError, match="non-finite") as e:
            pt.refit_mesh_inplace(6, q, n)
        assert e.value.status == INVALID
        unchanged(bad)
    # all vertices at one point: nothing is built, so nothing can fail to terminate
    pt.refit_mesh_inplace(6, *UC.one_point(S, 6))
    assert pt.scene_counts()["refits"] == counts["refits"] + 1 and pt.scene_counts()["blas_builds"] == counts["blas_builds"]
    pt.close()
    # list mode: no trees - the call does what update_mesh does
    lst, upd = host_pt(srt, S, use_bvh=False), host_pt(srt, S, use_bvh=False)
    c0 = lst.scene_counts()
    lst.refit_mesh_inplace(6, p, n)
    upd.update_mesh(6, p, n)
    assert lst.scene_counts() == c0 == upd.scene_counts()
    lst.close(); upd.close()


@pytest.mark.parametrize("which", sorted(SCENES))
def test_closest_hits_equal_the_oracle(scenes, which):
    """After each deformation the emulation's closest hits on the in-place refitted trees equal the oracle's on a fresh commit of the
    new vertices on all 2048 rays of RI.RAY_SEED - closest hits do not depend on the trees except at exact ties.  Exceptions: 0."""
    S = SCENES[which]()
    index = UC.BLOB_OBJECT
    org, d, b = random_rays(RI.RAY_SEED, RI.RAYS)
    e = RI.EmuInplace(S)
    for name, (p, n) in UC.deformations().items():
        assert e.refit_inplace(index, p, n) == 0
        nested, flat = e.hit9(org, d, b)
        o = H.OraclePT(IC.expand(scenes.with_vertices(S, index, p, n)), RC.W, RC.HT, RC.DEPTH, True)       # (an instance as a copy of its source)
        want = o.hit(org, d, b)
        differing = int(np.count_nonzero(np.any(np.ascontiguousarray(nested).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32), axis=1)))
        print(which, name, "rays differing from the oracle:", differing)
        assert differing <= RI.TIES_CAP and RC.bits_equal(nested, flat), (which, name, differing)
    e.close()


def test_sanitized_refit_inplace(tmp_path):
    """tests/host_emu/refit_inplace_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone - built with AddressSanitizer
    and UndefinedBehaviorSanitizer and run once on the CPU."""
    H.run_sanitized_main(tmp_path, "refit_inplace_sanitized_main.cpp")
