"""CPU: srt_pt_set_dynamic_lights on the host side.  The device functions of pt_light_update.h compiled for the host against
light_record / light_area_term / light_tri_record of pt_scene.cpp; the scene layer's repose / update / refit of area lights
(through tests/host_emu/lights_host.cpp) against a fresh build_scene of the same description, light tables byte for byte;
refusals that leave the scene as it was; the ABI on a host-only context; and a sanitized stand-alone program."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _light_cases as LC
import _repose_device_cases as RC
import _update_cases as UC

INVALID, UNSUPPORTED, STATE = -1, -4, -5          # SRT_ERR_* (include/srt_raster.h)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def test_device_functions_on_the_host():
    """light_matrices / light_area / light_triangle under every matrix of matrix_cases(), over a zero-area triangle (the term is
    inf), triangles with signed-zero coordinates and the 128 triangles of a deformed blob."""
    lib = LC.lights_lib()
    vals = np.array([0.0, -0.0, 0.25, -0.25], np.float32)
    tri = np.array([[a, b, c] for a in vals for b in vals for c in vals], np.float32)            # 64 triangles' x coordinates
    zp = np.stack([tri, tri[:, ::-1], np.roll(tri, 1, axis=1)], axis=2).reshape(-1, 3).astype(np.float32)
    flat = np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.4, -0.1, 0.2], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.8, 0.8, 0.8]], np.float32)   # a repeated corner; collinear
    bp, bn, _ = UC.blob_arrays(2, seed=11)
    assert len(bp) == 3 * 128
    pos = np.ascontiguousarray(np.concatenate([flat, zp, bp]), np.float32)
    nrm = np.ascontiguousarray(np.concatenate([np.tile(np.array([0.0, -0.0, 1.0], np.float32), (len(flat) + len(zp), 1)), bn]), np.float32)
    idx = np.arange(len(pos), dtype=np.uint32)
    total = {"inf": 0, "nan": 0, "no_trans": 0, "trans": 0}
    for name, mats in RC.matrix_cases().items():
        mats = np.ascontiguousarray(mats, np.float32).reshape(-1, 16)
        out = np.zeros(4, np.uint32)
        assert lib.lit_emu_mismatches(H.P(mats), len(mats), H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx) // 3, H.P(out)) == 0, name
        for k, v in zip(total, out):
            total[k] += int(v)
        if name in ("identity", "identity with -0"):
            assert out[2] == 1 and out[3] == 0 and out[0] >= 2, name      # has_trans 0: the pdf pair are identities; the flat triangles give inf
        if name == "NaN":                                                   # (a singular pose puts its NaNs into itrans and pdfiT; the area terms read pdfT)
            assert out[1] > 0, name
    assert total["inf"] > 0 and total["nan"] > 0 and total["no_trans"] >= 2 and total["trans"] > 300


def committed_T(S, index):
    return np.ascontiguousarray(S["objects"][index]["T"], np.float32).reshape(16)


REPOSE_CASES = {"quad": (LC.blob_light_scene, LC.CBOX_LIGHT), "blob": (LC.blob_light_scene, LC.BLOB_LIGHT), "sphere": (LC.three_light_scene, 9)}


@pytest.mark.parametrize("which", sorted(REPOSE_CASES))
@pytest.mark.parametrize("use_bvh", [True, False])
def test_repose_of_a_light_equals_fresh_build(which, use_bvh):
    """The light through the three poses, each against a fresh build of the description with that pose; then back to the committed
    pose: the first scene, storage included."""
    make, index = REPOSE_CASES[which]
    S = make()
    first = LC.LightScene(S, use_bvh, dynamic=True)
    hs = first.clone()
    seen = []
    for name, T in LC.poses(committed_T(S, index)).items():
        fresh = LC.LightScene(IC.with_poses(S, [index], [T]), use_bvh, may_fail=True)
        if fresh.failed:
            # the quad under the identity has the floor's centre: no commit of that description terminates, and neither does the repose
            assert (which, use_bvh, name) == ("quad", True, "identity") and "does not terminate" in fresh.failed
            kept = hs.clone()
            assert hs.repose([index], [T]) == 2 and "does not terminate" in hs.error() and hs.identical(kept)
            kept.close(); fresh.close()
            continue
        assert hs.repose([index], [T]) == 0, (name, hs.error())
        assert hs.same_computed(fresh), (which, use_bvh, name)
        assert LC.lights_equal(hs.dump_lights(), fresh.dump_lights()), name
        assert not LC.lights_equal(hs.dump_lights(), first.dump_lights()), name
        light = [k for k in range(len(hs.dump_lights()["heads"])) if hs.dump_lights()["heads"][k, 3] == index][0]
        seen.append(int(hs.dump_lights()["heads"][light, 0]))
        fresh.close()
    assert seen == ([1, 1] if (which, use_bvh) == ("quad", True) else [1, 1, 0])
    assert hs.repose([index], [committed_T(S, index)]) == 0
    assert hs.identical(first)
    hs.close(); first.close()


@pytest.mark.parametrize("use_bvh", [True, False])
def test_update_and_refit_of_an_emissive_mesh(scenes, use_bvh):
    """D1, D2, D3 in turn on the emissive blob, each by update and by refit, against a fresh build of scenes.with_vertices: an
    update in everything computed, a refit - whose tree is the kept one - in the light tables, the poses, the BVH<Object> and the
    vertex arrays; then the original arrays again."""
    S = LC.blob_light_scene()
    index = LC.BLOB_LIGHT
    first = LC.LightScene(S, use_bvh, dynamic=True)
    up, rf = first.clone(), first.clone()
    for name, (p, n) in LC.blob_light_deformations().items():
        assert up.update(index, p, n) == 0, up.error()
        fresh = LC.LightScene(scenes.with_vertices(S, index, p, n), use_bvh)
        assert up.same_computed(fresh) and LC.lights_equal(up.dump_lights(), fresh.dump_lights()), (use_bvh, name)
        assert not LC.lights_equal(up.dump_lights(), first.dump_lights())
        assert rf.refit(index, p, n) == (0 if use_bvh else 1)                    # (the scene layer refits trees only; the ABI updates a list scene)
        if use_bvh:
            assert rf.same_but_trees(fresh) and LC.lights_equal(rf.dump_lights(), fresh.dump_lights()), name
        fresh.close()
    p0, n0 = UC.original(S, index)
    assert up.update(index, p0, n0) == 0 and up.same_computed(first)
    if use_bvh:
        assert rf.refit(index, p0, n0) == 0 and rf.same_but_trees(first) and rf.update(index, p0, n0) == 0 and rf.same_computed(first)
    for x in (first, up, rf):
        x.close()


@pytest.mark.parametrize("use_bvh", [True, False])
def test_update_repose_update_of_one_light(scenes, use_bvh):
    S = LC.blob_light_scene()
    index = LC.BLOB_LIGHT
    D = LC.blob_light_deformations()
    T = LC.poses(committed_T(S, index))["rotation * scale"]
    Tq = LC.poses(committed_T(S, LC.CBOX_LIGHT))["translation"]
    first = LC.LightScene(S, use_bvh, dynamic=True)
    hs = first.clone()
    assert hs.update(index, *D["D1"]) == 0 and hs.repose([index, LC.CBOX_LIGHT], [T, Tq]) == 0
    assert hs.update(index, *D["D2"]) == 0
    want = LC.LightScene(IC.with_poses(scenes.with_vertices(S, index, *D["D2"]), [index, LC.CBOX_LIGHT], [T, Tq]), use_bvh)
    assert hs.same_computed(want) and LC.lights_equal(hs.dump_lights(), want.dump_lights())
    assert hs.update(index, *UC.original(S, index)) == 0 and hs.repose([LC.CBOX_LIGHT, index], [committed_T(S, LC.CBOX_LIGHT), committed_T(S, index)]) == 0
    assert hs.same_computed(first)
    for x in (first, hs, want):
        x.close()


def emissive_chain_scene():
    """UC.flat_chain_scene() with the chain mesh emissive: a light whose deformation nests 49 deep."""
    S, arrays = UC.flat_chain_scene()
    S = dict(S, objects=list(S["objects"]))
    S["objects"][6] = dict(S["objects"][6], is_light=True, material=7)
    return S, arrays


@pytest.mark.parametrize("use_bvh", [True, False])
def test_refusals_with_the_switch_on_leave_the_scene_identical(use_bvh):
    S = LC.three_light_scene()
    S["objects"].append(LC.blob_light_scene()["objects"][LC.BLOB_LIGHT])       # object 11: the emissive blob
    blob, sphere, nobj = 11, 9, 12
    hs = LC.LightScene(S, use_bvh, dynamic=True)
    before = hs.clone()
    lights = hs.dump_lights()
    T = LC.poses(committed_T(S, LC.CBOX_LIGHT))["translation"]
    p, n = UC.original(S, blob)
    lp, ln = UC.original(S, LC.CBOX_LIGHT)

    def unchanged(what):
        assert hs.identical(before) and LC.lights_equal(hs.dump_lights(), lights), what

    assert hs.repose([LC.CBOX_LIGHT, 5, LC.CBOX_LIGHT], [T, T, T]) == 1 and "listed twice" in hs.error()
    unchanged("a duplicate")
    assert hs.repose([LC.CBOX_LIGHT, nobj], [T, T]) == 1 and "out of range" in hs.error()
    unchanged("out of range")
    assert hs.update(sphere, lp, ln) == 1 and "is a sphere" in hs.error()
    unchanged("update of the sphere light")
    assert hs.refit(sphere, lp, ln) == 1 and "is a sphere" in hs.error()
    unchanged("refit of the sphere light")
    bad = p.copy()
    bad[17, 1] = np.inf
    assert hs.refit(blob, bad, n) == 1 and ("non-finite" in hs.error() or not use_bvh)
    unchanged("a non-finite refit position")
    if use_bvh:
        assert hs.update(blob, *UC.one_point(S, blob)) == 2 and "does not terminate" in hs.error()
        unchanged("one point")
    # the switch cleared: today's refusals, today's messages
    hs.set_dynamic(False)
    before.set_dynamic(False)
    assert hs.repose([LC.CBOX_LIGHT], [T]) == 1 and "is an area light: its light tables depend on its pose, commit the scene again" in hs.error()
    assert hs.repose([sphere], [T]) == 1 and "is an area light" in hs.error()
    assert hs.update(blob, p, n) == 1 and "is an area light: its light-list copy and light tables depend on its vertices, commit the scene again" in hs.error()
    assert hs.refit(blob, p, n) == 1 and "is an area light" in hs.error()
    unchanged("the switch cleared")
    hs.close(); before.close()


def test_deep_chain_on_a_light_is_refused():
    S, (cp, cn) = emissive_chain_scene()
    hs = LC.LightScene(S, True, dynamic=True)
    before = hs.clone()
    lights = hs.dump_lights()
    assert hs.depths()[1] < 48
    assert hs.update(6, cp, cn) == 2 and hs.identical(before) and LC.lights_equal(hs.dump_lights(), lights)
    hs.close(); before.close()


def host_pt(srt, scene, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, use_bvh)
    pt.set_dynamic_lights(dynamic)
    pt.build_scene(scene)
    return pt


def same_as_fresh(srt, pt, desc, use_bvh=True):
    fresh = host_pt(srt, desc, use_bvh)
    nobj = len(desc["objects"])
    ok = LC.lights_equal(pt.dump_lights(False), fresh.dump_lights(False))
    if use_bvh:
        ok = ok and IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj))
    fresh.close()
    return ok


def test_abi_on_a_host_only_context(srt, scenes):
    lib = srt.load_library()
    header = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    debug = open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()
    assert "int srt_pt_set_dynamic_lights(srt_pt* pt, int on);" in header and "int srt_pt_group_set_dynamic_lights(srt_pt_group* g, int on);" in header
    assert ("long srt_pt_dump_lights(srt_pt* pt, int from_device, uint32_t* heads, float* mats, size_t cap_lights, float* tris, size_t cap_tris);") in debug
    for name in ("srt_pt_set_dynamic_lights", "srt_pt_group_set_dynamic_lights", "srt_pt_dump_lights"):
        assert hasattr(lib, name)
    assert lib.srt_pt_set_dynamic_lights.argtypes == [ctypes.c_void_p, ctypes.c_int]
    for cls, names in ((srt.Pathtracer, ("set_dynamic_lights", "dump_lights")), (srt.PathtracerGroup, ("set_dynamic_lights",))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    assert lib.srt_pt_set_dynamic_lights(None, 1) == INVALID

    S = LC.blob_light_scene()
    quad, blob = LC.CBOX_LIGHT, LC.BLOB_LIGHT
    T = LC.poses(committed_T(S, quad))
    D = LC.blob_light_deformations()
    pt = host_pt(srt, S)
    first = pt.dump_lights(False)
    assert first["heads"].tolist() == [[0 if not np.any(committed_T(S, quad) != np.eye(4, dtype=np.float32).reshape(16)) else 1, 0, 2, quad],
                                       [1, 2, LC.BLOB_LIGHT_TRIS, blob]]
    assert lib.srt_pt_dump_lights(pt._ctx, 1, None, None, 0, None, 0) == UNSUPPORTED
    # off: refused as ever; on after the commit: accepted
    with pytest.raises(srt.SrtError, match="is an area light: its light tables depend on its pose, commit the scene again") as e:
        pt.repose([quad], [T["translation"]])
    assert e.value.status == INVALID
    with pytest.raises(srt.SrtError, match="is an area light: its light-list copy"):
        pt.update_mesh(blob, *D["D1"])
    with pytest.raises(srt.SrtError, match="is an area light: its light-list copy"):
        pt.refit_mesh(blob, *D["D1"])
    assert LC.lights_equal(pt.dump_lights(False), first)
    pt.set_dynamic_lights(True)
    idx = np.array([quad], np.uint32)
    assert lib.srt_pt_repose_device(pt._ctx, None, H.P(idx), H.P(T["translation"]), 1) == UNSUPPORTED
    Tb = LC.poses(committed_T(S, blob))
    for name in T:
        if name == "identity":            # the quad on the floor, with the floor's centre: what a commit of that description answers
            kept = pt.dump_lights(False)
            with pytest.raises(srt.SrtError, match="does not terminate") as e:
                pt.repose([quad, blob], [T[name], Tb[name]])
            assert e.value.status == UNSUPPORTED and LC.lights_equal(pt.dump_lights(False), kept)
            pt.repose([blob], [Tb[name]])
            desc = IC.with_poses(S, [quad, blob], [T["rotation * scale"], Tb[name]])
            assert pt.dump_lights(False)["heads"][:, 0].tolist() == [1, 0]
        else:
            pt.repose([quad, blob], [T[name], Tb[name]])
            desc = IC.with_poses(S, [quad, blob], [T[name], Tb[name]])
        assert same_as_fresh(srt, pt, desc), name
    pt.repose([quad, blob], [committed_T(S, quad), committed_T(S, blob)])
    assert same_as_fresh(srt, pt, S) and LC.lights_equal(pt.dump_lights(False), first)
    counts = pt.scene_counts()
    for name, (p, n) in D.items():
        pt.update_mesh(blob, p, n)
        assert same_as_fresh(srt, pt, scenes.with_vertices(S, blob, p, n)), name
    assert pt.scene_counts()["blas_builds"] == counts["blas_builds"] + 3
    pt.update_mesh(blob, *UC.original(S, blob))
    for name, (p, n) in D.items():
        pt.refit_mesh(blob, p, n)
        fresh = host_pt(srt, scenes.with_vertices(S, blob, p, n))
        assert LC.lights_equal(pt.dump_lights(False), fresh.dump_lights(False)), name
        fresh.close()
    pt.refit_mesh(blob, *UC.original(S, blob))
    assert LC.lights_equal(pt.dump_lights(False), first)
    # refusals through the ABI, the switch on
    before = pt.dump_lights(False)
    dumps = IC.all_dumps(pt, len(S["objects"]))
    bad = UC.original(S, blob)[0].copy()
    bad[3, 0] = np.nan
    for call, status, match in ((lambda: pt.repose([quad, quad], [T["translation"]] * 2), INVALID, "listed twice"),
                                (lambda: pt.repose([99], [T["translation"]]), INVALID, "out of range"),
                                (lambda: pt.refit_mesh(blob, bad, UC.original(S, blob)[1]), INVALID, "non-finite"),
                                (lambda: pt.update_mesh(blob, *UC.one_point(S, blob)), UNSUPPORTED, "does not terminate")):
        with pytest.raises(srt.SrtError, match=match) as e:
            call()
        assert e.value.status == status
        assert LC.lights_equal(pt.dump_lights(False), before) and IC.dumps_equal(IC.all_dumps(pt, len(S["objects"])), dumps), match
    # list mode
    lst = host_pt(srt, S, use_bvh=False, dynamic=True)
    lst.repose([quad], [T["rotation * scale"]])
    lst.refit_mesh(blob, *D["D2"])                           # a list has no tree: the update
    assert same_as_fresh(srt, lst, IC.with_poses(scenes.with_vertices(S, blob, *D["D2"]), [quad], [T["rotation * scale"]]), use_bvh=False)
    lst.close()
    pt.close()


def test_sanitized_lights(tmp_path):
    """tests/host_emu/lights_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: a light re-posed, updated, refitted,
    one refused call - built with AddressSanitizer and UndefinedBehaviorSanitizer and run once on the CPU."""
    H.run_sanitized_main(tmp_path, "lights_sanitized_main.cpp")
