"""CPU: srt_pt_repose_refit on the host side - the definition (prepare_top_refit / apply_top_refit, pt_scene.cpp) through the ABI on a
host-only context, against a numpy restatement of the boxes and against srt_pt_repose / a fresh commit wherever a refit and a
build must agree; the emulation of a refitted scene (tests/host_emu/repose_refit_flat_host.cpp) against the oracle's closest
hits on a fresh commit of the same poses; refusals; and a sanitized stand-alone program over the definition and the settle path."""
import os
import re

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _light_cases as LC
import _repose_device_cases as RDC
import _repose_refit_cases as C
from _cases import random_rays
from _refit_cases import tree_cost_numpy

INVALID, STATE, UNSUPPORTED = -1, -5, -4


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def particles():
    S = IC.particles_shared()[0]
    idx, Ts = IC.repose_case(S)
    return {"S": S, "idx": idx, "Ts": Ts, "home": np.array([S["objects"][i]["T"] for i in idx], np.float32)}


def host_pt(srt, scene, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, use_bvh)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    return pt


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    for name in ("srt_pt_repose_refit", "srt_pt_repose_refit_device", "srt_pt_scene_tree_cost", "srt_pt_top_refit_count", "srt_pt_top_refit_pending"):
        assert getattr(lib, name) is not None, name
    for name in ("repose_refit", "repose_refit_device", "scene_tree_cost", "top_refit_count"):
        assert callable(getattr(srt.Pathtracer, name)), name
    for name in ("repose_refit", "repose_refit_device"):
        assert callable(getattr(srt.PathtracerGroup, name)), name
    for header, names in (("srt_pt.h", ("srt_pt_repose_refit(", "srt_pt_repose_refit_device(", "srt_pt_scene_tree_cost(")), ("srt_pt_debug.h", ("srt_pt_top_refit_count(",))):
        text = open(os.path.join(H.ROOT, "include", header)).read()
        assert all(n in text for n in names), header


def test_committed_poses_give_the_commit_back(srt, particles):
    S, idx = particles["S"], particles["idx"]
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    first, cost = IC.all_dumps(pt, nobj), pt.scene_tree_cost()
    pt.repose_refit(idx, particles["home"])
    pt.repose_refit([], np.zeros((0, 16), np.float32))
    same, count, cost_after = IC.dumps_equal(IC.all_dumps(pt, nobj), first), pt.top_refit_count(), pt.scene_tree_cost()
    pt.close()
    assert same and count == 2 and cost_after == cost


@pytest.mark.parametrize("which", ["particles", "sweeps"])
def test_boxes_are_the_folds(srt, particles, which):
    """Links and order stay; the boxes are the numpy restatement's; every BVH<Triangle> stays; the cost is tree_cost of the dump;
    and back home the committed boxes return."""
    if which == "particles":
        S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    else:
        S = IC.sweeps_scene()
        idx, Ts = C.sweeps_case(S)
    nobj = len(S["objects"])
    pt = host_pt(srt, S)
    first = IC.all_dumps(pt, nobj)
    pt.repose_refit(idx, Ts)
    moved = IC.all_dumps(pt, nobj)
    cost = pt.scene_tree_cost()
    pt.repose_refit(idx, [S["objects"][int(i)]["T"] for i in idx])
    back = IC.all_dumps(pt, nobj)
    pt.close()
    boxes, links, order = moved[0]
    assert np.array_equal(links, first[0][1]) and np.array_equal(order, first[0][2])
    assert not C.bits_equal(boxes, first[0][0])
    assert C.bits_equal(boxes, C.expected_top_boxes(S, idx, Ts, links, order))
    assert IC.dumps_equal(moved[1:], first[1:])
    assert abs(cost - tree_cost_numpy(boxes, links)) <= 1e-9 * cost
    assert IC.dumps_equal(back, first)


def test_refit_then_rebuild_is_a_fresh_commit(srt, particles):
    """A refit of poses P followed by srt_pt_repose of the same P: the scene a fresh commit of the new description builds; the
    cost rises when the particles are scattered and returns to the fresh commit's with the rebuild."""
    S = particles["S"]
    nobj = len(S["objects"])
    idx, Ts = C.scatter(S, C.particle_indices(), spread=1.0)
    pt = host_pt(srt, S)
    cost0 = pt.scene_tree_cost()
    pt.repose_refit(idx, Ts)
    cost1 = pt.scene_tree_cost()
    pt.repose(idx, Ts)
    cost2, dumps = pt.scene_tree_cost(), IC.all_dumps(pt, nobj)
    pt.close()
    fresh = host_pt(srt, IC.with_poses(S, idx, Ts))
    want, fresh_cost = IC.all_dumps(fresh, nobj), fresh.scene_tree_cost()
    fresh.close()
    print(f"tree cost: committed {cost0:.3f}, scattered and refitted {cost1:.3f}, rebuilt {cost2:.3f}")
    assert IC.dumps_equal(dumps, want)
    assert cost1 > cost0 and cost1 > cost2 and cost2 == fresh_cost


def test_emulation_agrees_with_the_oracle_on_closest_hits(particles):
    """Closest hits do not depend on the tree except at exact ties: the emulation's hit records after a refit of the scattered
    particles (both walks) against the oracle's on a fresh commit of the same poses, over the 2048 random rays.  C.POSE_SEED was
    chosen so that no ray differs; the GPU is held to the same."""
    S = particles["S"]
    idx, Ts = C.scatter(S, C.particle_indices())
    want = C.expectation(S, [(idx, Ts)], samples=False)
    org, d, b = random_rays(C.RAY_SEED, C.RAYS)
    o = H.OraclePT(IC.expand(IC.with_poses(S, idx, Ts)), C.W, C.HT, C.DEPTH, True)
    oracle = np.ascontiguousarray(o.hit(org, d, b), np.float32)
    for walk, got in zip(("nested", "flattened"), want["hits"]):
        differ = int(np.sum(np.any(got.view(np.uint32) != oracle.view(np.uint32), axis=1)))
        print(f"{walk} walk: {differ} of {C.RAYS} rays differ from the oracle (seed {C.POSE_SEED})")
        assert differ <= C.TIES_CAP == 0
    assert np.count_nonzero(oracle[:, 0]) > 500
    # and the emulated refit of the committed poses is the emulated commit
    home = [S["objects"][int(i)]["T"] for i in idx]
    again, commit = C.expectation(S, [(idx, home)], samples=False), C.expectation(S, [], samples=False)
    assert all(C.bits_equal(x, y) for x, y in zip(again["hits"], commit["hits"])) and C.bits_equal(again["dump"][0], commit["dump"][0])


def test_one_object_a_list_scene_and_an_identity(srt, particles):
    one = C.one_object_scene()
    pt = host_pt(srt, one)
    boxes0, links0, _ = pt.dump_bvh(-1)
    T = IC.translate(one["objects"][0]["T"], (0.1, 0.2, -0.1))
    pt.repose_refit([0], [T])
    boxes, links, order = pt.dump_bvh(-1)
    pt.close()
    assert len(links) == 1 and links[0][2] == links[0][3] and np.array_equal(links, links0)          # the root is a leaf: no record, no level
    assert C.bits_equal(boxes, C.expected_top_boxes(one, [0], [T], links, order)) and not C.bits_equal(boxes, boxes0)
    # a list scene has no tree: the call rewrites the records only, and a rebuild-free repose of the same poses is what it equals
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    lst = host_pt(srt, S, use_bvh=False)
    lst.repose_refit(idx, Ts)
    with pytest.raises(srt.SrtError) as e:
        lst.scene_tree_cost()
    assert e.value.status == UNSUPPORTED and lst.top_refit_count() == 1
    lst.close()
    # an identity with -0 off the diagonal: has_trans becomes 0, the box is the object-space box
    ident = RDC.identity()
    ident[[1, 2, 4, 6, 8, 9, 12, 13, 14]] = np.float32(-0.0)
    a = IC.PARTICLE_FIRST + IC.PARTICLE_COUNT
    pt = host_pt(srt, S)
    pt.repose_refit([a], [ident])
    boxes, links, order = pt.dump_bvh(-1)
    pt.close()
    slot = int(np.nonzero(order == a + 1)[0][0])
    leaf = [k for k in range(len(links)) if links[k][2] == links[k][3] and links[k][1] == 1 and links[k][0] == slot][0]
    assert C.bits_equal(boxes[leaf], C.local_boxes_numpy(S)[a])
    assert C.bits_equal(boxes, C.expected_top_boxes(S, [a], [ident], links, order))


def test_hostile_matrices_are_not_refused(srt, particles):
    """-0, denormals, singular matrices and a NaN: no refusal, links and order stay, the boxes are the restated folds (NaNs
    compared as NaNs; a NaN bound is never taken by a fold)."""
    S = particles["S"]
    pidx = C.particle_indices()
    for name, M in RDC.matrix_cases().items():
        M = M[:len(pidx)]
        idx = pidx[:len(M)]
        pt = host_pt(srt, S)
        first = pt.dump_bvh(-1)
        pt.repose_refit(idx, M)
        boxes, links, order = pt.dump_bvh(-1)
        pt.close()
        assert np.array_equal(links, first[1]) and np.array_equal(order, first[2]), name
        assert C.bits_equal_nan(boxes, C.expected_top_boxes(S, idx, M, links, order)), name


def test_dynamic_lights_on_the_host(srt):
    """With the switch on, a reposed emissive quad and an emissive sphere take the light records srt_pt_repose gives them; with it
    off, the refusal is srt_pt_repose's."""
    S = LC.three_light_scene()
    idx = np.array([LC.CBOX_LIGHT, 9], np.uint32)
    Ts = np.array([LC.poses(S["objects"][int(i)]["T"])["rotation * scale"] for i in idx], np.float32)
    a, b = host_pt(srt, S, dynamic=True), host_pt(srt, S, dynamic=True)
    first = a.dump_lights()
    a.repose_refit(idx, Ts)
    b.repose(idx, Ts)
    got, want = a.dump_lights(), b.dump_lights()
    a.close(); b.close()
    assert LC.lights_equal(got, want) and not LC.lights_equal(got, first)
    off = host_pt(srt, S)
    messages = []
    for call in (off.repose, off.repose_refit):
        with pytest.raises(srt.SrtError, match="area light") as e:
            call(idx, Ts)
        assert e.value.status == INVALID
        messages.append(str(e.value).replace("srt_pt_repose_refit", "srt_pt_repose"))
    off.close()
    assert messages[0] == messages[1]


def test_refusals_leave_the_scene(srt, particles):
    """Every argument srt_pt_repose refuses, a NULL pointer, no commit, and the device form on a host-only context (which validates
    first): status and message, and the scene as it was."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    nobj = len(S["objects"])
    light = [k for k, o in enumerate(S["objects"]) if o.get("is_light")][0]
    pt = host_pt(srt, S)
    first = IC.all_dumps(pt, nobj)
    cases = [("area light", [int(idx[0]), light]), ("listed twice", [int(idx[1]), int(idx[1])]), ("out of range", [nobj, int(idx[1])])]
    for match, bad in cases:
        for call, name in ((pt.repose_refit, "srt_pt_repose_refit"), (lambda i, T: pt.repose_refit_device(i, T.ctypes.data), "srt_pt_repose_refit_device")):
            with pytest.raises(srt.SrtError, match=match) as e:
                call(bad, Ts[:2])
            assert e.value.status == INVALID and name + ":" in str(e.value)
        with pytest.raises(srt.SrtError, match=match) as r:
            pt.repose(bad, Ts[:2])
        assert re.split(r"srt_pt_\w+: ", str(r.value), 1)[1] == re.split(r"srt_pt_\w+: ", str(e.value), 1)[1]
    L = pt._lib
    assert L.srt_pt_repose_refit(pt._ctx, None, None, 2) == INVALID and L.srt_pt_repose_refit_device(pt._ctx, None, idx.ctypes.data, None, 2) == INVALID
    assert L.srt_pt_scene_tree_cost(pt._ctx, None) == INVALID and L.srt_pt_top_refit_count(pt._ctx, None) == INVALID
    with pytest.raises(srt.SrtError, match="host-only") as e:
        pt.repose_refit_device(idx, Ts.ctypes.data)
    assert e.value.status == UNSUPPORTED
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.top_refit_count() == 0
    pt.close()
    empty = srt.Pathtracer(device=-1)
    for call in (lambda: empty.repose_refit(idx, Ts), lambda: empty.repose_refit_device(idx, Ts.ctypes.data), empty.scene_tree_cost):
        with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
            call()
        assert e.value.status == STATE
    empty.close()


def test_sanitized_definition_and_settle(tmp_path, particles):
    """tests/host_emu/repose_refit_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: the definition and the
    settle-apply path on the 74-object particle scene and repose_case's list - built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once on the CPU."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    scene_file = str(tmp_path / "particles.scene")
    RDC.write_scene_file(scene_file, S, idx, Ts)
    H.run_sanitized_main(tmp_path, "repose_refit_sanitized_main.cpp", args=[scene_file], expect="repose_refit_sanitized: ok (74 objects, 12 listed)")
