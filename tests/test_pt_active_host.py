"""CPU: srt_pt_set_active on the host side - the definition (check_active_list / apply_set_active / mask_top, pt_scene.cpp) through
the ABI on a host-only context, against a numpy restatement of the masked boxes; the emulation of a scene with hidden objects
(tests/host_emu/active_flat_host.cpp) against the oracle's closest hits on a fresh commit without them; persistence across the calls
that rebuild or refit the BVH<Object>; refusals; and a sanitized stand-alone program over the definition and the settle bookkeeping.
(What needs a device even in its host form - srt_pt_particles_step, srt_pt_hit, the skins - is in test_pt_active_gpu.py.)"""
import os

import numpy as np
import pytest

import _active_cases as A
import _harness as H
import _instance_cases as IC
import _light_cases as LC
import _repose_device_cases as RDC
import _repose_refit_cases as C
import _update_cases as UC
from _cases import random_rays

INVALID, STATE, UNSUPPORTED = -1, -5, -4


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def particles():
    S = IC.particles_shared()[0]
    off = A.hidden()
    return {"S": S, "off": off, "nobj": len(S["objects"]), "zeros": np.zeros(len(off), np.uint8), "ones": np.ones(len(off), np.uint8)}


def host_pt(srt, scene, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, use_bvh)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    return pt


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    for name in ("srt_pt_set_active", "srt_pt_set_active_device", "srt_pt_get_active", "srt_pt_group_set_active", "srt_pt_group_set_active_device"):
        assert getattr(lib, name) is not None, name
    for name in ("set_active", "set_active_device", "active"):
        assert callable(getattr(srt.Pathtracer, name)), name
    for name in ("set_active", "set_active_device"):
        assert callable(getattr(srt.PathtracerGroup, name)), name
    text = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for n in ("srt_pt_set_active(", "srt_pt_set_active_device(", "srt_pt_get_active(", "srt_pt_group_set_active(", "srt_pt_group_set_active_device(",
              "NaN component", "ENQUEUE-ONLY", "root is a leaf", "use_bvh == 0", "SRT_ERR_UNSUPPORTED", "SRT_ERR_INVALID", "SRT_ERR_STATE"):
        assert n in text, n
    assert "needs a commit, as before" not in text


def test_boxes_are_the_masked_folds(srt, particles):
    """A seeded third of the particles off: links and order stay, the boxes are the numpy restatement's bit for bit, every
    BVH<Triangle> stays, the table round-trips and the cost is the numpy cost with the empty-node rule."""
    S, off, nobj = particles["S"], particles["off"], particles["nobj"]
    pt = host_pt(srt, S)
    first = IC.all_dumps(pt, nobj)
    assert np.array_equal(pt.active(), np.ones(nobj, np.uint8))
    pt.set_active(off, particles["zeros"])
    masked, table, cost = IC.all_dumps(pt, nobj), pt.active(), pt.scene_tree_cost()
    pt.close()
    boxes, links, order = masked[0]
    assert np.array_equal(links, first[0][1]) and np.array_equal(order, first[0][2])
    assert np.array_equal(table, A.flags_of(nobj, off))
    assert not A.bits_equal(boxes, first[0][0])
    assert A.bits_equal(boxes, A.expected_boxes(S, table, links, order))
    assert IC.dumps_equal(masked[1:], first[1:])
    want_cost = A.tree_cost_numpy(boxes, links)
    assert abs(cost - want_cost) <= 1e-12 * want_cost and np.any(boxes[:, 0] > boxes[:, 3])      # (some node is empty)
    # the emulation is the same definition
    e = A.expectation(S, [("active", off, particles["zeros"])], samples=False)
    assert A.bits_equal(e["dump"][0], boxes) and np.array_equal(e["active"], table) and e["cost"] == cost


def test_round_trip_and_no_change(srt, particles):
    """Off and on again: the committed boxes as values and the committed cost; a call that changes no flag leaves every dump
    byte-identical and the upload counter where it was."""
    S, off, nobj = particles["S"], particles["off"], particles["nobj"]
    pt = host_pt(srt, S)
    first, cost0, up0 = IC.all_dumps(pt, nobj), pt.scene_tree_cost(), pt.scene_counts()["uploaded_bytes"]
    pt.set_active(off, particles["ones"])                   # nothing changes
    pt.set_active([], [])
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first)
    pt.set_active(off, particles["zeros"])
    hidden = IC.all_dumps(pt, nobj)
    pt.set_active(off, particles["zeros"])                  # nothing changes
    pt.set_active(off[:3], [0, 0, 0])
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), hidden) and not IC.dumps_equal(hidden, first)
    pt.set_active(off, 5 * particles["ones"])               # any non-zero byte is active
    back, cost1, table, up1 = IC.all_dumps(pt, nobj), pt.scene_tree_cost(), pt.active(), pt.scene_counts()["uploaded_bytes"]
    pt.close()
    assert A.values_equal(back[0][0], first[0][0]) and np.array_equal(back[0][1], first[0][1]) and np.array_equal(back[0][2], first[0][2])
    assert IC.dumps_equal(back[1:], first[1:]) and cost1 == cost0 and np.all(table == 1) and up1 == up0


def test_emulation_agrees_with_the_oracle_on_closest_hits(particles):
    """Closest hits do not depend on the tree except at exact ties: the emulation's hit records with the particles of A.MASK_SEED
    hidden (both walks) against the oracle's on a fresh commit of the scene without them, over the 2048 random rays.  The seed was
    chosen so that no ray differs; the GPU is held to the same."""
    S, off = particles["S"], particles["off"]
    want = A.expectation(S, [("active", off, particles["zeros"])], samples=False)
    commit = A.expectation(S, [], samples=False)
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    o = H.OraclePT(A.without(S, off), A.W, A.HT, A.DEPTH, True)
    oracle = np.ascontiguousarray(o.hit(org, d, b), np.float32)
    for walk, got, all_on in zip(("nested", "flattened"), want["hits"], commit["hits"]):
        differ = A.mismatches(got, oracle)
        print(f"{walk} walk: {differ} of {A.RAYS} rays differ from the oracle (seed {A.MASK_SEED}); {A.mismatches(all_on, oracle)} rays hit a hidden particle before")
        assert differ <= A.TIES_CAP == 0
        assert A.mismatches(all_on, oracle) > 0             # (the hidden particles were in the way of some ray)
    assert np.count_nonzero(oracle[:, 0]) > 500


def test_all_particles_inactive(particles):
    """Every particle off - the source mesh of the instances included: the hits are the oracle's for the scene without particles."""
    S = particles["S"]
    off = A.particle_indices()
    want = A.expectation(S, [("active", off, np.zeros(len(off), np.uint8))], samples=False)
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    o = H.OraclePT(A.without(S, off), A.W, A.HT, A.DEPTH, True)
    oracle = np.ascontiguousarray(o.hit(org, d, b), np.float32)
    for got in want["hits"]:
        assert A.mismatches(got, oracle) <= A.TIES_CAP == 0
    assert int(np.sum(want["active"] == 0)) == IC.PARTICLE_COUNT and want["cost"] > 0.0


def test_a_hidden_source_keeps_its_instances(srt):
    """The blob of IC.sweeps_scene() off, its instance on: only the blob's own top-level box changes, and the instance is still hit."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    want = A.expectation(S, [("active", [UC.BLOB_OBJECT], [0])], samples=False)
    commit = A.expectation(S, [], samples=False)
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    o = H.OraclePT(A.without(S, [UC.BLOB_OBJECT]), A.W, A.HT, A.DEPTH, True)
    oracle = np.ascontiguousarray(o.hit(org, d, b), np.float32)
    assert A.mismatches(want["hits"][0], oracle) == 0 and A.mismatches(want["hits"][1], oracle) == 0
    assert A.mismatches(commit["hits"][0], oracle) > 0
    boxes, links, order = want["dump"]
    assert A.bits_equal(boxes, A.expected_boxes(S, A.flags_of(nobj, [UC.BLOB_OBJECT]), links, order))


def rebuild_calls(S):
    """(name, call(pt)) for the calls that rebuild or refit the BVH<Object> on a host-only context, on objects of IC.sweeps_scene()."""
    nobj = len(S["objects"])
    p, n = UC.deformations()["D1"]
    p3, n3 = UC.deformations()["D3"]
    idx, Ts = C.sweeps_case(S)                               # the instance (the last object) and a wall
    blob_T = [IC.translate(S["objects"][UC.BLOB_OBJECT]["T"], (0.05, 0.1, -0.05))]
    return nobj, [
        ("repose", lambda pt: pt.repose(idx, Ts)),
        ("repose of the hidden one", lambda pt: pt.repose([UC.BLOB_OBJECT], blob_T)),
        ("repose_refit", lambda pt: pt.repose_refit(idx, Ts)),
        ("repose_refit of the hidden one", lambda pt: pt.repose_refit([UC.BLOB_OBJECT], blob_T)),
        ("update_mesh of the hidden one", lambda pt: pt.update_mesh(UC.BLOB_OBJECT, p, n)),
        ("refit_mesh of the hidden one", lambda pt: pt.refit_mesh(UC.BLOB_OBJECT, p3, n3)),
    ]


def check_persistence(make, calls, nobj, off):
    """For every call: context a (objects `off` hidden) and context b (all active) run it.  The flags persist; a's topology and
    BVH<Triangle>s are b's; a's boxes are the masked fold of b's posed boxes (a leaf of b holds one object: its box is the posed
    box); and after reactivation a equals b as values - a hidden object moved while hidden sits at its new pose."""
    table = A.flags_of(nobj, off)
    for name, call in calls:
        a, b = make(), make()
        a.set_active(off, np.zeros(len(off), np.uint8))
        call(a)
        call(b)
        da, db, got_table = IC.all_dumps(a, nobj), IC.all_dumps(b, nobj), a.active()
        a.set_active(off, np.ones(len(off), np.uint8))
        back = IC.all_dumps(a, nobj)
        a.close(); b.close()
        assert np.array_equal(got_table, table), name
        assert np.array_equal(da[0][1], db[0][1]) and np.array_equal(da[0][2][:nobj], db[0][2][:nobj]), name
        assert IC.dumps_equal(da[1:], db[1:]), name
        posed = A.posed_from_leaves(db[0][0], db[0][1], db[0][2], nobj)
        assert A.bits_equal(da[0][0], C.top_boxes_numpy(da[0][1], da[0][2], A.masked(posed, table))), name
        assert not A.bits_equal(da[0][0], db[0][0]), name
        assert A.values_equal(back[0][0], db[0][0]) and np.array_equal(back[0][1], db[0][1]) and IC.dumps_equal(back[1:], db[1:]), name


def test_flags_persist_across_rebuilds_and_refits(srt):
    """repose, repose_refit, update_mesh and refit_mesh, on other objects and on the hidden one, with the blob and a wall hidden."""
    S = IC.sweeps_scene()
    nobj, calls = rebuild_calls(S)
    check_persistence(lambda: host_pt(srt, S), calls, nobj, [UC.BLOB_OBJECT, 2])


def test_refusals_leave_the_scene(srt, particles):
    """Emissive mesh and sphere light with and without dynamic lights, a duplicate, an index out of range, NULL arguments, no commit,
    a list scene, the one-object scene, the device form on a host-only context (which validates first): status, message, and every
    dump and the table as they were."""
    L = LC.three_light_scene()
    nl = len(L["objects"])
    flags2 = np.zeros(2, np.uint8)
    for dynamic in (False, True):
        pt = host_pt(srt, L, dynamic=dynamic)
        pt.set_active([1], [0])
        first, table = IC.all_dumps(pt, nl), pt.active()
        for bad in ([2, LC.CBOX_LIGHT], [9, 2]):            # the emissive quad, the emissive sphere
            for call, name in ((lambda: pt.set_active(bad, flags2), "srt_pt_set_active"), (lambda: pt.set_active_device(bad, flags2.ctypes.data), "srt_pt_set_active_device")):
                with pytest.raises(srt.SrtError, match="area light") as e:
                    call()
                assert e.value.status == INVALID and name + ":" in str(e.value)
        assert IC.dumps_equal(IC.all_dumps(pt, nl), first) and np.array_equal(pt.active(), table)
        pt.close()
    S, off, nobj = particles["S"], particles["off"], particles["nobj"]
    pt = host_pt(srt, S)
    pt.set_active(off[:4], [0, 0, 0, 0])
    first, table = IC.all_dumps(pt, nobj), pt.active()
    for match, bad in (("listed twice", [int(off[5]), int(off[5])]), ("out of range", [nobj, int(off[5])])):
        for call, name in ((lambda: pt.set_active(bad, flags2), "srt_pt_set_active"), (lambda: pt.set_active_device(bad, flags2.ctypes.data), "srt_pt_set_active_device")):
            with pytest.raises(srt.SrtError, match=match) as e:
                call()
            assert e.value.status == INVALID and name + ":" in str(e.value)
    lib = pt._lib
    assert lib.srt_pt_set_active(pt._ctx, None, None, 2) == INVALID and lib.srt_pt_set_active(pt._ctx, off.ctypes.data, None, 2) == INVALID
    assert lib.srt_pt_set_active_device(pt._ctx, None, off.ctypes.data, None, 2) == INVALID and lib.srt_pt_get_active(pt._ctx, None, nobj) == INVALID
    small = np.zeros(nobj - 1, np.uint8)
    assert lib.srt_pt_get_active(pt._ctx, small.ctypes.data, nobj - 1) == INVALID
    with pytest.raises(srt.SrtError, match="host-only") as e:
        pt.set_active_device(off, particles["zeros"].ctypes.data)
    assert e.value.status == UNSUPPORTED
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and np.array_equal(pt.active(), table)
    pt.close()
    empty = srt.Pathtracer(device=-1)
    for call in (lambda: empty.set_active(off, particles["zeros"]), lambda: empty.set_active_device(off, particles["zeros"].ctypes.data), empty.active):
        with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
            call()
        assert e.value.status == STATE
    empty.close()
    lst = host_pt(srt, S, use_bvh=False)
    with pytest.raises(srt.SrtError, match="without BVHs") as e:
        lst.set_active(off, particles["zeros"])
    assert e.value.status == UNSUPPORTED and np.all(lst.active() == 1)
    lst.close()
    one = host_pt(srt, A.one_object_scene())
    first = one.dump_bvh(-1)
    with pytest.raises(srt.SrtError, match="root of the BVH<Object> is a leaf") as e:
        one.set_active([0], [0])
    assert e.value.status == UNSUPPORTED and np.all(one.active() == 1) and A.bits_equal(one.dump_bvh(-1)[0], first[0])
    one.close()


def test_sanitized_definition_and_settle(tmp_path, particles):
    """tests/host_emu/active_sanitized_main.cpp - a stand-alone program over pt_scene.cpp alone: masking, the fold, the cost, the
    rebuild and refit paths while objects are hidden and the settle bookkeeping, on the 74-object particle scene and repose_case's
    list - built with AddressSanitizer and UndefinedBehaviorSanitizer and run once on the CPU."""
    S = particles["S"]
    idx, Ts = IC.repose_case(S)
    scene_file = str(tmp_path / "particles.scene")
    RDC.write_scene_file(scene_file, S, idx, Ts)
    H.run_sanitized_main(tmp_path, "active_sanitized_main.cpp", args=[scene_file], expect="active_sanitized: ok (74 objects, 12 listed)")
