"""CPU: what a refitted scene computes.  The scene layer's refit (pt_scene.cpp) walked by the device traversal headers compiled
for the host (tests/host_emu/refit_flat_host.cpp: the nested walk, the flattened walk and path_sample, one lane at a time) - the
expectation tests/test_pt_refit_gpu.py holds the GPU to, produced at test time.

The oracle only builds: on scenes.with_vertices(S, ..) it walks the tree a fresh build gives, not the refitted one.  Both trees
bound the same triangles with exact boxes, so the two may differ only on a ray that grazes a box of one of them.  For the seeds
and deformations below they agree on every ray and every sample: the number of exceptions is zero, and asserted so."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _refit_cases as RC
import _update_cases as UC
from _cases import random_rays


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def oracle_results(scene, normals=False):
    o = H.OraclePT(IC.expand(scene), RC.W, RC.HT, RC.DEPTH, True)
    org, d, b = random_rays(RC.RAY_SEED, RC.RAYS)
    return {"samples": o.trace_samples(RC.SEED, *RC.every_sample(RC.W, RC.HT, RC.SPP)), "epoch": o.epoch(RC.SEED, 0, RC.SPP), "hits": o.hit(org, d, b)}


def assert_same(e, want, what):
    assert np.array_equal(e["samples"][1], want["samples"][1]) and np.array_equal(e["samples"][2], want["samples"][2]), what    # RNG draws, rays
    assert RC.bits_equal(e["samples"][0], want["samples"][0]), what
    assert RC.bits_equal(e["epoch"], want["epoch"]), what               # (and _refit_cases.epoch_of folds samples as do_trace does)
    assert RC.bits_equal(e["hits"][0], want["hits"]) and RC.bits_equal(e["hits"][1], want["hits"]), what      # nested and flattened walk


def test_unrefitted_scene_is_the_oracles():
    """The driver itself: without a refit it computes what the oracle computes."""
    S = UC.blob_scene()
    assert_same(RC.expectation(S, []), oracle_results(S), "blob scene as committed")


@pytest.mark.parametrize("name", ["D1", "D2", "D3"])
def test_refitted_blob_against_the_oracle_on_the_new_vertices(scenes, name):
    S = UC.blob_scene()
    p, n = UC.deformations()[name]
    e = RC.expectation(S, [(UC.BLOB_OBJECT, p, n)])
    assert_same(e, oracle_results(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n)), name)
    assert np.count_nonzero(e["hits"][0][:, 0]) > 500


def test_refits_in_sequence_and_with_an_instance(scenes):
    """D1 then D2 on the scene with an instance of the blob: only the last vertices count, and the instance follows."""
    S = IC.sweeps_scene()
    (p1, n1), (p2, n2) = UC.deformations()["D1"], UC.deformations()["D2"]
    e = RC.expectation(S, [(6, p1, n1), (6, p2, n2)])
    assert_same(e, oracle_results(scenes.with_vertices(S, 6, p2, n2)), "D1, D2")
    again = RC.expectation(S, [(6, p2, n2)])
    assert RC.bits_equal(e["samples"][0], again["samples"][0]) and RC.bits_equal(e["hits"][0], again["hits"][0])


def test_deep_tree_with_delta_and_environment_lights(scenes):
    """deep_both (a BVH<Object> nesting 24, a BVH<Triangle> nesting 48, a point light, an environment light): the driver's light
    feeding against the oracle, then the chain's vertices moved by RC.deep_offset() - the oracle still commits those."""
    from _cases import pt_scene

    D = pt_scene("deep_both")
    w, h, depth, spp = RC.DEEP
    for refits, desc in (([], D), ([(RC.DEEP_MESH, *RC.deep_moved(D))], scenes.with_vertices(D, RC.DEEP_MESH, *RC.deep_moved(D)))):
        e = RC.expectation(D, refits, w, h, depth, spp)
        o = H.OraclePT(desc, w, h, depth, True)
        org, d, b = random_rays(RC.RAY_SEED, RC.RAYS)
        want = {"samples": o.trace_samples(RC.SEED, *RC.every_sample(w, h, spp)), "epoch": o.epoch(RC.SEED, 0, spp), "hits": o.hit(org, d, b)}
        assert_same(e, want, "deep_both" + (" refitted" if refits else ""))


def test_refused_refit_changes_nothing():
    S = UC.blob_scene()
    e = RC.EmuRefit(S)
    org, d, b = random_rays(RC.RAY_SEED, RC.RAYS)
    before = e.hit9(org, d, b)
    p, n = UC.deformations()["D1"]
    q = p.copy()
    q[5, 0] = np.nan
    assert e.refit(UC.BLOB_OBJECT, q, n) == 1 and e.refit(5, p, n) == 1 and e.refit(UC.BLOB_OBJECT, p[:-3], n[:-3]) == 1
    after = e.hit9(org, d, b)
    e.close()
    assert RC.bits_equal(before[0], after[0]) and RC.bits_equal(before[1], after[1])
