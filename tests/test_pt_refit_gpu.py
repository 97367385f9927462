"""GPU: srt_pt_refit_mesh / srt_pt_refit_mesh_device / srt_pt_skin_pose_refit - new vertices for one mesh of a committed scene,
its BVH<Triangle> kept: the refit kernels (pt_mesh_update.hip) give every node its new box, no build runs.  A refitted scene is
not a fresh commit's (the oracle would walk another tree), so the expectation is the host refit walked by the device headers on
the CPU (tests/_refit_cases.py: EmuRefit), produced here at test time; tests/test_pt_refit_emu_host.py shows on the CPU that for
these seeds and deformations it equals the oracle on the new vertices sample for sample.  Everything is compared bit for bit."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _refit_cases as RC
import _skin_cases as SC
import _update_cases as UC
from _cases import particle_cloud, pt_scene, random_rays
from _refit_cases import DEPTH, HT, SEED, SPP, W, bits_equal

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
MODES = (0, 1, 2, 4, 5, 6, 7)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def make_pt(srt, scene, device=0, w=W, h=HT, depth=DEPTH, builder=None):
    pt = srt.Pathtracer(device)
    pt.set_params(w, h, 1, depth, True)
    if builder is not None:
        pt.set_bvh_builder(*builder)
    pt.build_scene(scene)
    if device >= 0:
        pt.set_camera(scene["camera"])
    return pt


def host_dumps(srt, scene, refits):
    """all_dumps of a host-only context after the refits: what srt_pt_dump_bvh must give on the device."""
    pt = make_pt(srt, scene, device=-1)
    for index, p, n in refits:
        pt.refit_mesh(index, p, n)
    d = IC.all_dumps(pt, len(scene["objects"]))
    pt.close()
    return d


def check_against(pt, want, modes=MODES, w=W, h=HT, spp=SPP, hit_modes=(0, 5)):
    rgb, draws, rays = pt.trace_samples(SEED, *RC.every_sample(w, h, spp))
    want_rgb, want_draws, want_rays = want["samples"]
    assert np.array_equal(draws, want_draws) and np.array_equal(rays, want_rays)        # RNG draw and ray ledgers
    assert bits_equal(rgb, want_rgb)
    org, d, b = random_rays(RC.RAY_SEED, RC.RAYS)
    for mode in hit_modes:
        pt.set_kernel(mode)
        got = pt.hit(org, d, b)
        pt.set_kernel(0)
        assert bits_equal(got, want["hits"][1 if mode == 5 else 0]), f"hit under kernel mode {mode}"
    for mode in modes:
        pt.set_kernel(mode)
        got = pt.render_epoch(SEED, 0, spp)
        pt.set_kernel(0)
        assert bits_equal(got, want["epoch"]), f"kernel mode {mode}"


@pytest.fixture(scope="module")
def blob(srt):
    """cbox+blob512, its three deformations, and per deformation the emulated expectation and the host-only context's dumps
    (computed once, left unchanged)."""
    S = UC.blob_scene()
    D = UC.deformations()
    want = {name: RC.expectation(S, [(UC.BLOB_OBJECT, p, n)], normals=(name == "D1")) for name, (p, n) in D.items()}
    dumps = {name: host_dumps(srt, S, [(UC.BLOB_OBJECT, p, n)]) for name, (p, n) in D.items()}
    return {"S": S, "D": D, "want": want, "dumps": dumps}


def test_blob_refits(srt, blob):
    """D1, D2, D3 in turn on one context, every kernel form after each: per-sample radiance, RNG draw and ray ledgers, hit records
    of both walks, the epoch image, the dumped trees; and no build, no upload of a triangle-class byte."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    pt = make_pt(srt, S)
    for name, (p, n) in blob["D"].items():
        before = pt.scene_counts()
        pt.refit_mesh(UC.BLOB_OBJECT, p, n)
        after = pt.scene_counts()
        assert after["refits"] == before["refits"] + 1 and after["blas_builds"] == before["blas_builds"], name
        assert after["uploaded_triangle_bytes"] == before["uploaded_triangle_bytes"], name
        assert {k: after[k] for k in ("objects", "triangles", "blas_nodes", "blas_records", "device_bytes")} == \
               {k: before[k] for k in ("objects", "triangles", "blas_nodes", "blas_records", "device_bytes")}, name
        check_against(pt, blob["want"][name])
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"][name]), name
    pt.close()


def test_first_refit_uploads_the_tables_once(srt, blob):
    """The first refit of a mesh sends its refit tables up (4 B per triangle of primitive order among them); the second sends
    only the vertices and the top half."""
    p, n = blob["D"]["D1"]
    pt = make_pt(srt, blob["S"])
    c0 = pt.scene_counts()
    pt.refit_mesh(UC.BLOB_OBJECT, p, n)
    c1 = pt.scene_counts()
    pt.refit_mesh(UC.BLOB_OBJECT, *blob["D"]["D2"])
    c2 = pt.scene_counts()
    pt.close()
    first, second = c1["uploaded_bytes"] - c0["uploaded_bytes"], c2["uploaded_bytes"] - c1["uploaded_bytes"]
    ntri, nodes, recs = len(p) // 3, UC.NODES["original"], c0["blas_records"]      # (the box's other meshes are root leaves: no records)
    tables = 4 * ntri + 8 * nodes + 8 * recs                                       # + 4 B per level offset
    assert tables < first - second < tables + 1024
    assert 24 * len(p) < second < 24 * len(p) + 8192                               # the vertices, the BVH<Object> and the tables of object order


def test_identity_refit(srt, blob):
    S, nobj = blob["S"], len(blob["S"]["objects"])
    pt = make_pt(srt, S)
    image, dumps = pt.render_epoch(SEED, 0, SPP), IC.all_dumps(pt, nobj)
    pt.refit_mesh(UC.BLOB_OBJECT, *UC.original(S, UC.BLOB_OBJECT))
    again, after = pt.render_epoch(SEED, 0, SPP), IC.all_dumps(pt, nobj)
    refits = pt.scene_counts()["refits"]
    pt.close()
    assert image.tobytes() == again.tobytes() and IC.dumps_equal(dumps, after) and refits == 1


def test_refit_mesh_device_from_a_tensor(srt, blob):
    import torch

    S, nobj = blob["S"], len(blob["S"]["objects"])
    pt = make_pt(srt, S)
    keep = []
    for name in ("D2", "D1"):
        p, n = blob["D"][name]
        tp, tn = torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda()
        torch.cuda.synchronize()
        keep.extend([tp, tn])
        before = pt.scene_counts()
        pt.refit_mesh_device(UC.BLOB_OBJECT, tp.data_ptr(), tn.data_ptr(), len(p))
        after = pt.scene_counts()
        assert after["blas_builds"] == before["blas_builds"] and after["uploaded_triangle_bytes"] == before["uploaded_triangle_bytes"]
        if name == "D1":                               # (the second refit: the tables are resident) no vertex goes up, 24 B each
            assert after["uploaded_bytes"] - before["uploaded_bytes"] < 8192
        check_against(pt, blob["want"][name], modes=(0, 6))
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"][name]), name
    pt.close()


def test_skin_pose_refit(srt, blob):
    """skin_blob_chain3's poses through Skin.pose_refit against refit_mesh of the arrays the reference skinned (the fixture's), on
    a second context; the first pose also against the emulated expectation."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    g, joints = SC.load_fixture("blob_chain3")
    assert bits_equal(g["pos"], UC.original(S, UC.BLOB_OBJECT)[0])
    pt, other = make_pt(srt, S), make_pt(srt, S)
    skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints)
    for k, posed in enumerate(g["posed"]):
        flat = k == 1
        p, n = (g["flat_pos"][k], g["flat_nrm"][k]) if flat else (g["smooth_pos"][k], g["smooth_nrm"][k])
        before = pt.scene_counts()
        skin.pose_refit(posed, flat_normals=flat)
        after = pt.scene_counts()
        assert after["blas_builds"] == before["blas_builds"] and after["refits"] == before["refits"] + 1
        other.refit_mesh(UC.BLOB_OBJECT, p, n)
        a, b = pt.trace_samples(SEED, *RC.every_sample(W, HT, SPP)), other.trace_samples(SEED, *RC.every_sample(W, HT, SPP))
        assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert bits_equal(pt.render_epoch(SEED, 0, SPP), other.render_epoch(SEED, 0, SPP))
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(other, nobj)), k
        if k == 0:
            check_against(pt, RC.expectation(S, [(UC.BLOB_OBJECT, p, n)]), modes=(0, 6))
    # a skin made before a refit stays valid, and an update after refits rebuilds
    skin.pose(g["posed"][0])
    assert pt.scene_counts()["blas_builds"] == after["blas_builds"] + 1
    skin.close(); pt.close(); other.close()


def two_meshes_and_an_instance():
    """two_mesh_scene() plus an instance of the blob (object 6) and one of the small blob (object 8): objects 9 and 10."""
    S = UC.two_mesh_scene()
    S["objects"].append(dict(IC.sweeps_scene()["objects"][-1]))
    T = IC.translate(S["objects"][8]["T"], (0.45, -0.3, 0.25))
    S["objects"].append({"kind": "instance", "of": 8, "T": T, "material": 5})
    return S


def test_two_meshes_with_instances(srt):
    """Each mesh refitted in turn: zero builds, zero uploads of triangle-class bytes (the other mesh's records included), the other
    mesh's dump untouched, and the instances follow their sources."""
    S = two_meshes_and_an_instance()
    nobj = len(S["objects"])
    pt = make_pt(srt, S)
    d0 = IC.all_dumps(pt, nobj)
    slot = {i: RC.slot_of(d0[0], i, nobj) for i in (6, 8, 9, 10)}
    p6, n6 = UC.deformations()["D2"]
    p8, n8 = UC.small_blob_deformation()
    c0 = pt.scene_counts()
    pt.refit_mesh(6, p6, n6)
    c1 = pt.scene_counts()
    d1 = IC.all_dumps(pt, nobj)
    by = lambda d, i: d[1 + RC.slot_of(d[0], i, nobj)]
    assert IC.dumps_equal([by(d1, 8)], [d0[1 + slot[8]]]) and not IC.dumps_equal([by(d1, 6)], [d0[1 + slot[6]]])
    assert IC.dumps_equal([by(d1, 9)], [by(d1, 6)]) and IC.dumps_equal([by(d1, 10)], [by(d1, 8)])
    check_against(pt, RC.expectation(S, [(6, p6, n6)]), modes=(0, 2, 6))
    pt.refit_mesh(8, p8, n8)
    c2 = pt.scene_counts()
    check_against(pt, RC.expectation(S, [(6, p6, n6), (8, p8, n8)]))
    d2 = IC.all_dumps(pt, nobj)
    pt.close()
    assert IC.dumps_equal(d2, host_dumps(srt, S, [(6, p6, n6), (8, p8, n8)]))
    assert IC.dumps_equal([by(d2, 6)], [by(d1, 6)]) and IC.dumps_equal([by(d2, 10)], [by(d2, 8)])
    for a, b in ((c0, c1), (c1, c2)):
        assert b["blas_builds"] == a["blas_builds"] and b["uploaded_triangle_bytes"] == a["uploaded_triangle_bytes"]
        assert 0 < b["uploaded_bytes"] - a["uploaded_bytes"] < b["device_bytes"] and b["refits"] == a["refits"] + 1


@pytest.mark.parametrize("plan", ["shared_launches", "launch_per_level"])
def test_deep_tree(srt, monkeypatch, plan):
    """deep_both: the chain's BVH<Triangle> nests 48 interior nodes under a BVH<Object> nesting 24 - every level of the refit's
    level loop holds one node.  Its vertices move by a seeded small offset.  Under both launch plans: one workgroup walking all
    48 levels, and SRT_REFIT_LEVEL_LAUNCHES=1 (read when a mesh's refit tables are made), 48 launches of one lane."""
    if plan == "launch_per_level":
        monkeypatch.setenv("SRT_REFIT_LEVEL_LAUNCHES", "1")
    D = pt_scene("deep_both")
    w, h, depth, spp = RC.DEEP
    p, n = RC.deep_moved(D)
    want = RC.expectation(D, [(RC.DEEP_MESH, p, n)], w, h, depth, spp)
    pt = make_pt(srt, D, w=w, h=h, depth=depth)
    before = IC.all_dumps(pt, len(D["objects"]))
    pt.refit_mesh(RC.DEEP_MESH, p, n)
    check_against(pt, want, modes=(0, 1, 4, 6), w=w, h=h, spp=spp)
    got = IC.all_dumps(pt, len(D["objects"]))
    pt.close()
    assert IC.dumps_equal(got, host_dumps(srt, D, [(RC.DEEP_MESH, p, n)])) and not IC.dumps_equal(got, before)


def test_levels_beyond_one_workgroup(srt, scenes):
    """cornell_with_mesh(5): 8 192 triangles, whose tree has levels of more than 256 interior nodes (one multi-block launch each)
    between runs of smaller ones (shared launches): every node box against the host refit's, and the image against the emulation."""
    S = scenes.cornell_with_mesh(5, "glass")
    p, n, i = UC.blob_arrays(5, seed=11)
    assert np.array_equal(i, S["objects"][6]["idx"])
    host = make_pt(srt, S, device=-1)
    links = host.dump_bvh(RC.slot_of(host, 6, 8))[1]
    host.refit_mesh(6, p, n)
    want_dumps = IC.all_dumps(host, 8)
    host.close()
    level = np.zeros(len(links), np.int64)
    for k, (_, _, l, r) in enumerate(links):
        if l != r:
            level[l] = level[r] = level[k] + 1
    per_level = np.bincount(level[links[:, 2] != links[:, 3]])
    assert per_level.max() > 256 and per_level[0] == 1 and per_level[-1] <= 256
    pt = make_pt(srt, S)
    before = pt.scene_counts()
    pt.refit_mesh(6, p, n)
    after = pt.scene_counts()
    got = IC.all_dumps(pt, 8)
    image = pt.render_epoch(SEED, 0, SPP)
    pt.close()
    assert IC.dumps_equal(got, want_dumps)
    assert after["blas_builds"] == before["blas_builds"] and after["uploaded_triangle_bytes"] == before["uploaded_triangle_bytes"]
    assert bits_equal(image, RC.expectation(S, [(6, p, n)])["epoch"])


def test_refit_then_update_equals_a_fresh_commit(srt, scenes, blob):
    S, nobj = blob["S"], len(blob["S"]["objects"])
    (p1, n1), (p2, n2) = blob["D"]["D1"], blob["D"]["D2"]
    pt = make_pt(srt, S)
    pt.refit_mesh(UC.BLOB_OBJECT, p1, n1)
    pt.update_mesh(UC.BLOB_OBJECT, p2, n2)
    desc = scenes.with_vertices(S, UC.BLOB_OBJECT, p2, n2)
    fresh = make_pt(srt, desc)
    same = IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj))
    o = H.OraclePT(desc, W, HT, DEPTH, True)
    org, d, b = random_rays(RC.RAY_SEED, RC.RAYS)
    hits = o.hit(org, d, b)
    check_against(pt, {"samples": o.trace_samples(SEED, *RC.every_sample(W, HT, SPP)), "epoch": o.epoch(SEED, 0, SPP), "hits": (hits, hits)}, modes=(0, 2, 5, 6, 7))
    # and a refit after the rebuild works from the new tree (its tables were dropped with the old one)
    pt.refit_mesh(UC.BLOB_OBJECT, p1, n1)
    ok = IC.dumps_equal(IC.all_dumps(pt, nobj), host_dumps_after_update(srt, S, (p2, n2), (p1, n1)))
    fresh.close(); pt.close()
    assert same and ok


def host_dumps_after_update(srt, scene, updated, refitted):
    pt = make_pt(srt, scene, device=-1)
    pt.update_mesh(UC.BLOB_OBJECT, *updated)
    pt.refit_mesh(UC.BLOB_OBJECT, *refitted)
    d = IC.all_dumps(pt, len(scene["objects"]))
    pt.close()
    return d


def test_refusals(srt):
    """Each refusal returns its status and the next render_epoch equals the one before, byte for byte."""
    import torch

    lib = srt.load_library()
    S = IC.sweeps_scene()
    pt = make_pt(srt, S)
    image = pt.render_epoch(SEED, 0, SPP)
    counts = pt.scene_counts()
    p, n = UC.deformations()["D1"]
    lp, ln = UC.original(S, 7)
    nan, inf = p.copy(), p.copy()
    nan[100, 2], inf[7, 0] = np.nan, -np.inf
    cases = [("an area light", 7, lp, ln, len(lp)), ("an instance", 8, p, n, len(p)), ("another vertex count", 6, p, n, len(p) - 3), ("a sphere", 5, p, n, len(p)),
             ("out of range", len(S["objects"]), p, n, len(p)), ("a NaN", 6, nan, n, len(p)), ("an Inf", 6, inf, n, len(p))]
    for what, index, pp, nn, nverts in cases:
        assert lib.srt_pt_refit_mesh(pt._ctx, index, H.P(pp), H.P(nn), nverts) == INVALID, what
        assert pt.render_epoch(SEED, 0, SPP).tobytes() == image.tobytes(), what
        assert pt.scene_counts() == counts, what                      # every count, the upload figures included
    # the device form meets the NaN only in its copy-back, after its kernels have run - into arrays of their own
    tp, tn = torch.from_numpy(nan).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(srt.SrtError, match="non-finite") as e:
        pt.refit_mesh_device(6, tp.data_ptr(), tn.data_ptr(), len(p))
    assert e.value.status == INVALID and pt.render_epoch(SEED, 0, SPP).tobytes() == image.tobytes()
    assert pt.scene_counts() == counts
    # .. and a good refit afterwards is not disturbed by the refused ones
    pt.refit_mesh(6, p, n)
    want = RC.expectation(S, [(6, p, n)])
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), want["epoch"])
    pt.close()


def test_group(srt, blob):
    S = blob["S"]
    p, n = blob["D"]["D2"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    grp.refit_mesh(UC.BLOB_OBJECT, p, n)
    moved = grp.render_epoch(SEED, 0, SPP)
    counts = grp.scene_counts()
    grp.close()
    single = make_pt(srt, S)
    single.refit_mesh(UC.BLOB_OBJECT, p, n)
    image = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert bits_equal(moved, image) and bits_equal(moved, blob["want"]["D2"]["epoch"])
    assert counts[0] == counts[1] and counts[0]["refits"] == 1


def test_particles_and_normal_colors_after_a_refit(srt, scenes, blob):
    """The two other users of the scene's arrays.  The normal-colors view against the emulated refitted scene.  Scene_Particles' step
    (scene.hit per leg) against the oracle on the new vertices, which walks the rebuilt tree: that the refitted tree gives the same
    hits on these legs is not shown elsewhere - it is what this comparison itself establishes (a leg that grazed a box of one tree
    only could differ; none of these does)."""
    S = blob["S"]
    p, n = blob["D"]["D1"]
    pt = make_pt(srt, S)
    pt.refit_mesh(UC.BLOB_OBJECT, p, n)
    pt.set_normal_colors(True)
    rgb, draws, rays = pt.trace_samples(SEED, *RC.every_sample(W, HT, SPP))
    image = pt.render_epoch(SEED, 0, SPP)
    pt.set_normal_colors(False)
    want = blob["want"]["D1"]["normals"]
    assert bits_equal(rgb, want[0]) and np.array_equal(draws, want[1]) and np.array_equal(rays, want[2])
    assert np.count_nonzero(image) > 0 and bits_equal(image, RC.epoch_of(want[0], W, HT, SPP))
    pos, vel, age = particle_cloud(31, 512)
    got = pt.particles_step(pos, vel, age, 0.01, 0.015)
    o = H.OraclePT(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n), W, HT, DEPTH, True)
    expect = o.particles_update(pos, vel, age, 0.01, 0.015)
    pt.close()
    assert all(bits_equal(x, y) for x, y in zip(got[:3], expect[:3])) and np.array_equal(got[3], expect[3])
