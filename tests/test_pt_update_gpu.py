"""GPU: srt_pt_update_mesh / srt_pt_update_mesh_device - new vertex arrays for one mesh of a committed scene, one BVH<Triangle>
rebuilt, the triangle records rewritten by a kernel.  After every update the context must compute, bit for bit, what the oracle
computes on scenes.with_vertices(S, ..) (the oracle knows nothing of updates) and dump the trees of a context freshly committed
on that description; only storage and counters differ."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _update_cases as UC
from _cases import particle_cloud, random_rays

pytestmark = pytest.mark.gpu

W = HT = 32
DEPTH, SPP, SEED = 5, 2, 9
INVALID, UNSUPPORTED = -1, -4


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def make_pt(srt, scene, use_bvh=True, builder=None, w=W, h=HT, depth=DEPTH):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, use_bvh)
    if builder is not None:
        pt.set_bvh_builder(*builder)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def every_sample(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32), ss.reshape(-1).astype(np.uint32)


def reference(scene, use_bvh=True, w=W, h=HT, depth=DEPTH):
    """What the oracle computes on a description (instances expanded): every sample, the epoch image, the hit records."""
    o = H.OraclePT(IC.expand(scene), w, h, depth, use_bvh)
    org, d, b = random_rays(3, 2048)
    return {"oracle": o, "samples": o.trace_samples(SEED, *every_sample(w, h, SPP)), "epoch": o.epoch(SEED, 0, SPP), "hits": o.hit(org, d, b)}


def check_against(pt, ref, modes, w=W, h=HT, hit_modes=(0, 5)):
    rgb, draws, rays = pt.trace_samples(SEED, *every_sample(w, h, SPP))
    want_rgb, want_draws, want_rays = ref["samples"]
    assert np.array_equal(draws, want_draws) and np.array_equal(rays, want_rays)
    assert bits_equal(rgb, want_rgb)
    org, d, b = random_rays(3, 2048)
    for mode in hit_modes:
        pt.set_kernel(mode)
        got = pt.hit(org, d, b)
        pt.set_kernel(0)
        assert bits_equal(got, ref["hits"]), f"hit under kernel mode {mode}"
    for mode in modes:
        pt.set_kernel(mode)
        got = pt.render_epoch(SEED, 0, SPP)
        pt.set_kernel(0)
        assert bits_equal(got, ref["epoch"]), f"kernel mode {mode}"


@pytest.fixture(scope="module")
def blob(scenes):
    """cbox+blob512, its three deformations, and the oracle's results on each description (computed once, left unchanged)."""
    S = UC.blob_scene()
    D = UC.deformations()
    refs = {"original": reference(S)}
    for name, (p, n) in D.items():
        refs[name] = reference(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n))
    return {"S": S, "D": D, "refs": refs}


@pytest.mark.parametrize("how", ["host_builder", "device_builder", "device_builder_device_arrays"])
def test_blob_deformations(srt, scenes, blob, how):
    """D1, D2, D3 in turn on one context.  device_builder: set_bvh_builder(True, 64) puts the 512-triangle mesh through the boxes
    kernel, the device builder's core and the record kernel; device_builder_device_arrays feeds them from a torch tensor."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    builder = (False,) if how == "host_builder" else (True, 64)
    pt = make_pt(srt, S, builder=builder)
    first = pt.render_epoch(SEED, 0, SPP)
    assert bits_equal(first, blob["refs"]["original"]["epoch"])
    keep = []

    def update(p, n):
        if how == "device_builder_device_arrays":
            import torch

            tp, tn = torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda()
            torch.cuda.synchronize()
            keep.extend([tp, tn])
            pt.update_mesh_device(UC.BLOB_OBJECT, tp.data_ptr(), tn.data_ptr(), len(p))
        else:
            pt.update_mesh(UC.BLOB_OBJECT, p, n)

    for name, (p, n) in blob["D"].items():
        before = pt.scene_counts()
        update(p, n)
        after = pt.scene_counts()
        assert after["blas_builds"] == before["blas_builds"] + 1, name
        assert after["triangles"] == before["triangles"] and after["objects"] == before["objects"], name
        assert after["uploaded_bytes"] - before["uploaded_bytes"] < after["device_bytes"], name
        check_against(pt, blob["refs"][name], (0, 2, 5, 6, 7))
        fresh = make_pt(srt, scenes.with_vertices(S, UC.BLOB_OBJECT, p, n), builder=builder)
        same = IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj))
        blob_nodes = fresh.scene_counts()["blas_nodes"]
        fresh.close()
        assert same, name
        assert after["blas_nodes"] == blob_nodes
    update(*UC.original(S, UC.BLOB_OBJECT))
    back = pt.render_epoch(SEED, 0, SPP)
    pt.close()
    assert bits_equal(back, first)


def upload_of_one_update(srt, scene, builder, p, n, device_arrays=False):
    """uploaded_bytes an update of object 6 adds on a fresh context under `builder`."""
    pt = make_pt(srt, scene, builder=builder)
    before = pt.scene_counts()["uploaded_bytes"]
    if device_arrays:
        import torch

        tp, tn = torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda()
        torch.cuda.synchronize()
        pt.update_mesh_device(UC.BLOB_OBJECT, tp.data_ptr(), tn.data_ptr(), len(p))
    else:
        pt.update_mesh(UC.BLOB_OBJECT, p, n)
    added = pt.scene_counts()["uploaded_bytes"] - before
    pt.close()
    return added


def test_device_path_is_taken(srt, blob):
    """Host and device build give the same arrays, so only the upload figure tells which one ran: an update whose tree the device
    core built (boxes kernel -> core -> record kernel) uploads everything a host-built one does EXCEPT the primitive order, 4 B
    per triangle, which is in the workspace already; the device form uploads no vertices (24 B each) either."""
    p, n = blob["D"]["D1"]
    ntri = len(p) // 3
    host = upload_of_one_update(srt, blob["S"], (False,), p, n)
    below = upload_of_one_update(srt, blob["S"], (True, 1024), p, n)          # device builder, mesh below its threshold: a host build
    device = upload_of_one_update(srt, blob["S"], (True, 64), p, n)
    arrays = upload_of_one_update(srt, blob["S"], (True, 64), p, n, device_arrays=True)
    assert below == host
    assert host - device == 4 * ntri
    assert host - arrays == 4 * ntri + 24 * len(p)


def test_sweeps_scene_source_and_instance(srt, scenes):
    """The source of sweeps_scene() updated: both objects on the shared range change.  Then the instance re-posed, then the source
    updated again."""
    S = IC.sweeps_scene()
    n_obj = len(S["objects"])
    pt = make_pt(srt, S)
    p2, n2 = UC.deformations()["D2"]
    pt.update_mesh(6, p2, n2)
    S2 = scenes.with_vertices(S, 6, p2, n2)
    check_against(pt, reference(S2), (0, 2, 5, 6, 7))
    T = IC.translate(S["objects"][n_obj - 1]["T"], (0.5, -0.25, 0.3))
    pt.repose([n_obj - 1], [T])
    p1, n1 = UC.deformations()["D1"]
    pt.update_mesh(6, p1, n1)
    S3 = IC.with_poses(scenes.with_vertices(S, 6, p1, n1), [n_obj - 1], [T])
    check_against(pt, reference(S3), (0, 2, 5, 6, 7))
    fresh = make_pt(srt, S3)
    same = IC.dumps_equal(IC.all_dumps(pt, n_obj), IC.all_dumps(fresh, n_obj))
    fresh.close(); pt.close()
    assert same


def test_particle_scene_source(srt, scenes):
    """74 objects (the streamed form): object 8, the source of 59 instances, gets new vertices."""
    S = IC.particles_shared()[0]
    src = IC.PARTICLE_FIRST
    p, n = UC.original(S, src)
    p2 = (p * np.array([1.4, 0.7, 1.1], np.float32) + np.array([0.01, 0.0, -0.02], np.float32)).astype(np.float32)
    S2 = scenes.with_vertices(S, src, p2, n)
    w, h, depth = 32, 24, 4
    pt = make_pt(srt, S, w=w, h=h, depth=depth)
    before = pt.render_epoch(SEED, 0, SPP)
    pt.update_mesh(src, p2, n)
    ref = reference(S2, w=w, h=h, depth=depth)
    assert pt.kernel_form() == 3
    assert not bits_equal(before, ref["epoch"])
    check_against(pt, ref, (0, 1, 4, 6), w=w, h=h, hit_modes=(0,))        # (the flattened walk of mode 5 holds at most 31 objects)
    fresh = make_pt(srt, S2, w=w, h=h, depth=depth)
    images = []
    for x in (pt, fresh):
        x.set_normal_colors(True)
        images.append(x.render_epoch(SEED, 0, SPP))
        x.set_normal_colors(False)
    same = IC.dumps_equal(IC.all_dumps(pt, 74), IC.all_dumps(fresh, 74))
    fresh.close()
    assert same and np.count_nonzero(images[0]) > 0 and bits_equal(images[0], images[1])
    pos, vel, age = particle_cloud(31, 512)
    got = pt.particles_step(pos, vel, age, 0.01, 0.015)
    want = ref["oracle"].particles_update(pos, vel, age, 0.01, 0.015)
    pt.close()
    assert all(bits_equal(x, y) for x, y in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])


def test_two_meshes(srt, scenes):
    """Two meshes with a BVH<Triangle> each, updated in turn: the updated range lies once in front of and once behind the other in
    storage; the other mesh's dump stays, and an update uploads less than the scene holds."""
    S = UC.two_mesh_scene()
    nobj = len(S["objects"])
    pt = make_pt(srt, S)
    d0 = IC.all_dumps(pt, nobj)
    slot = {i: [k for k in range(nobj) if d0[0][2][k] == i + 1][0] for i in (6, 8)}
    p6, n6 = UC.deformations()["D1"]
    p8, n8 = UC.small_blob_deformation()
    c0 = pt.scene_counts()
    pt.update_mesh(6, p6, n6)
    c1 = pt.scene_counts()
    d1 = IC.all_dumps(pt, nobj)
    S1 = scenes.with_vertices(S, 6, p6, n6)
    check_against(pt, reference(S1), (0, 6))
    pt.update_mesh(8, p8, n8)
    c2 = pt.scene_counts()
    S2 = scenes.with_vertices(S1, 8, p8, n8)
    check_against(pt, reference(S2), (0, 2, 5, 6, 7))
    fresh = make_pt(srt, S2)
    d2, df = IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj)
    fresh.close(); pt.close()
    assert IC.dumps_equal(d2, df)
    by_object = lambda d, i: d[1 + [k for k in range(nobj) if d[0][2][k] == i + 1][0]]
    assert IC.dumps_equal([by_object(d1, 8)], [d0[1 + slot[8]]]) and not IC.dumps_equal([by_object(d1, 6)], [d0[1 + slot[6]]])
    assert IC.dumps_equal([by_object(d2, 6)], [by_object(d1, 6)]) and not IC.dumps_equal([by_object(d2, 8)], [by_object(d1, 8)])
    for a, b in ((c0, c1), (c1, c2)):
        assert 0 < b["uploaded_bytes"] - a["uploaded_bytes"] < b["device_bytes"] and b["blas_builds"] == a["blas_builds"] + 1


def test_list_mode(srt, scenes):
    S = UC.blob_scene()
    p, n = UC.deformations()["D1"]
    pt = make_pt(srt, S, use_bvh=False)
    before = pt.scene_counts()
    pt.update_mesh(UC.BLOB_OBJECT, p, n)
    assert pt.scene_counts()["blas_builds"] == before["blas_builds"] == 0
    ref = reference(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n), use_bvh=False)
    rgb, draws, rays = pt.trace_samples(SEED, *every_sample(W, HT, SPP))
    got = pt.render_epoch(SEED, 0, SPP)
    org, d, b = random_rays(3, 2048)
    hits = pt.hit(org, d, b)
    pt.close()
    assert np.array_equal(draws, ref["samples"][1]) and np.array_equal(rays, ref["samples"][2]) and bits_equal(rgb, ref["samples"][0])
    assert bits_equal(got, ref["epoch"]) and bits_equal(hits, ref["hits"])


def test_default_builder_rule_above_the_threshold(srt, scenes):
    """cornell_with_mesh(6): 32 768 triangles, above the device builder's default threshold.  Dumps only, against a fresh commit."""
    S = scenes.cornell_with_mesh(6, "glass")
    p, n, i = UC.blob_arrays(6, seed=11)
    assert np.array_equal(i, S["objects"][6]["idx"])
    pt = make_pt(srt, S)
    before = pt.scene_counts()
    pt.update_mesh(6, p, n)
    after = pt.scene_counts()
    fresh = make_pt(srt, scenes.with_vertices(S, 6, p, n))
    same = IC.dumps_equal(IC.all_dumps(pt, 8), IC.all_dumps(fresh, 8))
    fresh.close(); pt.close()
    assert same and after["blas_builds"] == before["blas_builds"] + 1
    # 24 B per vertex went up, not 132 B per triangle
    assert after["uploaded_bytes"] - before["uploaded_bytes"] < 32768 * 132
    # and the tree came from the device core: no primitive order (4 B per triangle) went up, as it does after a host build
    assert upload_of_one_update(srt, S, (False,), p, n) - (after["uploaded_bytes"] - before["uploaded_bytes"]) == 4 * 32768


def test_refusals(srt, scenes):
    """Each refusal returns its status and the next render_epoch equals the one before, bit for bit."""
    lib = srt.load_library()
    S = IC.sweeps_scene()
    pt = make_pt(srt, S)
    pt.set_bvh_builder(False)
    image = pt.render_epoch(SEED, 0, SPP)
    counts = pt.scene_counts()
    p, n = UC.deformations()["D1"]
    lp, ln = UC.original(S, 7)
    for what, index, pp, nn, nverts in [("an area light", 7, lp, ln, len(lp)), ("an instance", 8, p, n, len(p)), ("another vertex count", 6, p, n, len(p) - 3)]:
        assert lib.srt_pt_update_mesh(pt._ctx, index, H.P(pp), H.P(nn), nverts) == INVALID, what
        assert bits_equal(pt.render_epoch(SEED, 0, SPP), image), what
    assert pt.scene_counts()["blas_builds"] == counts["blas_builds"]
    pt.close()
    S2, (cp, cn) = UC.flat_chain_scene()
    pt = make_pt(srt, S2, builder=(False,))
    image = pt.render_epoch(SEED, 0, SPP)
    assert lib.srt_pt_update_mesh(pt._ctx, 6, H.P(cp), H.P(cn), len(cp)) == UNSUPPORTED
    again = pt.render_epoch(SEED, 0, SPP)
    pt.close()
    assert bits_equal(again, image)


def test_group(srt, scenes, blob):
    S = blob["S"]
    p, n = blob["D"]["D2"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    first = grp.render_epoch(SEED, 0, SPP)
    grp.update_mesh(UC.BLOB_OBJECT, p, n)
    moved = grp.render_epoch(SEED, 0, SPP)
    counts = grp.scene_counts()
    grp.close()
    assert bits_equal(first, blob["refs"]["original"]["epoch"]) and bits_equal(moved, blob["refs"]["D2"]["epoch"])
    assert counts[0] == counts[1]
