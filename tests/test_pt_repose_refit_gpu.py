"""GPU: srt_pt_repose_refit / srt_pt_repose_refit_device - new poses with the BVH<Object> kept: same links and object order, new
boxes, written by kernels that are only enqueued.  A refitted scene is not a fresh commit's (the oracle would walk another tree),
so the expectation is the host definition walked by the device headers on the CPU (tests/_repose_refit_cases.py: EmuTop),
produced here at test time; wherever a refit and a build must agree the other side is srt_pt_repose / a fresh commit.  Everything
is compared bit for bit.  Device arrays are torch tensors passed by data_ptr()."""
import re

import numpy as np
import pytest

import _instance_cases as IC
import _light_cases as LC
import _repose_device_cases as RDC
import _repose_refit_cases as C
import _skin_cases as SC
import _update_cases as UC
from _cases import random_rays
from _refit_cases import tree_cost_numpy
from _repose_refit_cases import DEPTH, HT, SEED, SPP, W, bits_equal

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -5, -4


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make_pt(srt, scene, device=0, w=W, h=HT, depth=DEPTH, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(device)
    pt.set_params(w, h, 1, depth, use_bvh)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    if device >= 0:
        pt.set_camera(scene["camera"])
    return pt


def on_device(torch, Ts):
    return torch.from_numpy(np.ascontiguousarray(Ts, np.float32).reshape(-1, 16)).to("cuda:0")


def device_refit(torch, pt, idx, Ts, stream=0):
    """The device form from a fresh tensor; the tensor is returned so that it lives until the caller has waited."""
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    pt.repose_refit_device(idx, d.data_ptr(), stream)
    return d


def top_dump(pt, nobj):
    boxes, links, order = pt.dump_bvh(-1, cap=2 * nobj + 2)
    return boxes, links, order[:nobj]


def top_equal(a, b, nan=False):
    return (C.bits_equal_nan if nan else bits_equal)(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check_against(pt, want, modes, w=W, h=HT, spp=SPP, hit_modes=(0,)):
    """Every sample with its RNG draw and ray ledgers, the hit records of the walks, the epoch image per kernel mode."""
    rgb, draws, rays = pt.trace_samples(SEED, *C.every_sample(w, h, spp))
    assert np.array_equal(draws, want["samples"][1]) and np.array_equal(rays, want["samples"][2])
    assert bits_equal(rgb, want["samples"][0])
    check_hits(pt, want, hit_modes)
    for mode in modes:
        pt.set_kernel(mode)
        got = pt.render_epoch(SEED, 0, spp)
        pt.set_kernel(0)
        assert bits_equal(got, want["epoch"]), f"kernel mode {mode}"


def check_hits(pt, want, hit_modes=(0,)):
    org, d, b = random_rays(C.RAY_SEED, C.RAYS)
    for mode in hit_modes:
        pt.set_kernel(mode)
        got = pt.hit(org, d, b)
        pt.set_kernel(0)
        assert bits_equal(got, want["hits"][1 if mode == 5 else 0]), f"hit under kernel mode {mode}"


@pytest.fixture(scope="module")
def particles():
    """The 74-object particle scene, repose_case's list, and the emulated expectation after a refit of it (computed once)."""
    S = IC.particles_shared()[0]
    idx, Ts = IC.repose_case(S)
    return {"S": S, "idx": idx, "Ts": Ts, "home": np.array([S["objects"][i]["T"] for i in idx], np.float32), "want": C.expectation(S, [(idx, Ts)])}


def test_sweeps_scene(srt, torch):
    """At most 16 objects: the wave-uniform kernel, which reads the sweep records, the inline walks (2) and the flattened walk (5).
    The rotated, non-uniformly scaled instance and one wall; then srt_pt_repose_device of the same poses: a fresh commit."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    idx, Ts = C.sweeps_case(S)
    want = C.expectation(S, [(idx, Ts)])
    pt = make_pt(srt, S)
    pt.set_kernel(2)
    assert pt.kernel_form() in (0, 1)                       # the persistent sweeps: they read the sweep records
    pt.set_kernel(0)
    first = top_dump(pt, nobj)
    keep = device_refit(torch, pt, idx, Ts)
    check_against(pt, want, modes=(0, 2, 5, 7), hit_modes=(0, 5))
    got = top_dump(pt, nobj)
    assert top_equal(got, want["dump"]) and np.array_equal(got[1], first[1]) and np.array_equal(got[2], first[2]) and not bits_equal(got[0], first[0])
    assert pt.top_refit_count() == 1
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    pt.repose_device(idx, d.data_ptr())
    fresh = make_pt(srt, IC.with_poses(S, idx, Ts))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(fresh, nobj))
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), fresh.render_epoch(SEED, 0, SPP))
    org, dd, b = random_rays(C.RAY_SEED, C.RAYS)
    assert bits_equal(pt.hit(org, dd, b), fresh.hit(org, dd, b))
    # and the host form on the device context: the same scene as the device form's
    host = make_pt(srt, S)
    host.repose_refit(idx, Ts)
    check_against(host, want, modes=(0,), hit_modes=(0, 5))
    assert top_equal(top_dump(host, nobj), want["dump"])
    for p in (pt, fresh, host):
        p.close()
    del keep


def test_particles(srt, torch, particles):
    """68+ objects: the streamed form (auto, 6) and the lane-per-pixel kernel (1), which reads the top-level Node boxes.  Every
    sample, the epoch image and the hit walk equal the emulation; links and order stay and the boxes are the numpy folds."""
    S, idx, Ts, want = particles["S"], particles["idx"], particles["Ts"], particles["want"]
    nobj = len(S["objects"])
    pt = make_pt(srt, S)
    assert pt.kernel_form() in (3, 4)
    first = IC.all_dumps(pt, nobj)
    keep = device_refit(torch, pt, idx, Ts)
    # (the nested hit walk only: the flattened walk of mode 5 holds at most 31 objects and cannot run on this scene - both walks are
    #  compared on the sweeps scene)
    check_against(pt, want, modes=(0, 1, 6))
    moved = IC.all_dumps(pt, nobj)
    boxes, links, order = moved[0]
    assert np.array_equal(links, first[0][1]) and np.array_equal(order[:nobj], first[0][2][:nobj]) and IC.dumps_equal(moved[1:], first[1:])
    assert bits_equal(boxes, C.expected_top_boxes(S, idx, Ts, links, order[:nobj])) and bits_equal(boxes, want["dump"][0])
    # home again through the device form: the committed scene, as values
    keep2 = device_refit(torch, pt, idx, particles["home"])
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and pt.top_refit_count() == 2
    pt.close()
    del keep, keep2


@pytest.mark.parametrize("level_launches", ["0", "1"])
def test_pool_of_1200(srt, torch, monkeypatch, level_launches):
    """1200 instances of a 12-triangle mesh: levels of more than 256 interior nodes (refit_level_kernel) above and below runs of
    small levels (the shared-workgroup launch); with SRT_REFIT_LEVEL_LAUNCHES=1 one launch per level.  Hits and the tree only."""
    monkeypatch.setenv("SRT_REFIT_LEVEL_LAUNCHES", level_launches)
    S = C.pool_scene()
    nobj = len(S["objects"])
    idx, Ts = C.scatter(S, np.arange(0, nobj, 3, dtype=np.uint32), seed=3, spread=0.2)
    want = C.expectation(S, [(idx, Ts)], samples=False)
    assert C.widest_level(want["dump"][1]) > 256
    pt = make_pt(srt, S)
    first = top_dump(pt, nobj)
    keep = device_refit(torch, pt, idx, Ts)
    check_hits(pt, want)
    got = top_dump(pt, nobj)
    pt.close()
    del keep
    assert np.count_nonzero(want["hits"][0][:, 0]) > 100
    assert top_equal(got, want["dump"]) and np.array_equal(got[1], first[1]) and not bits_equal(got[0], first[0])


def test_scattered_particles_hit_what_the_oracle_hits(srt, torch, particles):
    """The poses of C.POSE_SEED, for which tests/test_pt_repose_refit_host.py shows that the emulation's closest hits equal the
    oracle's on a fresh commit on every one of the 2048 rays: the GPU's hit records after the device-form refit equal the
    emulation's bit for bit, and so differ from a fresh commit's (here: srt_pt_repose of the same poses on a second context) on
    at most C.TIES_CAP = 0 rays."""
    S = particles["S"]
    idx, Ts = C.scatter(S, C.particle_indices())
    want = C.expectation(S, [(idx, Ts)], samples=False)
    pt, rebuilt = make_pt(srt, S), make_pt(srt, S)
    keep = device_refit(torch, pt, idx, Ts)
    check_hits(pt, want)
    rebuilt.repose(idx, Ts)
    org, d, b = random_rays(C.RAY_SEED, C.RAYS)
    a, r = pt.hit(org, d, b), rebuilt.hit(org, d, b)
    differ = int(np.sum(np.any(a.view(np.uint32) != r.view(np.uint32), axis=1)))
    print(f"{differ} of {C.RAYS} rays differ between the refitted and the rebuilt tree (seed {C.POSE_SEED})")
    pt.close(); rebuilt.close()
    del keep
    assert differ <= C.TIES_CAP == 0 and np.count_nonzero(r[:, 0]) > 500


def test_pending_state_stays_bounded(srt, torch, particles):
    """A loop that never settles: 200 device-form calls, alternating between two lists that overlap.  What the context keeps is a
    set - at most one entry per listed object - and a count of calls; one settle then applies all of it."""
    S = particles["S"]
    nobj = len(S["objects"])
    pidx = C.particle_indices()
    lists = (pidx[:40], pidx[20:])
    Ts = [C.scatter(S, l, seed=21 + k)[1] for k, l in enumerate(lists)]
    d = [on_device(torch, T) for T in Ts]
    torch.cuda.synchronize()
    pt, ref = make_pt(srt, S), make_pt(srt, S, device=-1)
    assert pt.top_refit_pending() == (0, 0)
    pt.repose_refit_device(lists[0], d[0].data_ptr())
    pt.repose_refit_device(lists[0], d[0].data_ptr())
    assert pt.top_refit_pending() == (2, 40)              # the same list again adds nothing
    for k in range(198):
        pt.repose_refit_device(lists[k % 2], d[k % 2].data_ptr())
    assert pt.top_refit_pending() == (200, len(pidx))
    ref.repose_refit(lists[0], Ts[0])
    ref.repose_refit(lists[1], Ts[1])                     # the last call of each list decides: list 0's, then list 1's on top
    got, want = top_dump(pt, nobj), top_dump(ref, nobj)
    assert pt.top_refit_pending() == (0, 0) and pt.top_refit_count() == 200
    assert top_equal(got, want) and IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(ref, nobj))
    pt.close(); ref.close()


def test_one_object_a_list_scene_and_an_identity(srt, torch, particles):
    one = C.one_object_scene()
    T = IC.translate(one["objects"][0]["T"], (0.1, 0.2, -0.1))
    want = C.expectation(one, [([0], [T])], samples=False)
    pt = make_pt(srt, one)
    keep = device_refit(torch, pt, [0], [T])
    check_hits(pt, want)
    assert top_equal(top_dump(pt, 1), want["dump"]) and len(want["dump"][1]) == 1
    pt.close()
    # a list scene: the records alone; the image does not depend on how the objects are searched
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    ref, dev = make_pt(srt, S, use_bvh=False), make_pt(srt, S, use_bvh=False)
    org, d, b = random_rays(C.RAY_SEED, C.RAYS)
    before = dev.hit(org, d, b)
    ref.repose(idx, Ts)
    keep2 = device_refit(torch, dev, idx, Ts)
    got, ref_hits = dev.hit(org, d, b), ref.hit(org, d, b)
    assert bits_equal(got, ref_hits) and not bits_equal(got, before)
    assert bits_equal(dev.render_epoch(SEED, 0, SPP), particles["want"]["epoch"])
    ref.close(); dev.close()
    # an identity with -0 off the diagonal (has_trans becomes 0) and a pure translation
    ident = RDC.identity()
    ident[[1, 2, 4, 6, 8, 9, 12, 13, 14]] = np.float32(-0.0)
    a = IC.PARTICLE_FIRST + IC.PARTICLE_COUNT
    pair, Tp = [a, a + 1], np.stack([ident, RDC.translate_scale((0.2, 0.35, -0.1), 1.0)])
    want = C.expectation(S, [(pair, Tp)], samples=False)
    pt = make_pt(srt, S)
    keep3 = device_refit(torch, pt, pair, Tp)
    check_hits(pt, want)
    assert top_equal(top_dump(pt, len(S["objects"])), want["dump"])
    pt.close()
    del keep, keep2, keep3


def test_hostile_matrices(srt, torch, particles):
    """-0, denormals, singular matrices and a NaN: the device form equals the host-only context's host form on the tree and the
    device context's host form on hits, NaNs compared as NaNs."""
    S = particles["S"]
    nobj = len(S["objects"])
    pidx = C.particle_indices()
    org, d, b = random_rays(C.RAY_SEED, 512)
    dev, host = make_pt(srt, S), make_pt(srt, S)
    only = make_pt(srt, S, device=-1)
    keep = []
    for name, M in RDC.matrix_cases().items():
        M = M[:len(pidx)]
        idx = pidx[:len(M)]
        keep.append(device_refit(torch, dev, idx, M))
        host.repose_refit(idx, M)
        only.repose_refit(idx, M)
        assert top_equal(top_dump(dev, nobj), top_dump(only, nobj), nan=True), name
        assert C.bits_equal_nan(dev.hit(org, d, b), host.hit(org, d, b)), name
    for p in (dev, host, only):
        p.close()


def test_dynamic_lights(srt, torch):
    """With the switch on, a reposed emissive quad and an emissive sphere: the device's light tables equal the host-only context's
    after repose_refit, and the samples equal the host form's; with it off, the refusal text is srt_pt_repose's."""
    S = LC.three_light_scene()
    idx = np.array([LC.CBOX_LIGHT, 9, 5], np.uint32)
    Ts = np.array([LC.poses(S["objects"][int(i)]["T"])["rotation * scale"] for i in idx], np.float32)
    only = make_pt(srt, S, device=-1, dynamic=True)
    only.repose_refit(idx, Ts)
    want_lights = only.dump_lights()
    only.close()
    dev, host = make_pt(srt, S, dynamic=True), make_pt(srt, S, dynamic=True)
    first = dev.dump_lights(from_device=True)
    keep = device_refit(torch, dev, idx, Ts)
    host.repose_refit(idx, Ts)
    assert LC.lights_equal(dev.dump_lights(from_device=True), want_lights) and LC.lights_equal(dev.dump_lights(), want_lights)
    assert LC.lights_equal(host.dump_lights(from_device=True), want_lights) and not LC.lights_equal(first, want_lights)
    xs, ys, ss = C.every_sample(W, HT, 2)
    a, b = dev.trace_samples(SEED, xs, ys, ss), host.trace_samples(SEED, xs, ys, ss)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert bits_equal(dev.render_epoch(SEED, 0, 2), host.render_epoch(SEED, 0, 2))
    dev.close(); host.close()
    off = make_pt(srt, S)
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    texts = []
    for call in (lambda: off.repose(idx, Ts), lambda: off.repose_refit(idx, Ts), lambda: off.repose_refit_device(idx, d.data_ptr())):
        with pytest.raises(srt.SrtError, match="area light") as e:
            call()
        assert e.value.status == INVALID
        texts.append(re.split(r"srt_pt_\w+: ", str(e.value), 1)[1])
    off.close()
    assert texts[0] == texts[1] == texts[2]
    del keep


def test_enqueue_only(srt, torch, particles):
    """On a side stream: a kernel that writes the transforms, repose_refit_device and render_epoch_device with no host wait in
    between - the image is the expectation's.  A second call with the same list uploads nothing, a new list 4 B per listed object;
    three calls before one dump cost one settle and count three."""
    S, idx, Ts, want = particles["S"], particles["idx"], particles["Ts"], particles["want"]
    nobj = len(S["objects"])
    pt = make_pt(srt, S)
    local_tiles, _, floats_per_tile = pt.tile_info()
    half = on_device(torch, Ts * np.float32(0.5))
    tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
    image = torch.zeros(HT * W * 3, device="cuda:0")
    busy = torch.ones((1024, 1024), device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        for _ in range(4):
            busy = busy @ busy * 1e-3
        d = half + half                                   # exact: Ts again, written by a kernel on the stream
        pt.repose_refit_device(idx, d.data_ptr(), st.cuda_stream)
        pt.render_epoch_device(st.cuda_stream, SEED, 0, SPP, tiles.data_ptr())
        pt.untile_device(st.cuda_stream, tiles.data_ptr(), image.data_ptr())
    st.synchronize()
    assert bits_equal(image.cpu().numpy().reshape(HT, W, 3), want["epoch"])
    assert top_equal(top_dump(pt, nobj), want["dump"])
    # the upload figure
    c0 = pt.scene_counts()["uploaded_bytes"]
    pt.repose_refit_device(idx, d.data_ptr(), st.cuda_stream)
    c1 = pt.scene_counts()["uploaded_bytes"]
    other = np.ascontiguousarray(idx[::-1][:7])
    pt.repose_refit_device(other, d.data_ptr(), st.cuda_stream)
    c2 = pt.scene_counts()["uploaded_bytes"]
    assert c1 - c0 == 0 and c2 - c1 == 4 * len(other)
    pt.close()
    # three calls, one settle: the tree of three host refits
    steps = [C.scatter(S, C.particle_indices(), seed=s) for s in (11, 12, 13)]
    ref = make_pt(srt, S, device=-1)
    dev = make_pt(srt, S)
    before = dev.top_refit_count()
    keep = []
    for sidx, sT in steps:
        ref.repose_refit(sidx, sT)
        keep.append(on_device(torch, sT))
    torch.cuda.synchronize()
    for (sidx, _), t in zip(steps, keep):
        dev.repose_refit_device(sidx, t.data_ptr())
    got, want_dump = top_dump(dev, nobj), top_dump(ref, nobj)
    assert dev.top_refit_count() == before + 3 and top_equal(got, want_dump)
    assert IC.dumps_equal(IC.all_dumps(dev, nobj), IC.all_dumps(ref, nobj))
    dev.close(); ref.close()


def computed(pt, nobj):
    org, d, b = random_rays(5, 512)
    return {"dumps": IC.all_dumps(pt, nobj), "hits": pt.hit(org, d, b), "cost": pt.scene_tree_cost(), "count": pt.top_refit_count()}


def same_computed(a, b):
    return IC.dumps_equal(a["dumps"], b["dumps"]) and bits_equal(a["hits"], b["hits"]) and a["cost"] == b["cost"] and a["count"] == b["count"]


SETTLE_PATHS = ("repose", "repose_device", "update_mesh", "refit_mesh", "pose_refit", "hit", "scene_tree_cost", "build_scene")


@pytest.mark.parametrize("path", SETTLE_PATHS)
def test_settle_on_every_path(srt, torch, path):
    """After a device-form call, every entry point that is not enqueue-only gives what it gives after the host form of the same
    refit: it settles first."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    idx, Ts = C.sweeps_case(S)
    T2 = np.array([IC.translate(S["objects"][nobj - 1]["T"], (-0.2, 0.1, 0.1))], np.float32)
    p, n = UC.deformations()["D1"]
    dev, host = make_pt(srt, S), make_pt(srt, S)
    keep = [device_refit(torch, dev, idx, Ts)]
    host.repose_refit(idx, Ts)
    g, joints = SC.load_fixture("blob_chain3")
    skins = []
    for pt in (dev, host):
        if path == "repose":
            pt.repose([nobj - 1], T2)
        elif path == "repose_device":
            keep.append(on_device(torch, T2))
            torch.cuda.synchronize()
            pt.repose_device([nobj - 1], keep[-1].data_ptr())
        elif path == "update_mesh":
            pt.update_mesh(UC.BLOB_OBJECT, p, n)
        elif path == "refit_mesh":
            pt.refit_mesh(UC.BLOB_OBJECT, p, n)
        elif path == "pose_refit":
            skins.append(pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints))
            skins[-1].pose_refit(g["posed"][0])
        elif path == "build_scene":
            pt.build_scene(IC.with_poses(S, [1], [IC.translate(S["objects"][1]["T"], (0.0, 0.0, -0.05))]))
    if path == "hit":
        org, d, b = random_rays(5, 512)
        assert bits_equal(dev.hit(org, d, b), host.hit(org, d, b))
    if path == "scene_tree_cost":
        assert dev.scene_tree_cost() == host.scene_tree_cost()
    a, b = computed(dev, nobj), computed(host, nobj)
    assert same_computed(a, b)
    assert bits_equal(dev.render_epoch(SEED, 0, 2), host.render_epoch(SEED, 0, 2))
    dev.close(); host.close()


def test_particle_loop(srt, torch, particles):
    """particles_step_device -> particle_transforms_device -> repose_refit_device -> render_epoch_device, three frames on one
    stream, the host touched only at the end.  The positions equal the same loop's with repose_device (the closest hits the step
    kernel takes do not depend on the tree, ties apart: C.TIES_CAP), and hits and image equal the emulation of a refit of the
    final transforms bit for bit."""
    S = particles["S"]
    nobj = len(S["objects"])
    pidx = C.particle_indices()
    n = len(pidx)
    pos0 = RDC.particle_positions(S)
    rng = np.random.default_rng(8)
    vel0 = ((rng.random((n, 3)) - 0.5) * 2.0).astype(np.float32)
    results = {}
    for how in ("refit", "rebuild"):
        pt = make_pt(srt, S)
        local_tiles, _, floats_per_tile = pt.tile_info()
        d_pos, d_vel = torch.from_numpy(pos0.copy()).to("cuda:0"), torch.from_numpy(vel0.copy()).to("cuda:0")
        d_age, d_alive = torch.full((n,), 10.0, device="cuda:0"), torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        d_T = torch.zeros((n, 16), device="cuda:0")
        tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device="cuda:0")
        s = st.cuda_stream
        for frame in range(3):
            pt.particles_step_device(d_pos.data_ptr(), d_vel.data_ptr(), d_age.data_ptr(), n, 0.01, 0.015, d_alive.data_ptr(), s)
            pt.particle_transforms_device(d_pos.data_ptr(), n, RDC.PARTICLE_SCALE, d_T.data_ptr(), s)
            if how == "refit":
                pt.repose_refit_device(pidx, d_T.data_ptr(), s)
            else:
                pt.repose_device(pidx, d_T.data_ptr(), s)
            pt.render_epoch_device(s, SEED, frame, 1, tiles.data_ptr())
        pt.untile_device(s, tiles.data_ptr(), image.data_ptr())
        st.synchronize()
        org, d, b = random_rays(C.RAY_SEED, C.RAYS)
        results[how] = {"pos": d_pos.cpu().numpy(), "T": d_T.cpu().numpy(), "hits": pt.hit(org, d, b), "image": image.cpu().numpy().reshape(HT, W, 3),
                        "dump": top_dump(pt, nobj), "count": pt.top_refit_count()}
        pt.close()
    a, b = results["refit"], results["rebuild"]
    assert a["count"] == 3 and b["count"] == 0
    assert bits_equal(a["T"], RDC.translate_scale_product(a["pos"], RDC.PARTICLE_SCALE)) and not bits_equal(a["pos"], pos0)
    assert int(np.sum(np.any(a["pos"].view(np.uint32) != b["pos"].view(np.uint32), axis=1))) <= C.TIES_CAP
    assert int(np.sum(np.any(a["hits"].view(np.uint32) != b["hits"].view(np.uint32), axis=1))) <= C.TIES_CAP
    # the emulation: the committed tree refitted to the final transforms, the last frame's epoch
    e = C.EmuTop(S)
    assert e.repose_refit(pidx, a["T"]) == 0
    org, d, bb = random_rays(C.RAY_SEED, C.RAYS)
    samples = e.trace_samples(SEED, *C.every_sample(W, HT, 3))[0].reshape(HT, W, 3, 3)
    want_hits, want_dump = e.hit9(org, d, bb)[0], e.dump_top()
    e.close()
    assert bits_equal(a["hits"], want_hits) and top_equal(a["dump"], want_dump)
    assert bits_equal(a["image"], C.epoch_of(samples[:, :, 2:3], W, HT, 1))


def test_refusals_leave_the_scene(srt, torch, particles):
    """Every argument srt_pt_repose refuses, a NULL pointer and no commit: status and message; dumps, a render and the upload
    counter unchanged afterwards, nothing pending created - and the next refit works."""
    S, idx, Ts, want = particles["S"], particles["idx"], particles["Ts"], particles["want"]
    nobj = len(S["objects"])
    light = [k for k, o in enumerate(S["objects"]) if o.get("is_light")][0]
    pt = make_pt(srt, S)
    first, image, counts, refits = IC.all_dumps(pt, nobj), pt.render_epoch(SEED, 0, SPP), pt.scene_counts(), pt.top_refit_count()
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    cases = [("area light", [int(idx[0]), light]), ("listed twice", [int(idx[1]), int(idx[1])]), ("out of range", [nobj, int(idx[1])])]
    for match, bad in cases:
        for call, name in ((lambda: pt.repose_refit(bad, Ts[:2]), "srt_pt_repose_refit"), (lambda: pt.repose_refit_device(bad, d.data_ptr()), "srt_pt_repose_refit_device")):
            with pytest.raises(srt.SrtError, match=match) as e:
                call()
            assert e.value.status == INVALID and name + ":" in str(e.value)
        with pytest.raises(srt.SrtError, match=match) as r:
            pt.repose(bad, Ts[:2])
        assert re.split(r"srt_pt_\w+: ", str(r.value), 1)[1] == re.split(r"srt_pt_\w+: ", str(e.value), 1)[1]
    with pytest.raises(srt.SrtError, match="NULL argument") as e:
        pt.repose_refit_device(idx, 0)
    assert e.value.status == INVALID
    assert pt.scene_counts() == counts and pt.top_refit_count() == refits
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), first) and bits_equal(pt.render_epoch(SEED, 0, SPP), image)
    keep = device_refit(torch, pt, idx, Ts)
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), want["epoch"])
    pt.close()
    empty = srt.Pathtracer(0)
    for call in (lambda: empty.repose_refit(idx, Ts), lambda: empty.repose_refit_device(idx, d.data_ptr()), empty.scene_tree_cost):
        with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
            call()
        assert e.value.status == STATE
    empty.close()
    del keep


def test_scene_tree_cost(srt, torch, particles):
    """tree_cost of the dump; it rises when the particles are scattered by a refit and returns to the fresh commit's value after
    repose_device of the same poses."""
    S = particles["S"]
    nobj = len(S["objects"])
    idx, Ts = C.scatter(S, C.particle_indices(), spread=1.0)
    pt = make_pt(srt, S)
    cost0 = pt.scene_tree_cost()
    keep = device_refit(torch, pt, idx, Ts)
    cost1 = pt.scene_tree_cost()
    boxes, links, _ = top_dump(pt, nobj)
    pt.repose_device(idx, keep.data_ptr())
    cost2 = pt.scene_tree_cost()
    pt.close()
    fresh = make_pt(srt, IC.with_poses(S, idx, Ts), device=-1)
    fresh_cost = fresh.scene_tree_cost()
    fresh.close()
    print(f"tree cost: committed {cost0:.3f}, scattered and refitted {cost1:.3f}, rebuilt {cost2:.3f}")
    assert abs(cost1 - tree_cost_numpy(boxes, links)) <= 1e-9 * cost1
    assert cost1 > cost0 and cost1 > cost2 and cost2 == fresh_cost
    lst = make_pt(srt, S, use_bvh=False)
    with pytest.raises(srt.SrtError) as e:
        lst.scene_tree_cost()
    assert e.value.status == UNSUPPORTED
    lst.close()


def test_group(srt, torch, particles):
    """A two-rank PathtracerGroup on one device: repose_refit_device and repose_refit reach both members and the image is the
    single context's."""
    S, idx, Ts, want = particles["S"], particles["idx"], particles["Ts"], particles["want"]
    nobj = len(S["objects"])
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    grp.repose_refit_device(idx, [d.data_ptr(), d.data_ptr()])
    moved = grp.render_epoch(SEED, 0, SPP)
    dumps = [top_dump(m, nobj) for m in grp.members]
    grp.repose_refit(idx, particles["home"])
    home = grp.render_epoch(SEED, 0, SPP)
    with pytest.raises(ValueError):
        grp.repose_refit_device(idx, [d.data_ptr()])
    grp.close()
    single = make_pt(srt, S)
    first = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert bits_equal(moved, want["epoch"]) and bits_equal(home, first)
    assert all(top_equal(x, want["dump"]) for x in dumps)
