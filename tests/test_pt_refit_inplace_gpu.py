"""GPU: srt_pt_refit_mesh_inplace / srt_pt_refit_mesh_inplace_device / srt_pt_skin_pose_inplace[_at] - new vertices for one mesh of
a committed scene with BOTH trees kept; the device form only enqueues: the refit kernels of the mesh's tree, the link kernel
(pt_pose.hip) that poses the new root box for the mesh and its instances, and the BVH<Object>'s own refit stages.  Such a scene is
not a fresh commit's (the oracle would walk other trees), so the expectation is the host definition walked by the device headers on
the CPU (tests/_refit_inplace_cases.py: EmuInplace), produced here at test time; tests/test_pt_refit_inplace_host.py shows on the
CPU that its closest hits equal the oracle's.  Everything is compared bit for bit.  Device arrays are torch tensors passed by
data_ptr()."""
import re

import numpy as np
import pytest

import _anim_cases as AC
import _instance_cases as IC
import _light_cases as LC
import _refit_cases as RC
import _refit_inplace_cases as RI
import _repose_device_cases as RDC
import _repose_refit_cases as PR
import _skin_cases as SC
import _update_cases as UC
from _cases import pt_scene, random_rays
from _refit_cases import DEPTH, HT, SEED, SPP, W, bits_equal

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, STATE = -1, -4, -5
MODES = (0, 1, 2, 4, 5, 6, 7)
BLOB = UC.BLOB_OBJECT


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def make_pt(srt, scene, device=0, w=W, h=HT, depth=DEPTH, dynamic=False):
    pt = srt.Pathtracer(device)
    pt.set_params(w, h, 1, depth, True)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    if device >= 0:
        pt.set_camera(scene["camera"])
    return pt


def host_dumps(srt, scene, steps):
    """all_dumps of a host-only context after the steps' host forms: what srt_pt_dump_bvh must give on the device."""
    pt = make_pt(srt, scene, device=-1)
    RI.host_forms(pt, steps)
    d = IC.all_dumps(pt, len(scene["objects"]))
    pt.close()
    return d


def vertices_on_device(torch, p, n):
    return torch.from_numpy(np.ascontiguousarray(p, np.float32)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(n, np.float32)).to("cuda:0")


def device_inplace(torch, pt, index, p, n, stream=0):
    """The device form from fresh tensors; they are returned so that they live until the caller has waited."""
    tp, tn = vertices_on_device(torch, p, n)
    torch.cuda.synchronize()
    pt.refit_mesh_inplace_device(index, tp.data_ptr(), tn.data_ptr(), len(p), stream)
    return tp, tn


def check_against(pt, want, modes=MODES, w=W, h=HT, spp=SPP, hit_modes=(0, 5)):
    """Every sample with its RNG draw and ray ledgers, the hit records of both walks, the epoch image per kernel mode."""
    rgb, draws, rays = pt.trace_samples(SEED, *RC.every_sample(w, h, spp))
    assert np.array_equal(draws, want["samples"][1]) and np.array_equal(rays, want["samples"][2])
    assert bits_equal(rgb, want["samples"][0])
    org, d, b = random_rays(RI.RAY_SEED, RI.RAYS)
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


def same_computed(a, b, nobj, spp=2):
    ra, rb = a.trace_samples(SEED, *RC.every_sample(W, HT, spp)), b.trace_samples(SEED, *RC.every_sample(W, HT, spp))
    assert bits_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert bits_equal(a.render_epoch(SEED, 0, spp), b.render_epoch(SEED, 0, spp))
    assert IC.dumps_equal(IC.all_dumps(a, nobj), IC.all_dumps(b, nobj))
    assert a.scene_tree_cost() == b.scene_tree_cost()


@pytest.fixture(scope="module")
def blob(srt):
    """cbox+blob512, its three deformations, and per deformation the emulated expectation and the host-only context's dumps
    (computed once, left unchanged).  An in-place refit's result depends on the new vertices alone, not on the refits before it."""
    S = UC.blob_scene()
    D = UC.deformations()
    want = {name: RI.expectation(S, [("inplace", BLOB, p, n)]) for name, (p, n) in D.items()}
    dumps = {name: host_dumps(srt, S, [("inplace", BLOB, p, n)]) for name, (p, n) in D.items()}
    return {"S": S, "D": D, "want": want, "dumps": dumps}


@pytest.mark.parametrize("form", ["device", "host"])
def test_blob_refits(srt, torch, blob, form):
    """D1, D2, D3 in turn on one context through the device form from a torch tensor (and through the host form on a device
    context), every kernel form after each: per-sample radiance, RNG draw and ray ledgers, hit records of both walks, the epoch
    image, the dumped trees; no build, no upload of a triangle-class byte, and the device form steady at zero uploaded bytes."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    pt = make_pt(srt, S)
    keep = []
    for k, (name, (p, n)) in enumerate(blob["D"].items()):
        before = pt.scene_counts()
        if form == "device":
            keep.append(device_inplace(torch, pt, BLOB, p, n))
        else:
            pt.refit_mesh_inplace(BLOB, p, n)
        after = pt.scene_counts()
        assert after["refits"] == before["refits"] + 1 and after["blas_builds"] == before["blas_builds"], name
        assert after["uploaded_triangle_bytes"] == before["uploaded_triangle_bytes"], name
        assert {x: after[x] for x in ("objects", "triangles", "blas_nodes", "blas_records", "device_bytes")} == \
               {x: before[x] for x in ("objects", "triangles", "blas_nodes", "blas_records", "device_bytes")}, name
        if k and form == "device":
            assert after["uploaded_bytes"] == before["uploaded_bytes"], name
        if k and form == "host":                       # the vertices, the top-level nodes and the sweep records - no table of object order
            nodes = len(blob["dumps"][name][0][1])
            assert after["uploaded_bytes"] - before["uploaded_bytes"] == 24 * len(p) + 32 * nodes + 64 * (nodes // 2), name
        check_against(pt, blob["want"][name])
        assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"][name]), name
        assert PR.bits_equal_nan(pt.dump_bvh(-1)[0], blob["want"][name]["dump"][0])
    pt.close()


def test_sweeps_scene(srt, torch):
    """At most 16 objects - the wave kernel reads the sweep records - and the blob has a rotated, non-uniformly scaled instance."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    assert nobj <= 16
    p, n = UC.deformations()["D2"]
    steps = [("inplace", BLOB, p, n)]
    pt = make_pt(srt, S)
    keep = device_inplace(torch, pt, BLOB, p, n)
    check_against(pt, RI.expectation(S, steps), modes=(0, 2, 7))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), host_dumps(srt, S, steps))
    pt.close()
    del keep


def test_enqueue_only(srt, torch, blob):
    """On a side stream behind a few busy matmuls: a torch op writes the vertices, then refit_mesh_inplace_device, render_epoch_device
    and untile_device with no host call in between and one synchronize at the end - the image is the emulation's.  A second
    steady-state call uploads nothing; three calls before one dump are (3, 1) pending, one settle and three refits."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    p, n = blob["D"]["D1"]
    pt = make_pt(srt, S)
    local_tiles, _, floats_per_tile = pt.tile_info()
    half_p, tn = vertices_on_device(torch, p * np.float32(0.5), n)
    tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
    image = torch.zeros(HT * W * 3, device="cuda:0")
    busy = torch.ones((1024, 1024), device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        for _ in range(4):
            busy = busy @ busy * 1e-3
        tp = half_p + half_p                              # exact: p again, written by a kernel on the stream
        pt.refit_mesh_inplace_device(BLOB, tp.data_ptr(), tn.data_ptr(), len(p), st.cuda_stream)
        pt.render_epoch_device(st.cuda_stream, SEED, 0, SPP, tiles.data_ptr())
        pt.untile_device(st.cuda_stream, tiles.data_ptr(), image.data_ptr())
    st.synchronize()
    assert bits_equal(image.cpu().numpy().reshape(HT, W, 3), blob["want"]["D1"]["epoch"])
    # mesh_tree_cost is the first call that is not enqueue-only: it settles, and gives the host form's figure for the refitted tree
    assert pt.mesh_refit_pending() == (1, 1)
    only = make_pt(srt, S, device=-1)
    committed = only.mesh_tree_cost(BLOB)
    only.refit_mesh_inplace(BLOB, p, n)
    want_cost = only.mesh_tree_cost(BLOB)
    only.close()
    assert pt.mesh_tree_cost(BLOB) == want_cost != committed and pt.mesh_refit_pending() == (0, 0)
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"]["D1"])
    c0 = pt.scene_counts()
    pt.refit_mesh_inplace_device(BLOB, tp.data_ptr(), tn.data_ptr(), len(p), st.cuda_stream)
    assert pt.mesh_refit_pending() == (1, 1)
    c1 = pt.scene_counts()
    assert c1["uploaded_bytes"] - c0["uploaded_bytes"] == 0 and pt.mesh_refit_pending() == (0, 0)
    # three calls, one settle: the caller's arrays are overwritten behind each call, the host's record is the last call's
    keep = [vertices_on_device(torch, *blob["D"][name]) for name in ("D2", "D3", "D2")]
    torch.cuda.synchronize()
    for a, b in keep:
        pt.refit_mesh_inplace_device(BLOB, a.data_ptr(), b.data_ptr(), len(p))
        a.zero_()
    assert pt.mesh_refit_pending() == (3, 1)
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"]["D2"]) and pt.mesh_refit_pending() == (0, 0)
    assert pt.scene_counts()["refits"] == c1["refits"] + 3 and pt.top_refit_count() == 0
    check_against(pt, blob["want"]["D2"], modes=(0,))
    pt.close()


def test_shared_tables(srt, torch):
    """refit_mesh_inplace_device followed, with no settle in between, by repose_refit_device of the mesh, its instance and another
    object: that call poses the NEW object-space boxes, and uploads only its list.  Equal to the host forms in the same order."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    p, n = UC.deformations()["D3"]
    idx = np.array([BLOB, RI.family_of(S, BLOB)[1], 5], np.uint32)
    Ts = np.array([IC.translate(S["objects"][int(i)]["T"], d) for i, d in zip(idx, ((0.1, 0.05, -0.1), (-0.15, 0.1, 0.05), (0.05, 0.0, 0.1)))], np.float32)
    steps = [("inplace", BLOB, p, n), ("repose_refit", idx, Ts)]
    dev = make_pt(srt, S)
    d_T = torch.from_numpy(Ts).to("cuda:0")
    keep = device_inplace(torch, dev, BLOB, p, n)
    c0 = dev.scene_counts()["uploaded_bytes"]              # (settles; then both calls are made again, back to back)
    dev.refit_mesh_inplace_device(BLOB, keep[0].data_ptr(), keep[1].data_ptr(), len(p))
    dev.repose_refit_device(idx, d_T.data_ptr())
    assert dev.mesh_refit_pending() == (1, 1) and dev.top_refit_pending() == (2, 3)
    c1 = dev.scene_counts()
    assert c1["uploaded_bytes"] - c0 == 4 * len(idx) and dev.top_refit_count() == 1 and c1["refits"] == 2
    check_against(dev, RI.expectation(S, steps), modes=(0, 2, 6))
    assert IC.dumps_equal(IC.all_dumps(dev, nobj), host_dumps(srt, S, steps))
    host = make_pt(srt, S)
    RI.host_forms(host, steps)
    same_computed(dev, host, nobj)
    dev.close(); host.close()


def set_rig(skin, rig):
    skin.set_rig(*[rig[k] for k in ("parent", "base", "rest_pose", "knot_offsets", "knot_times", "knot_quats")])


def test_skins(srt, blob):
    """Skin.pose_inplace / pose_inplace_at on the recorded skin_blob_chain3 poses and rig against pose_refit / pose_refit_at followed
    by repose_refit of the family with its transforms.  The staging is overwritten by a second pose before the first settles: the
    host's record is the last pose's.  With a rig a frame uploads nothing."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    g, joints = SC.load_fixture("blob_chain3")
    rig = AC.load_rig("blob_chain3")
    family = RI.family_of(S, BLOB)
    Ts = PR.transforms_of(S)[family]
    pt, other = make_pt(srt, S), make_pt(srt, S)
    skin, skin2 = (x.create_skin(BLOB, g["pos"], g["nrm"], joints) for x in (pt, other))
    set_rig(skin, rig); set_rig(skin2, rig)
    for k, posed in enumerate(g["posed"]):
        flat = k == 1
        skin.pose_inplace(g["posed"][(k + 1) % len(g["posed"])], flat_normals=not flat)      # (overwritten before it settles)
        skin.pose_inplace(posed, flat_normals=flat)
        assert pt.mesh_refit_pending() == (2, 1)
        skin2.pose_refit(posed, flat_normals=flat)
        other.repose_refit(family, Ts)
        same_computed(pt, other, nobj)
    skin.pose_inplace_at(float(rig["times"][2]))            # (the first call with the rig has made nothing new either)
    for i in (6, 11):
        c0 = pt.scene_counts()
        skin.pose_inplace_at(float(rig["times"][i]), flat_normals=i == 6)
        skin2.pose_refit_at(float(rig["times"][i]), flat_normals=i == 6)
        other.repose_refit(family, Ts)
        c1 = pt.scene_counts()
        assert c1["uploaded_bytes"] == c0["uploaded_bytes"] and c1["refits"] == c0["refits"] + 1
        same_computed(pt, other, nobj)
    skin.close(); skin2.close()
    pt.close(); other.close()


def two_meshes_and_an_instance():
    """two_mesh_scene() plus an instance of the blob (object 6) and one of the small blob (object 8): objects 9 and 10."""
    S = UC.two_mesh_scene()
    S["objects"].append(dict(IC.sweeps_scene()["objects"][-1]))
    T = IC.translate(S["objects"][8]["T"], (0.45, -0.3, 0.25))
    S["objects"].append({"kind": "instance", "of": 8, "T": T, "material": 5})
    return S


def test_two_meshes_with_instances(srt, torch):
    """Each mesh refitted in turn, both pending at once: two entries, one settle; the instances follow their sources."""
    S = two_meshes_and_an_instance()
    nobj = len(S["objects"])
    p6, n6 = UC.deformations()["D2"]
    p8, n8 = UC.small_blob_deformation()
    steps = [("inplace", 6, p6, n6), ("inplace", 8, p8, n8)]
    pt = make_pt(srt, S)
    keep = [device_inplace(torch, pt, 6, p6, n6), device_inplace(torch, pt, 8, p8, n8)]
    pt.refit_mesh_inplace_device(6, keep[0][0].data_ptr(), keep[0][1].data_ptr(), len(p6))
    assert pt.mesh_refit_pending() == (3, 2)
    check_against(pt, RI.expectation(S, steps), modes=(0, 2, 6))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), host_dumps(srt, S, steps)) and pt.scene_counts()["refits"] == 3
    pt.close()


@pytest.mark.parametrize("plan", ["shared_launches", "launch_per_level"])
def test_deep_tree(srt, torch, monkeypatch, plan):
    """deep_both: the chain's BVH<Triangle> nests 48 interior nodes under a BVH<Object> nesting 24, under both launch plans
    (SRT_REFIT_LEVEL_LAUNCHES is read when a tree's refit tables are made)."""
    if plan == "launch_per_level":
        monkeypatch.setenv("SRT_REFIT_LEVEL_LAUNCHES", "1")
    D = pt_scene("deep_both")
    w, h, depth, spp = RC.DEEP
    p, n = RC.deep_moved(D)
    steps = [("inplace", RC.DEEP_MESH, p, n)]
    pt = make_pt(srt, D, w=w, h=h, depth=depth)
    keep = device_inplace(torch, pt, RC.DEEP_MESH, p, n)
    check_against(pt, RI.expectation(D, steps, w, h, depth, spp), modes=(0, 1, 4, 6), w=w, h=h, spp=spp)
    assert IC.dumps_equal(IC.all_dumps(pt, len(D["objects"])), host_dumps(srt, D, steps))
    pt.close()
    del keep


def test_levels_beyond_one_workgroup(srt, torch, scenes):
    """cornell_with_mesh(5): 8 192 triangles, whose tree has levels of more than 256 interior nodes."""
    S = scenes.cornell_with_mesh(5, "glass")
    p, n, i = UC.blob_arrays(5, seed=11)
    assert np.array_equal(i, S["objects"][6]["idx"])
    steps = [("inplace", 6, p, n)]
    pt = make_pt(srt, S)
    keep = device_inplace(torch, pt, 6, p, n)
    image = pt.render_epoch(SEED, 0, SPP)
    got = IC.all_dumps(pt, 8)
    pt.close()
    assert PR.widest_level(got[1 + RC.slot_of(got[0], 6, 8)][1]) > 256
    assert IC.dumps_equal(got, host_dumps(srt, S, steps))
    assert bits_equal(image, RI.expectation(S, steps, samples=True)["epoch"])
    del keep


def test_emissive_mesh(srt, torch):
    """An emissive mesh under set_dynamic_lights: the light tables of both sides equal the host form's; refused with refit_mesh's text
    while the switch is off."""
    S = LC.blob_light_scene()
    nobj = len(S["objects"])
    dev, host = make_pt(srt, S, dynamic=True), make_pt(srt, S, dynamic=True)
    only = make_pt(srt, S, device=-1, dynamic=True)
    first = dev.dump_lights(from_device=True)
    keep = []
    for name, (p, n) in LC.blob_light_deformations().items():
        keep.append(device_inplace(torch, dev, LC.BLOB_LIGHT, p, n))
        host.refit_mesh_inplace(LC.BLOB_LIGHT, p, n)
        only.refit_mesh_inplace(LC.BLOB_LIGHT, p, n)
        want = only.dump_lights()
        assert LC.lights_equal(dev.dump_lights(from_device=True), want) and LC.lights_equal(dev.dump_lights(), want), name
        assert LC.lights_equal(host.dump_lights(from_device=True), want) and not LC.lights_equal(first, want), name
        same_computed(dev, host, nobj)
    dev.close(); host.close(); only.close()
    off = make_pt(srt, S)
    p, n = LC.blob_light_deformations()["D1"]
    tp, tn = vertices_on_device(torch, p, n)
    torch.cuda.synchronize()
    image, texts = off.render_epoch(SEED, 0, 2), []
    for call in (lambda: off.refit_mesh(LC.BLOB_LIGHT, p, n), lambda: off.refit_mesh_inplace(LC.BLOB_LIGHT, p, n),
                 lambda: off.refit_mesh_inplace_device(LC.BLOB_LIGHT, tp.data_ptr(), tn.data_ptr(), len(p))):
        with pytest.raises(srt.SrtError, match="area light") as e:
            call()
        assert e.value.status == INVALID
        texts.append(re.split(r"srt_pt_\w+: ", str(e.value), 1)[1])
    assert texts[0] == texts[1] == texts[2] and off.mesh_refit_pending() == (0, 0)
    assert bits_equal(off.render_epoch(SEED, 0, 2), image)
    off.close()


SETTLE_PATHS = ("repose", "repose_device", "update_mesh", "refit_mesh", "pose_refit", "hit", "scene_tree_cost", "build_scene", "update_same_mesh")


@pytest.mark.parametrize("path", SETTLE_PATHS)
def test_settle_on_every_path(srt, torch, path):
    """After a device-form call, every entry point that is not enqueue-only gives what it gives after the host form of the same
    refit: it settles first.  (update_mesh: of the small blob, another mesh; update_same_mesh: of the refitted one.)"""
    S = two_meshes_and_an_instance()
    nobj = len(S["objects"])
    p, n = UC.deformations()["D1"]
    p2, n2 = UC.deformations()["D2"]
    p8, n8 = UC.small_blob_deformation()
    T2 = np.array([IC.translate(S["objects"][nobj - 1]["T"], (-0.2, 0.1, 0.1))], np.float32)
    dev, host = make_pt(srt, S), make_pt(srt, S)
    keep = [device_inplace(torch, dev, BLOB, p, n)]
    host.refit_mesh_inplace(BLOB, p, n)
    g, joints = SC.load_fixture("blob_chain3")
    skins = []
    for pt in (dev, host):
        if path == "repose":
            pt.repose([nobj - 1], T2)
        elif path == "repose_device":
            keep.append(torch.from_numpy(T2).to("cuda:0"))
            torch.cuda.synchronize()
            pt.repose_device([nobj - 1], keep[-1].data_ptr())
        elif path == "update_mesh":
            pt.update_mesh(8, p8, n8)
        elif path == "update_same_mesh":
            pt.update_mesh(BLOB, p2, n2)
        elif path == "refit_mesh":
            pt.refit_mesh(BLOB, p2, n2)
        elif path == "pose_refit":
            skins.append(pt.create_skin(BLOB, g["pos"], g["nrm"], joints))
            skins[-1].pose_refit(g["posed"][0])
        elif path == "build_scene":
            pt.build_scene(IC.with_poses(S, [1], [IC.translate(S["objects"][1]["T"], (0.0, 0.0, -0.05))]))
    if path == "hit":
        org, d, b = random_rays(5, 512)
        assert bits_equal(dev.hit(org, d, b), host.hit(org, d, b))
    if path == "scene_tree_cost":
        assert dev.scene_tree_cost() == host.scene_tree_cost()
    assert dev.mesh_refit_pending() == (0, 0)
    same_computed(dev, host, nobj)
    assert dev.scene_counts()["refits"] == host.scene_counts()["refits"] and dev.top_refit_count() == host.top_refit_count()
    # and an in-place refit afterwards works from whatever trees that path left
    keep.append(device_inplace(torch, dev, BLOB, *UC.deformations()["D3"]))
    host.refit_mesh_inplace(BLOB, *UC.deformations()["D3"])
    same_computed(dev, host, nobj)
    for k in skins:
        k.close()
    dev.close(); host.close()


def test_refusals(srt, torch):
    """Each refusal returns its status and leaves both sides as they were; a host-only context is refused as unsupported."""
    lib = srt.load_library()
    S = IC.sweeps_scene()
    pt = make_pt(srt, S)
    image, counts = pt.render_epoch(SEED, 0, 2), pt.scene_counts()
    p, n = UC.deformations()["D1"]
    lp, ln = UC.original(S, 7)
    tp, tn = vertices_on_device(torch, p, n)
    tl, tln = vertices_on_device(torch, lp, ln)
    nan = p.copy()
    nan[100, 2] = np.nan
    torch.cuda.synchronize()
    cases = [("an area light", 7, tl, tln, len(lp)), ("an instance", 8, tp, tn, len(p)), ("another vertex count", 6, tp, tn, len(p) - 3),
             ("a sphere", 5, tp, tn, len(p)), ("out of range", len(S["objects"]), tp, tn, len(p))]
    for what, index, a, b, nverts in cases:
        assert lib.srt_pt_refit_mesh_inplace_device(pt._ctx, None, index, a.data_ptr(), b.data_ptr(), nverts) == INVALID, what
        assert pt.mesh_refit_pending() == (0, 0) and pt.top_refit_pending() == (0, 0), what
        assert pt.render_epoch(SEED, 0, 2).tobytes() == image.tobytes() and pt.scene_counts() == counts, what
    for what, index, pp, nn, nverts in [(w, i, a.cpu().numpy(), b.cpu().numpy(), v) for w, i, a, b, v in cases] + [("a NaN", 6, nan, n, len(p))]:
        pp, nn = np.ascontiguousarray(pp, np.float32), np.ascontiguousarray(nn, np.float32)
        assert lib.srt_pt_refit_mesh_inplace(pt._ctx, index, pp.ctypes.data, nn.ctypes.data, nverts) == INVALID, what
        assert pt.render_epoch(SEED, 0, 2).tobytes() == image.tobytes() and pt.scene_counts() == counts, what
    assert lib.srt_pt_refit_mesh_inplace_device(pt._ctx, None, 6, None, tn.data_ptr(), len(p)) == INVALID
    pt.close()
    only = make_pt(srt, S, device=-1)
    first = IC.all_dumps(only, len(S["objects"]))
    with pytest.raises(srt.SrtError, match="host-only") as e:
        only.refit_mesh_inplace_device(6, tp.data_ptr(), tn.data_ptr(), len(p))
    assert e.value.status == UNSUPPORTED and IC.dumps_equal(IC.all_dumps(only, len(S["objects"])), first)
    only.close()


def test_nan_vertex(srt, torch, blob):
    """A NaN vertex is not refused by the device form: it returns OK and so does sync(), the host's record takes what the kernels
    computed; a following finite in-place refit gives exactly the finite case's results.  No render in between."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    p, n = blob["D"]["D1"]
    bad = p.copy()
    bad[100, 2] = np.nan
    pt = make_pt(srt, S)
    keep = [device_inplace(torch, pt, BLOB, bad, n)]
    pt.sync()
    assert pt.mesh_refit_pending() == (0, 0)
    only = make_pt(srt, S, device=-1)
    got, was = pt.dump_bvh(RC.slot_of(pt, BLOB, nobj)), only.dump_bvh(RC.slot_of(only, BLOB, nobj))
    only.close()
    assert np.array_equal(got[1], was[1]) and np.array_equal(got[2], was[2])      # links and order: the committed ones
    keep.append(device_inplace(torch, pt, BLOB, p, n))
    check_against(pt, blob["want"]["D1"], modes=(0, 6))
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), blob["dumps"]["D1"])
    pt.close()


def test_mixed_pool_frame(srt, torch):
    """One stream, no host wait: particles_step_device -> particle_transforms_device -> set_active_device -> repose_refit_device ->
    Skin.pose_inplace_at -> render_epoch_device, on the particle scene plus the rigged blob.  Compared with the host forms applied
    in the same order to a second context, from the positions and flags the first one computed."""
    base = IC.particles_shared()[0]
    B = UC.blob_scene()
    S = dict(base, objects=list(base["objects"]) + [dict(B["objects"][BLOB], material=0)])
    nobj = len(S["objects"])
    mesh = nobj - 1
    g, joints = SC.load_fixture("blob_chain3")
    rig = AC.load_rig("blob_chain3")
    pidx = PR.particle_indices()
    npart = len(pidx)
    pos0 = RDC.particle_positions(S)
    vel0 = ((np.random.default_rng(8).random((npart, 3)) - 0.5) * 2.0).astype(np.float32)
    t = float(rig["times"][6])
    dev, host = make_pt(srt, S), make_pt(srt, S)
    skin, skin2 = (x.create_skin(mesh, g["pos"], g["nrm"], joints) for x in (dev, host))
    set_rig(skin, rig); set_rig(skin2, rig)
    local_tiles, _, floats_per_tile = dev.tile_info()
    d_pos, d_vel = torch.from_numpy(pos0.copy()).to("cuda:0"), torch.from_numpy(vel0.copy()).to("cuda:0")
    d_age, d_alive = torch.full((npart,), 0.02, device="cuda:0"), torch.zeros(npart, dtype=torch.uint8, device="cuda:0")
    d_T = torch.zeros((npart, 16), device="cuda:0")
    tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    dev.particles_step_device(d_pos.data_ptr(), d_vel.data_ptr(), d_age.data_ptr(), npart, 0.01, 0.015, d_alive.data_ptr(), s)
    dev.particle_transforms_device(d_pos.data_ptr(), npart, RDC.PARTICLE_SCALE, d_T.data_ptr(), s)
    dev.set_active_device(pidx, d_alive.data_ptr(), s)
    dev.repose_refit_device(pidx, d_T.data_ptr(), s)
    skin.pose_inplace_at(t, stream=s)
    dev.render_epoch_device(s, SEED, 0, 2, tiles.data_ptr())
    dev.untile_device(s, tiles.data_ptr(), image.data_ptr())
    st.synchronize()
    assert dev.mesh_refit_pending() == (1, 1) and dev.top_refit_pending()[0] == 3
    host.set_active(pidx, d_alive.cpu().numpy())
    host.repose_refit(pidx, d_T.cpu().numpy())
    host.refit_mesh_inplace(mesh, *skin2.vertices(rig["posed"][6]))      # (the BVH<Object> of moved particles is not what a rebuild gives)
    assert bits_equal(image.cpu().numpy().reshape(HT, W, 3), host.render_epoch(SEED, 0, 2))
    assert np.array_equal(dev.active(), host.active())
    same_computed(dev, host, nobj)
    skin.close(); skin2.close()
    dev.close(); host.close()


def test_group(srt, torch, blob):
    """A two-rank group on one device: the host form, the device form and the skin form; the image is a single context's."""
    S = blob["S"]
    p, n = blob["D"]["D2"]
    g, joints = SC.load_fixture("blob_chain3")
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    grp.refit_mesh_inplace(BLOB, *blob["D"]["D1"])
    first = grp.render_epoch(SEED, 0, SPP)
    tp, tn = vertices_on_device(torch, p, n)
    torch.cuda.synchronize()
    grp.refit_mesh_inplace_device(BLOB, [tp.data_ptr()] * 2, [tn.data_ptr()] * 2, len(p))
    assert all(m.mesh_refit_pending() == (0, 0) for m in grp.members)
    moved = grp.render_epoch(SEED, 0, SPP)
    counts = grp.scene_counts()
    skins = grp.create_skin(BLOB, g["pos"], g["nrm"], joints)
    skins.pose_inplace(g["posed"][0])
    posed = grp.render_epoch(SEED, 0, SPP)
    rig = AC.load_rig("blob_chain3")
    set_rig(skins, rig)
    skins.pose_inplace_at(float(rig["times"][6]), flat_normals=True)
    assert all(m.mesh_refit_pending() == (0, 0) for m in grp.members)
    keyed = grp.render_epoch(SEED, 0, SPP)
    skins.close(); grp.close()
    single = make_pt(srt, S)
    skin = single.create_skin(BLOB, g["pos"], g["nrm"], joints)
    skin.pose_inplace(g["posed"][0])
    image = single.render_epoch(SEED, 0, SPP)
    skin.pose_inplace(rig["posed"][6], flat_normals=True)
    image_keyed = single.render_epoch(SEED, 0, SPP)
    skin.close(); single.close()
    assert bits_equal(first, blob["want"]["D1"]["epoch"]) and bits_equal(moved, blob["want"]["D2"]["epoch"]) and bits_equal(posed, image)
    assert bits_equal(keyed, image_keyed) and not bits_equal(keyed, posed)
    assert counts[0] == counts[1] and counts[0]["refits"] == 2
