"""GPU: srt_pt_repose_device - new poses from a device array of transforms - against srt_pt_repose of the same matrices on an
identical context: everything the scene computes must be bit-equal (trees, hit records, every sample, the epoch image of every
kernel form), refusals must leave the scene as it was, and the records must never be uploaded.  Device arrays are torch tensors
passed by data_ptr()."""
import numpy as np
import pytest

import _instance_cases as IC
import _repose_device_cases as RC
from _cases import random_rays

pytestmark = pytest.mark.gpu

NOBJ = 74
W, HT, DEPTH, SPP, SEED = 32, 24, 4, 2, 9
INVALID, UNSUPPORTED = -1, -4


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make_pt(srt, scene, w=W, h=HT, depth=DEPTH, use_bvh=True, builder=None):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, use_bvh)
    if builder is not None:
        pt.set_bvh_builder(*builder)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def on_device(torch, Ts):
    return torch.from_numpy(np.ascontiguousarray(Ts, np.float32).reshape(-1, 16)).to("cuda:0")


def device_repose(torch, pt, idx, Ts, stream=0):
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    pt.repose_device(idx, d.data_ptr(), stream)


def every_sample(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32), ss.reshape(-1).astype(np.uint32)


def epochs(pt, modes, spp=SPP):
    out = {}
    for mode in modes:
        pt.set_kernel(mode)
        out[mode] = pt.render_epoch(SEED, 0, spp)
    pt.set_kernel(0)
    return out


def computed(pt, nobj, w, h, spp, modes, nrays=512):
    """Everything the tests compare of a context: trees, hit records, every sample, the epoch image per kernel mode."""
    org, d, b = random_rays(5, nrays)
    return {"dumps": IC.all_dumps(pt, nobj), "hits": pt.hit(org, d, b), "samples": pt.trace_samples(SEED, *every_sample(w, h, spp)),
            "epochs": epochs(pt, modes, spp)}


def assert_same(got, want, what=""):
    assert IC.dumps_equal(got["dumps"], want["dumps"]), what
    assert bits_equal(got["hits"], want["hits"]), what
    assert np.array_equal(got["samples"][1], want["samples"][1]) and np.array_equal(got["samples"][2], want["samples"][2]), what
    assert bits_equal(got["samples"][0], want["samples"][0]), what
    for mode, image in want["epochs"].items():
        assert bits_equal(got["epochs"][mode], image), (what, mode)


PARTICLE_MODES = (0, 1, 4, 6)


@pytest.fixture(scope="module")
def particles(srt):
    """S, repose_case(S), and what a context computes before and after srt_pt_repose of that case (computed once)."""
    S = IC.particles_shared()[0]
    idx, Ts = IC.repose_case(S)
    pt = make_pt(srt, S)
    first = computed(pt, NOBJ, W, HT, SPP, PARTICLE_MODES)
    pt.repose(idx, Ts)
    moved = computed(pt, NOBJ, W, HT, SPP, PARTICLE_MODES)
    pt.close()
    assert not bits_equal(first["epochs"][0], moved["epochs"][0]) and np.count_nonzero(moved["hits"][:, 0]) > 100
    return {"S": S, "idx": idx, "Ts": Ts, "home": np.array([S["objects"][i]["T"] for i in idx], np.float32), "first": first, "moved": moved}


def test_equals_repose(srt, torch, particles):
    """12 objects of the 74-object scene - an instance with a rotation, the source with a non-uniform scale, a sphere: trees, hit
    records, every sample, every kernel form; and back through the device form."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    assert S["objects"][idx[0]]["kind"] == "mesh" and S["objects"][idx[1]]["kind"] == "instance" and S["objects"][idx[-1]]["kind"] == "sphere"
    pt = make_pt(srt, S)
    device_repose(torch, pt, idx, Ts)
    got = computed(pt, NOBJ, W, HT, SPP, PARTICLE_MODES)
    device_repose(torch, pt, idx, particles["home"])
    back = computed(pt, NOBJ, W, HT, SPP, (0,))
    # the host's record is true: a host repose after device reposes starts from it
    pt.repose(idx[:3], Ts[:3])
    device_repose(torch, pt, idx[3:], Ts[3:])
    mixed = computed(pt, NOBJ, W, HT, SPP, (0,))
    pt.close()
    assert_same(got, particles["moved"], "moved")
    assert_same(back, dict(particles["first"], epochs={0: particles["first"]["epochs"][0]}), "back")
    assert_same(mixed, dict(particles["moved"], epochs={0: particles["moved"]["epochs"][0]}), "host and device reposes mixed")


def test_sweeps_scene(srt, torch):
    """9 objects, the instance of the 512-triangle blob re-posed to the other side of its source: object order, the meshes'
    ordinals and the lazy bits change; the sweeps with inline walks (2), the flattened walk (5), the streamed forms (6, 7, auto)."""
    S = IC.sweeps_scene()
    n = len(S["objects"])
    T = IC.translate(S["objects"][n - 1]["T"], (0.5, -0.25, 0.3))
    modes = (0, 2, 5, 6, 7)
    ref, dev = make_pt(srt, S, 32, 32, 5), make_pt(srt, S, 32, 32, 5)
    first = computed(ref, n, 32, 32, 2, (0,))
    ref.repose([n - 1], [T])
    device_repose(torch, dev, [n - 1], [T])
    want, got = computed(ref, n, 32, 32, 2, modes), computed(dev, n, 32, 32, 2, modes)
    device_repose(torch, dev, [n - 1], [S["objects"][n - 1]["T"]])
    back = computed(dev, n, 32, 32, 2, (0,))
    ref.close(); dev.close()
    assert not bits_equal(want["epochs"][0], first["epochs"][0])
    assert_same(got, want, "moved")
    assert_same(back, first, "back")


def test_device_builder(srt, torch, particles):
    """set_bvh_builder(True, 8): the BVH<Object> of the 74 objects comes from the device builder, over boxes that were never on
    the host.  Trees and images are those of the host-builder context."""
    pt = make_pt(srt, particles["S"], builder=(True, 8))
    device_repose(torch, pt, particles["idx"], particles["Ts"])
    got = computed(pt, NOBJ, W, HT, SPP, (0, 6))
    device_repose(torch, pt, particles["idx"], particles["home"])
    back = computed(pt, NOBJ, W, HT, SPP, (0,))
    pt.close()
    assert_same(got, dict(particles["moved"], epochs={m: particles["moved"]["epochs"][m] for m in (0, 6)}), "device builder")
    assert_same(back, dict(particles["first"], epochs={0: particles["first"]["epochs"][0]}), "device builder, back")


def test_identity_and_translation(srt, torch, particles):
    """An identity matrix whose off-diagonal zeros are -0.0f (has_trans == 0: the box is not posed, the rays are not transformed)
    on one sphere, a pure translation on another."""
    S = particles["S"]
    a, b = IC.PARTICLE_FIRST + IC.PARTICLE_COUNT, IC.PARTICLE_FIRST + IC.PARTICLE_COUNT + 1
    assert S["objects"][a]["kind"] == "sphere" and S["objects"][b]["kind"] == "sphere"
    ident = RC.identity()
    ident[[1, 2, 4, 6, 8, 9, 12, 13, 14]] = np.float32(-0.0)
    Ts = np.stack([ident, RC.translate_scale((0.2, 0.35, -0.1), 1.0)])
    ref, dev = make_pt(srt, S), make_pt(srt, S)
    ref.repose([a, b], Ts)
    device_repose(torch, dev, [a, b], Ts)
    want, got = computed(ref, NOBJ, W, HT, SPP, (0,), nrays=2048), computed(dev, NOBJ, W, HT, SPP, (0,), nrays=2048)
    ref.close(); dev.close()
    assert np.count_nonzero(want["hits"][:, 0]) > 500
    assert_same(got, want)


def test_list_mode(srt, torch, particles):
    """A scene committed with use_bvh = 0: slot order is insertion order, there is no tree."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    ref, dev = make_pt(srt, S, use_bvh=False), make_pt(srt, S, use_bvh=False)
    org, d, b = random_rays(5, 512)
    before = dev.hit(org, d, b)
    ref.repose(idx, Ts)
    device_repose(torch, dev, idx, Ts)
    want = (ref.hit(org, d, b), ref.render_epoch(SEED, 0, SPP))
    got = (dev.hit(org, d, b), dev.render_epoch(SEED, 0, SPP))
    ref.close(); dev.close()
    assert not bits_equal(before, want[0])
    assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
    assert bits_equal(got[1], particles["moved"]["epochs"][0])       # (the image does not depend on how the objects are searched)


def test_upload_accounting(srt, torch, particles):
    """Every non-light object re-posed.  The host form uploads whole 176-B records; the device form uploads none: what it adds to
    the upload figure is at most the host form's minus the 128 B of matrices per listed object (the first call, which sends 24 B of
    object-space box per object), and at most the host form's minus the records plus 8 B per slot and 4 B per listed object
    (every later call: the order of a host-built tree, the mesh ordinals, the list)."""
    S = particles["S"]
    idx = np.array([k for k, o in enumerate(S["objects"]) if not o.get("is_light")], np.uint32)
    assert len(idx) == NOBJ - 1
    Ts = np.array([IC.translate(S["objects"][i]["T"], (0.01, 0.0, -0.01)) for i in idx], np.float32)
    ref, dev = make_pt(srt, S), make_pt(srt, S)
    c0, d0 = ref.scene_counts(), dev.scene_counts()
    assert c0 == d0
    ref.repose(idx, Ts)
    device_repose(torch, dev, idx, Ts)
    c1, d1 = ref.scene_counts(), dev.scene_counts()
    device_repose(torch, dev, idx, Ts)
    d2 = dev.scene_counts()
    same = IC.dumps_equal(IC.all_dumps(ref, NOBJ), IC.all_dumps(dev, NOBJ))
    ref.close(); dev.close()
    host_added, first_added, second_added = c1["uploaded_bytes"] - c0["uploaded_bytes"], d1["uploaded_bytes"] - d0["uploaded_bytes"], d2["uploaded_bytes"] - d1["uploaded_bytes"]
    print(f"uploaded per repose of {len(idx)} objects: host form {host_added} B, device form {first_added} B (first), {second_added} B (later)")
    assert same
    for c in (c1, d1, d2):
        assert c["uploaded_triangle_bytes"] == c0["uploaded_triangle_bytes"] > 0 and c["blas_builds"] == c0["blas_builds"] and c["device_bytes"] == c0["device_bytes"]
    assert host_added > 176 * NOBJ
    assert 0 < first_added <= host_added - 128 * len(idx)
    assert 0 < second_added <= host_added - 176 * NOBJ + 8 * NOBJ + 4 * len(idx) and second_added < first_added


def test_refusals_leave_the_scene(srt, torch, particles):
    """Refused lists, a NULL array, and poses whose BVH<Object> build does not terminate (every listed particle at one point; the
    host build at this size gives the verdict): status and message as srt_pt_repose's, trees and image unchanged - and the next
    device repose works."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    light = [k for k, o in enumerate(S["objects"]) if o.get("is_light")][0]
    pt = make_pt(srt, S)
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    first = particles["first"]
    cases = [("area light", [int(idx[0]), light], INVALID), ("listed twice", [int(idx[1]), int(idx[1])], INVALID), ("out of range", [NOBJ, int(idx[1])], INVALID)]
    for match, bad, status in cases:
        with pytest.raises(srt.SrtError, match=match) as e:
            pt.repose_device(bad, d.data_ptr())
        assert e.value.status == status and "srt_pt_repose_device" in str(e.value)
        assert IC.dumps_equal(IC.all_dumps(pt, NOBJ), first["dumps"]), match
    with pytest.raises(srt.SrtError, match="NULL argument") as e:
        pt.repose_device(idx, 0)
    assert e.value.status == INVALID
    stuck_idx = idx[1:11]
    stuck = np.tile(Ts[1], (len(stuck_idx), 1))
    with pytest.raises(srt.SrtError, match="does not terminate") as e:
        device_repose(torch, pt, stuck_idx, stuck)
    assert e.value.status == UNSUPPORTED
    counts = pt.scene_counts()
    after = computed(pt, NOBJ, W, HT, SPP, (0,))
    assert_same(after, dict(first, epochs={0: first["epochs"][0]}), "after the refusals")
    # the same refusal after a device repose that went through: the tables the kernels keep are then in use
    device_repose(torch, pt, idx, Ts)
    with pytest.raises(srt.SrtError, match="does not terminate"):
        device_repose(torch, pt, stuck_idx, stuck)
    got = computed(pt, NOBJ, W, HT, SPP, (0,))
    device_repose(torch, pt, idx, particles["home"])
    back = computed(pt, NOBJ, W, HT, SPP, (0,))
    pt.close()
    assert counts["uploaded_triangle_bytes"] > 0
    assert_same(got, dict(particles["moved"], epochs={0: particles["moved"]["epochs"][0]}), "a repose, then a refusal")
    assert_same(back, dict(first, epochs={0: first["epochs"][0]}), "back")


def test_stream_order(srt, torch, particles):
    """d_trans is produced by torch ops on a stream of the caller's, behind work that keeps the stream busy; repose_device gets the
    stream's handle and nothing synchronises in between."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    pt = make_pt(srt, S)
    half = on_device(torch, Ts * np.float32(0.5))
    busy = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        for _ in range(8):
            busy = busy @ busy * 1e-4
        d = half + half                                   # exact: Ts again
        pt.repose_device(idx, d.data_ptr(), st.cuda_stream)
    got = computed(pt, NOBJ, W, HT, SPP, (0,))
    pt.close()
    assert bits_equal(d.cpu().numpy(), Ts)
    assert_same(got, dict(particles["moved"], epochs={0: particles["moved"]["epochs"][0]}))


def test_particle_loop(srt, torch, particles):
    """positions -> particle_transforms_device -> repose_device: the transforms are mat_mul(translate, scale) bit for bit, the scene
    is srt_pt_repose's; then one Particle::update step and the same again: the scene of a fresh commit on the moved particles."""
    S = particles["S"]
    pidx = np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + IC.PARTICLE_COUNT, dtype=np.uint32)
    pos = RC.particle_positions(S)
    ref, dev = make_pt(srt, S), make_pt(srt, S)

    def transforms(p):
        d_pos = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to("cuda:0")
        d_T = torch.full((len(p), 16), float("nan"), device="cuda:0")
        torch.cuda.synchronize()
        dev.particle_transforms_device(d_pos.data_ptr(), len(p), RC.PARTICLE_SCALE, d_T.data_ptr())
        return d_T                                        # (enqueued on the null stream, where repose_device reads it)

    d_T = transforms(pos)
    dev.repose_device(pidx, d_T.data_ptr())
    want_T = RC.translate_scale_product(pos, RC.PARTICLE_SCALE)
    assert bits_equal(d_T.cpu().numpy(), want_T)
    ref.repose(pidx, want_T)
    assert_same(computed(dev, NOBJ, W, HT, SPP, (0,)), computed(ref, NOBJ, W, HT, SPP, (0,)), "the committed positions")
    # one step (the host form of the step kernel: it is not under test), the new positions up, and round again
    rng = np.random.default_rng(8)
    vel = ((rng.random((len(pos), 3)) - 0.5) * 2.0).astype(np.float32)
    age = np.full(len(pos), 10.0, np.float32)
    moved = dev.particles_step(pos, vel, age, 0.01, 0.015)[0]
    assert not bits_equal(moved, pos)
    d_T = transforms(moved)
    dev.repose_device(pidx, d_T.data_ptr())
    moved_T = RC.translate_scale_product(moved, RC.PARTICLE_SCALE)
    assert bits_equal(d_T.cpu().numpy(), moved_T)
    fresh = make_pt(srt, IC.with_poses(S, pidx, moved_T))
    assert_same(computed(dev, NOBJ, W, HT, SPP, (0,)), computed(fresh, NOBJ, W, HT, SPP, (0,)), "a fresh commit on the moved particles")
    for pt in (ref, dev, fresh):
        pt.close()


def test_group(srt, torch, particles):
    """A two-rank PathtracerGroup on one device: repose_device reaches both members (they share the array) and the image is the
    single context's."""
    S, idx, Ts = particles["S"], particles["idx"], particles["Ts"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    first = grp.render_epoch(SEED, 0, SPP)
    d = on_device(torch, Ts)
    torch.cuda.synchronize()
    grp.repose_device(idx, [d.data_ptr(), d.data_ptr()])
    moved = grp.render_epoch(SEED, 0, SPP)
    dumps = [IC.all_dumps(m, NOBJ) for m in grp.members]
    with pytest.raises(ValueError):
        grp.repose_device(idx, [d.data_ptr()])
    grp.close()
    assert bits_equal(first, particles["first"]["epochs"][0]) and bits_equal(moved, particles["moved"]["epochs"][0])
    assert all(IC.dumps_equal(x, particles["moved"]["dumps"]) for x in dumps)
