"""GPU: every kernel form's traversal stack at depth.  The scenes are the skewed trees of tests/_cases.py (deep_*): a mesh whose
BVH<Triangle> nests 16 (deep_mid) or 48 = kMaxBlasDepth (deep_max) interior nodes, a BVH<Object> that nests 22 (deep_tlas), and
both limits at once (deep_both: 24 + 48 = kFlatStack frames).  tests/test_pt_stack_depth_host.py shows on the CPU that every
camera ray of these renders walks to the bottom of the trees, i.e. that the frames checked here - the private arrays of the
nested walks (modes 1, 4), stack[kFlatStack] of the flattened walk (mode 5), the LDS frames and the per-lane spill columns of
the streamed ray-cast kernel (modes 6, 7) on both sides of every SRT_CAST_LDS_FRAMES boundary - are really written and read back.
Every image is compared bit for bit with the oracle's."""
import functools

import numpy as np
import pytest

import _harness as H
from _cases import chain_rays, pt_scene

pytestmark = pytest.mark.gpu

W, HGT, SPP, DEPTH, SEED, BASE = 32, 24, 3, 4, 5, 2
FORM_OF_MODE = {1: -2, 4: -1, 5: 2, 6: 3, 7: 4}          # srt_pt_kernel_form of each srt_pt_set_kernel mode on a scene with a real mesh


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return pt_scene(name)


@functools.lru_cache(maxsize=None)
def oracle_image(name, camera="camera"):
    """The oracle's epoch image of the scene, computed once per session and shared (read-only)."""
    scene = dict(scene_of(name))
    scene["camera"] = scene[camera]
    img = H.OraclePT(scene, W, HGT, DEPTH, True).epoch(SEED, BASE, SPP)
    img.setflags(write=False)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > W * HGT // 4, "the reference image is not a flat colour"
    return img


@functools.lru_cache(maxsize=None)
def tree_depths(name):
    """(max_tlas_depth, max_blas_depth) of the host build."""
    emu = H.EmuPT(scene_of(name), True)
    z = np.zeros((1, 3), np.float32)
    _, _, tb = emu.hit_depth(z, z + 1, np.zeros((1, 2), np.float32))
    emu.close()
    return tb


def make_pt(srt, name, camera="camera"):
    scene = scene_of(name)
    pt = srt.Pathtracer(0)
    pt.set_params(W, HGT, SPP, DEPTH, True)
    pt.build_scene(scene)
    pt.set_camera(scene[camera])
    return pt


@pytest.mark.parametrize("name,modes", [("deep_mid", (1, 4, 5, 6, 7)), ("deep_max", (1, 4, 5, 6, 7)), ("deep_tlas", (1, 4, 6)),
                                        ("deep_both", (1, 4, 6))])
def test_every_kernel_form_at_depth(srt, name, modes):
    scene = scene_of(name)
    want = oracle_image(name)
    pt = make_pt(srt, name)
    for mode in modes:
        pt.set_kernel(mode)
        assert pt.kernel_form() == FORM_OF_MODE[mode]
        assert bits_equal(pt.render_epoch(SEED, BASE, SPP), want), f"{name}: kernel mode {mode} differs from the oracle"
    # scene.hit records of rays aimed down the chain: through the nested walk and through the flattened one
    org, d, b = chain_rays(7, 3000, scene)
    want_hits = H.OraclePT(scene, W, HGT, DEPTH, True).hit(org, d, b)
    assert int(want_hits[:, 0].sum()) > 2000
    for mode in (0, 5) if len(scene["objects"]) <= 31 else (0,):     # (the flattened walk takes at most 31 objects: deep_both's 28
        pt.set_kernel(mode)                                          #  fill all kFlatStack = 72 frames of its stack)
        assert bits_equal(pt.hit(org, d, b), want_hits), f"{name}: scene.hit (kernel mode {mode}) differs from the oracle"
    if "camera_outside" in scene:                          # the view from in front of the box: walks of every length up to ~40 frames
        want = oracle_image(name, "camera_outside")
        pt.set_camera(scene["camera_outside"])
        for mode in modes:
            pt.set_kernel(mode)
            assert bits_equal(pt.render_epoch(SEED, BASE, SPP), want), f"{name} from outside: kernel mode {mode} differs from the oracle"
    pt.close()


def lds_settings(name, mode):
    """SRT_CAST_LDS_FRAMES values around every boundary: one frame in LDS (everything else spills), two, the mesh's nesting
    (the BVH<Object> part of the stack in LDS, most of the mesh's spilled - or the reverse), all but one of the frames
    render_epoch_stream reserves, all of them, and the kernel's default (13; 10 for mode 7's walk-only build)."""
    t, b = tree_depths(name)
    depth = (t if mode == 6 else 0) + b + 1
    return list(dict.fromkeys([1, 2, b, depth - 1, depth, None]))


@pytest.mark.parametrize("name,mode,settings", [
    ("deep_mid", 6, "all"), ("deep_mid", 7, "all"), ("deep_max", 6, "all"), ("deep_max", 7, "all"),
    ("deep_tlas", 6, (1, None)), ("deep_both", 6, (1, None)),
])
def test_lds_spill_boundary(srt, monkeypatch, name, mode, settings):
    """The launch shape of the ray-cast kernel is derived once per committed scene: a fresh context per setting.  Every setting
    gives the oracle's image (hence the same image as every other setting), with and without dead-ray elision, and with a
    population of 256 path slots, far fewer than the 768 x 3 samples: the spill columns of every wave are in use at once."""
    want = oracle_image(name)
    settings = lds_settings(name, mode) if settings == "all" else settings
    for i, k in enumerate(settings):
        if k is None:
            monkeypatch.delenv("SRT_CAST_LDS_FRAMES", raising=False)
        else:
            monkeypatch.setenv("SRT_CAST_LDS_FRAMES", str(k))
        pt = make_pt(srt, name)
        pt.set_kernel(mode)
        assert pt.kernel_form() == FORM_OF_MODE[mode]
        assert bits_equal(pt.render_epoch(SEED, BASE, SPP), want), f"{name} mode {mode}: SRT_CAST_LDS_FRAMES={k} differs from the oracle"
        if i < 2:                                          # (one frame in LDS: elision; two: the small population)
            if i == 0:
                pt.set_elision(True)
            else:
                pt.set_stream_slots(256)
            assert bits_equal(pt.render_epoch(SEED, BASE, SPP), want), f"{name} mode {mode}: SRT_CAST_LDS_FRAMES={k}, variant {i}, differs from the oracle"
        pt.close()


@pytest.mark.parametrize("mode", [6, 7])
def test_recommit_between_deep_and_shallow_scenes(srt, mode):
    """One context: deep_max, a shallow mesh, deep_max again - the ray-cast kernel's stack depth is derived again after every
    commit and its spill buffer grows back."""
    pt = srt.Pathtracer(0)
    pt.set_params(W, HGT, SPP, DEPTH, True)
    pt.set_kernel(mode)
    for name in ("deep_max", "cbox_blob512_glass", "deep_max"):
        scene = scene_of(name)
        pt.build_scene(scene)
        pt.set_camera(scene["camera"])
        assert pt.kernel_form() == FORM_OF_MODE[mode]
        assert bits_equal(pt.render_epoch(SEED, BASE, SPP), oracle_image(name)), f"mode {mode}: {name} differs from the oracle"
    pt.close()


def test_device_builder_refuses_a_too_deep_tree_cleanly(srt):
    """deep_over's BVH<Triangle> (nesting 49) built on the device is refused at commit like the host build's; the context then
    commits and renders the Cornell box."""
    pt = srt.Pathtracer(0)
    pt.set_params(W, HGT, SPP, DEPTH, True)
    pt.set_bvh_builder(True, 1)
    with pytest.raises(srt.SrtError) as e:
        pt.build_scene(pt_scene("deep_over"))
    assert e.value.status == -4 and "too deep" in str(e.value)
    scene = scene_of("cbox")
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    assert bits_equal(pt.render_epoch(SEED, BASE, SPP), oracle_image("cbox"))
    pt.close()
