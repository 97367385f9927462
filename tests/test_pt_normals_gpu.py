"""GPU: the normal-colors debug view (srt_pt_set_normal_colors; the reference's debug_data.normal_colors,
student/pathtracer.cpp:199) through every render entry point.

Expected values come from tests/_normals_expected.py: SRT-RNG v1's first two draws, Camera::generate_ray and Ray::transform
restated in float32, the oracle's scene.hit (pinned to the reference build) and Spectrum::direction on the hit's normal; a camera
ray that leaves the scene takes what the oracle's ordinary render returns for the same sample.  tests/test_pt_normals_host.py
checks the helper's rays against rays the reference build logged.  Every comparison is on the float bits, NaN positions included."""
import ctypes
import os

import numpy as np
import pytest

import _harness as H
import _normals_expected as N
from _cases import pt_scene

pytestmark = pytest.mark.gpu

SEED = 11
NORMALS_FORM = -3                                   # srt_pt_kernel_form while the switch is on (include/srt_pt_debug.h)
_SCENES, _ORACLES, _EPOCHS = {}, {}, {}


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def zero_normal_scene():
    """The Cornell walls plus one quad facing the camera whose two triangles carry all-zero vertex normals.  No object transform:
    Trace::normal is the interpolated vertex normal itself, (0, 0, 0), and Spectrum::direction divides 0 by 0."""
    import srt_amd  # noqa: F401
    from soft_rendering_toolsets_amd import scenes

    s = scenes.cornell_box("cbox_lambertian")
    s["objects"] = s["objects"][:5]
    pos = np.array([[-0.3, 0.2, 0], [0.3, 0.2, 0], [0.3, 0.8, 0], [-0.3, 0.2, 0], [0.3, 0.8, 0], [-0.3, 0.8, 0]], np.float32)
    s["objects"].append({"kind": "mesh", "pos": pos, "nrm": np.zeros((6, 3), np.float32), "idx": np.arange(6, dtype=np.uint32),
                         "T": np.eye(4, dtype=np.float32).reshape(16), "material": 2, "is_light": False})
    s["name"] = "walls+zero_normal_quad"
    return s


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = zero_normal_scene() if name == "zero_normals" else pt_scene(name)
    return _SCENES[name]


def oracle_of(name, w, h, use_bvh=True):
    key = (name, w, h, use_bvh)
    if key not in _ORACLES:
        _ORACLES[key] = H.OraclePT(scene_of(name), w, h, 4, use_bvh)
    return _ORACLES[key]


def expected_epoch(name, w, h, base, n, use_bvh=True):
    """(per-sample radiance [n, h, w, 3], epoch image [h, w, 3]) of the view; computed once per case and shared."""
    key = (name, w, h, base, n, use_bvh)
    if key not in _EPOCHS:
        per, img = N.expected_epoch(oracle_of(name, w, h, use_bvh), scene_of(name), w, h, SEED, base, n)
        per.setflags(write=False); img.setflags(write=False)
        _EPOCHS[key] = (per, img)
    return _EPOCHS[key]


def context(srt, name, w, h, use_bvh=True, depth=4):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, use_bvh)
    pt.build_scene(scene_of(name))
    pt.set_camera(scene_of(name)["camera"])
    return pt


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def differing(a, b):
    return int((bits(a) != bits(b)).any(axis=-1).sum())


# the case tests 3, 4, 6, 8 and 9 share: 2 x 2 tiles of 32 x 32 with padding in the last column and row, a real BVH<Triangle>
E_NAME, E_W, E_H, E_BASE, E_N = "cbox_blob512_glass", 48, 40, 3, 5


# ---- 1. per sample, every pixel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,use_bvh", [("cbox", False), ("cbox", True), ("cbox_blob512_glass", True), ("cbox_envmap", True),
                                          ("cbox_envhemi", True), ("cbox_envsphere", True), ("cbox_nolight", True)])
def test_every_sample_of_every_pixel(srt, name, use_bvh):
    w, h = 32, 24
    ys, xs = (a.reshape(-1).astype(np.uint32) for a in np.mgrid[0:h, 0:w])
    pt = context(srt, name, w, h, use_bvh)
    pt.set_normal_colors(True)
    for s in (0, 1, 63, 64, (1 << 28) - 1):
        ss = np.full(w * h, s, np.uint32)
        want, hit = N.expected_samples(oracle_of(name, w, h, use_bvh), scene_of(name), w, h, SEED, xs, ys, ss)
        assert hit.any() and (~hit).any(), f"{name}: the frame needs both hits and misses ({hit.sum()} hits of {hit.size})"
        if "env" in name:
            assert (want[~hit] != 0).any(), "the environment light shows where the camera ray leaves the scene"
        else:
            assert (want[~hit] == 0).all()
        rgb, draws, rays = pt.trace_samples(SEED, xs, ys, ss)
        assert np.array_equal(bits(rgb), bits(want)), f"{name}, BVH {use_bvh}, sample {s}: {differing(rgb, want)} of {w * h} samples differ"
        assert (draws == 2).all() and (rays == 1).all()
    pt.close()


# ---- 2. invalid samples --------------------------------------------------------------------------------------------------
def test_zero_normals_are_dropped_as_invalid_samples(srt):
    w, h, n = 16, 16, 3
    per, want = expected_epoch("zero_normals", w, h, 0, n)
    on_quad = np.isnan(per).all(axis=-1)                                     # [n, h, w]
    always = on_quad.all(axis=0)
    assert always.sum() >= 8 and not np.isnan(per[:, ~on_quad.any(axis=0)]).any(), "the quad covers some pixels in all three samples"
    assert (want[always] == 0).all() and (want[~always] != 0).any()
    pt = context(srt, "zero_normals", w, h)
    pt.set_normal_colors(True)
    ys, xs = (a.reshape(-1).astype(np.uint32) for a in np.mgrid[0:h, 0:w])
    rgb = pt.trace_samples(SEED, xs, ys, np.zeros(w * h, np.uint32))[0].reshape(h, w, 3)
    assert np.array_equal(np.isnan(rgb), np.isnan(per[0])) and np.isnan(rgb[on_quad[0]]).all(), "0 / 0 in every channel on the quad"
    got = pt.render_epoch(SEED, 0, n)
    assert (bits(got[always]) == 0).all(), "a pixel with no valid sample is exactly zero"
    assert np.array_equal(bits(got), bits(want)), f"{differing(got, want)} pixels differ from the valid mean"
    pt.close()


# ---- 3. epoch mean and padding --------------------------------------------------------------------------------------------
def test_epoch_is_the_in_order_valid_mean(srt):
    _, want = expected_epoch(E_NAME, E_W, E_H, E_BASE, E_N)
    pt = context(srt, E_NAME, E_W, E_H)
    pt.set_normal_colors(True)
    got = pt.render_epoch(SEED, E_BASE, E_N)
    assert np.array_equal(bits(got), bits(want)), f"{differing(got, want)} of {E_W * E_H} pixels differ"
    pt.close()


# ---- 4. form independence ------------------------------------------------------------------------------------------------
def test_every_kernel_mode_takes_the_same_kernel(srt):
    _, want = expected_epoch(E_NAME, E_W, E_H, E_BASE, E_N)
    pt = context(srt, E_NAME, E_W, E_H)
    ordinary = {}
    for mode in (0, 1, 4, 6, 7):                                             # (the scene has one mesh with a real BVH<Triangle>: 7 applies)
        pt.set_kernel(mode)
        ordinary[mode] = pt.kernel_form()
        pt.set_normal_colors(True)
        assert pt.kernel_form() == NORMALS_FORM
        got = pt.render_epoch(SEED, E_BASE, E_N)
        assert np.array_equal(bits(got), bits(want)), f"kernel mode {mode}: {differing(got, want)} pixels differ"
        pt.set_normal_colors(False)
        assert pt.kernel_form() == ordinary[mode]
    assert NORMALS_FORM not in ordinary.values() and len(set(ordinary.values())) >= 4
    pt.close()


# ---- 5. the fold path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_launches_fold_into_the_reference_epochs(srt, mode):
    """Launches of 3 and 4 samples folded with samples_per_epoch 2, total 7: after the first, one epoch and a dangling half that
    stays invisible; after the second, three whole epochs and the short last one.  Mode 1 keeps no per-sample radiance in an
    ordinary render; the view's kernel always does."""
    import torch

    name, w, h, spe, total = "cbox", 40, 28, 2, 7
    per, _ = expected_epoch(name, w, h, 0, total)
    means = H.oracle_running_means(lambda s, n: N.valid_mean(per[s:s + n]), total, spe, shape=(h, w, 3))
    assert len(means) == 5
    pt = context(srt, name, w, h)
    pt.set_kernel(mode)
    pt.set_normal_colors(True)
    stream = torch.cuda.current_stream().cuda_stream
    _, per_rank, fpt = pt.tile_info()
    acc = torch.zeros(pt.accumulator_floats(), dtype=torch.float32, device="cuda")
    tiles = torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda")
    image = torch.zeros(w * h * 3, dtype=torch.float32, device="cuda")
    pos = 0
    for n in (3, 4):
        pt.render_samples_device(stream, SEED, pos, n)
        pt.fold_epochs_device(stream, spe, pos, total, 0, acc.data_ptr())
        pos += n
        pt.accumulator_tiles_device(stream, acc.data_ptr(), tiles.data_ptr())
        pt.untile_device(stream, tiles.data_ptr(), image.data_ptr())
        torch.cuda.synchronize()
        got = image.cpu().numpy().reshape(h, w, 3)
        k = H.epochs_through(pos, total, spe)
        assert np.array_equal(bits(got), bits(means[k])), f"mode {mode}: after {pos} samples {differing(got, means[k])} pixels differ from {k} epochs"
    pt.close()


# ---- 6. bookkeeping -------------------------------------------------------------------------------------------------------
def test_one_ray_per_camera_sample_and_an_empty_ray_log(srt):
    pt = context(srt, E_NAME, E_W, E_H)
    pt.set_ray_log(1024)
    pt.set_normal_colors(True)
    pt.ray_count(reset=True)
    pt.rays_elided(reset=True)
    pt.render_epoch(SEED, E_BASE, E_N)
    assert pt.ray_count() == (E_W * E_H * E_N, E_W * E_H * E_N)
    assert pt.rays_elided() == 0
    rays, dropped = pt.read_ray_log()
    assert len(rays) == 0 and dropped == 0
    pt.close()


# ---- 7. the switch leaves nothing behind ----------------------------------------------------------------------------------
def test_ordinary_renders_around_the_view_are_untouched(srt):
    name, w, h, spp = "cbox", 32, 32, 4
    fresh = context(srt, name, w, h, depth=8)
    want = fresh.render_epoch(SEED, 0, spp)
    fresh.close()
    pt = context(srt, name, w, h, depth=8)
    first = pt.render_epoch(SEED, 0, spp)
    pt.set_normal_colors(True)
    view = pt.render_epoch(SEED, 0, spp)
    pt.set_normal_colors(False)
    third = pt.render_epoch(SEED, 0, spp)
    assert np.array_equal(bits(view), bits(expected_epoch(name, w, h, 0, spp)[1]))
    assert differing(view, first) > w * h // 4, "the view is not the ordinary render"
    assert np.array_equal(bits(first), bits(third)) and np.array_equal(bits(first), bits(want))
    pt.close()


# ---- 8. tiling and group --------------------------------------------------------------------------------------------------
def test_a_shard_writes_only_its_tiles(srt):
    _, want = expected_epoch(E_NAME, E_W, E_H, E_BASE, E_N)
    pt = context(srt, E_NAME, E_W, E_H)
    pt.set_tiling(32, 32, 1, 3)                                              # tiles 0..3 dealt to 3 ranks: rank 1 owns tile 1 only
    pt.set_normal_colors(True)
    out = np.full((E_H, E_W, 3), -7.0, np.float32)
    pt.render_epoch(SEED, E_BASE, E_N, out)
    mine = np.zeros((E_H, E_W), bool)
    mine[0:32, 32:48] = True
    assert np.array_equal(bits(out[mine]), bits(want[mine])), f"{differing(out[mine], want[mine])} pixels of rank 1's tile differ"
    assert (out[~mine] == -7.0).all(), "pixels of other ranks' tiles were written"
    assert pt.ray_count() == (16 * 32 * E_N, 16 * 32 * E_N)
    pt.close()


def test_group_of_two_logical_ranks_equals_the_single_context(srt):
    _, want = expected_epoch(E_NAME, E_W, E_H, E_BASE, E_N)
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(E_W, E_H, E_N, 4, True)
    grp.build_scene(scene_of(E_NAME))
    grp.set_camera(scene_of(E_NAME)["camera"])
    grp.set_normal_colors(True)
    assert all(m.kernel_form() == NORMALS_FORM for m in grp.members)
    for k in range(2):                                                       # twice: the second epoch reuses the exchange buffers
        grp.ray_count(reset=True)
        got = grp.render_epoch(SEED, E_BASE, E_N)
        assert np.array_equal(bits(got), bits(want)), f"epoch {k}: {differing(got, want)} pixels differ"
        assert grp.ray_count() == (E_W * E_H * E_N, E_W * E_H * E_N)
    d, s = grp.render_epoch_lane(1, SEED, E_BASE, E_N)                       # a second lane: its own streams and buffers
    import torch

    torch.cuda.synchronize()
    lane = np.zeros((E_H, E_W, 3), np.float32)
    L = grp._lib
    assert L.hipMemcpyAsync(lane.ctypes.data_as(ctypes.c_void_p), d, lane.nbytes, 2, s) == 0 and L.hipStreamSynchronize(s) == 0
    assert np.array_equal(bits(lane), bits(want))
    grp.close()


# ---- 9. cancel ------------------------------------------------------------------------------------------------------------
def test_cancel_and_clear(srt):
    _, want = expected_epoch(E_NAME, E_W, E_H, E_BASE, E_N)
    pt = context(srt, E_NAME, E_W, E_H)
    pt.set_normal_colors(True)
    pt.cancel_device()
    with pytest.raises(srt.SrtCancelled):
        pt.render_epoch(SEED, E_BASE, E_N)
    pt.clear_cancel()
    got = pt.render_epoch(SEED, E_BASE, E_N)
    assert np.array_equal(bits(got), bits(want)), f"{differing(got, want)} pixels differ after clear_cancel"
    pt.close()


# ---- 10. the class --------------------------------------------------------------------------------------------------------
DROPIN_PT_FULL = os.path.join(H.ROOT, "integration", "_build", "libdropin_pt_full.so")


def test_the_class_follows_the_reference_debug_box(srt):
    """PT::Pathtracer inside the reference's scene layer: the harness ticks the reference's own debug_data.normal_colors, the
    class reads it in begin_render.  Expected: the running mean of the helper's epochs under the class's epoch scheme
    (samples_per_epoch = max(1, samples / (threads * 10)), rays/pathtracer.cpp:250-256); with the box cleared, the ordinary render."""
    if not os.path.exists(DROPIN_PT_FULL):
        pytest.skip("integration/_build/libdropin_pt_full.so is built in the authoring container (make -C integration)")
    srt.load_library()
    lib = ctypes.CDLL(DROPIN_PT_FULL)
    variant, w, h, depth, samples, threads = 3, 32, 32, 4, 23, 1              # variant 3: the Cornell box alone; 11 epochs of 2 samples and a short one
    cam = np.zeros(18, np.float32)
    dump = np.zeros(8 << 20, np.uint8)
    n = ctypes.c_uint64(0)

    def render():
        rgb = np.zeros((h, w, 3), np.float32)
        rc = lib.dropin_pt_full_render(variant, w, h, samples, 0, depth, 1, threads, H.P(rgb), H.P(cam), H.P(dump), ctypes.c_uint64(dump.size),
                                       ctypes.byref(n))
        assert rc == 0
        return rgb

    assert lib.dropin_pt_full_set_normal_colors(0) == 0, "the reference's box starts cleared"
    before = render()
    assert lib.dropin_pt_full_set_normal_colors(1) == 0
    try:
        view = render()
    finally:
        assert lib.dropin_pt_full_set_normal_colors(0) == 1
    after = render()
    scene = H.parse_scene_dump(dump[: n.value].tobytes())
    scene["camera"] = {"iview": cam[:16].copy(), "vfov": float(cam[16]), "ar": float(cam[17])}
    o = H.OraclePT(scene, w, h, depth, True)
    spe = max(1, samples // (threads * 10))
    per, _ = N.expected_epoch(o, scene, w, h, 0, 0, samples)                   # the class's seed is 0
    want_view = H.oracle_running_means(lambda s, k: N.valid_mean(per[s:s + k]), samples, spe, shape=(h, w, 3))[-1]
    assert np.array_equal(bits(view), bits(want_view)), f"{differing(view, want_view)} pixels of the view differ"
    want = H.oracle_running_means(lambda s, k: o.epoch(0, s, k), samples, spe, shape=(h, w, 3))[-1]
    assert np.array_equal(bits(before), bits(want)), f"{differing(before, want)} pixels of the ordinary render differ from the oracle"
    assert np.array_equal(bits(after), bits(before)), "with the box cleared again the class renders as before"
    lib.dropin_pt_full_logged_rays.restype = ctypes.c_uint64
    lib.dropin_pt_full_logged_rays(None, ctypes.c_uint64(0))                  # (empty the harness's ray log for whoever comes next)
