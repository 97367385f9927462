"""GPU: Env_Map's importance sampler (srt_pt_set_env_sampling("image"); Samplers::Sphere::Image, student/samplers.cpp:27-137) on the
device - the probes and the device tables against the component fixture, every kernel form that takes an environment map against
the path fixture recorded from the reference's path tracer with its image sampler switched on (tests/golden/make_env_image_golden.py),
and the switch's life on a committed context."""
import ctypes
import os

import numpy as np
import pytest

import _env_image_cases as E
import _harness as H
from _cases import pt_scene

pytestmark = pytest.mark.gpu
ENV_MAP_MODES = (0, 1, 2, 4, 6)          # srt_pt_set_kernel values that take an environment map (tests/test_pt_gpu.py::test_environment_map)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def components():
    return H.load_golden("env_image_components.npz")


@pytest.fixture(scope="module")
def paths():
    return H.load_golden("env_image_paths.npz")


def make_pt(srt, scene, w=E.W, h=E.H, depth=E.DEPTH):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, True)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def scene_with_map(img):
    s = pt_scene("cbox_envonly")
    s["env"] = {"type": 3, "image": img}
    return s


@pytest.mark.parametrize("name", list(E.MAPS))
def test_probe_and_device_tables_equal_the_reference(srt, components, name):
    g, img = components, E.env_map(name)
    pt = make_pt(srt, scene_with_map(img))
    assert pt.env_sampling() == "uniform"                    # the probes do not ask for the mode
    dev, host = pt.dump_env_sampler(from_device=True), pt.dump_env_sampler(from_device=False)
    assert (dev["w"], dev["h"]) == (img.shape[1], img.shape[0])
    assert bits_equal(dev["cdf"], g[f"{name}.cdf"]) and bits_equal(dev["pdf"], g[f"{name}.pdf"]) and bits_equal(dev["total"], np.float32(g[f"{name}.total"]))
    want = dict(zip(("sin_theta", "cos_theta", "cos_phi", "sin_phi"), E.trig_tables(img.shape[1], img.shape[0])))
    for k in want:                                           # the test's own restatement (libm), not the library's host copy
        assert bits_equal(dev[k], want[k]) and bits_equal(host[k], want[k]), k
    index, sample, pdf = pt.env_sampler_probe(g[f"{name}.u"], g[f"{name}.dirs"])
    assert np.array_equal(index, g[f"{name}.index"])
    assert bits_equal(sample, g[f"{name}.sample"])
    assert bits_equal(pdf, g[f"{name}.pdf_of"])
    pt.close()


def test_device_sin_unit_equals_the_host_restatement(srt):
    emu = ctypes.CDLL(H.build_host_lib("env_image_host", ["env_image_host.cpp"], scene_layer=True))
    x = E.sin_unit_arguments()
    host, libm = np.zeros(len(x), np.float64), np.zeros(len(x), np.float64)
    assert emu.emu_sin_unit(H.P(x), ctypes.c_size_t(len(x)), H.P(host), H.P(libm)) == 0
    pt = srt.Pathtracer(0)
    got = pt.math_sin_unit(x)
    pt.close()
    assert bits_equal(got, host)


@pytest.mark.parametrize("name", list(E.PATH_SCENES))
def test_every_kernel_form_equals_the_reference(srt, paths, name):
    """trace_samples' radiance and draw ledger, and the 6-spp epoch image under every kernel mode that takes a map, bit for bit; the
    ray count is the same under every mode; the forms that refuse environment lights still do."""
    g = paths
    pt = make_pt(srt, E.path_scene(name))
    pt.set_env_sampling("image")
    assert pt.env_sampling() == "image"
    xs, ys, ss = E.sample_list()
    rgb, draws, _ = pt.trace_samples(E.SEED, xs, ys, ss)
    assert np.array_equal(draws, g[f"{name}.draws"]), "the draw ledger differs from the reference's"
    assert bits_equal(rgb, g[f"{name}.rgb"]), "per-sample radiance differs from the reference's"
    rays = set()
    for mode in ENV_MAP_MODES:
        pt.set_kernel(mode)
        pt.ray_count(reset=True)
        img = pt.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP)
        assert bits_equal(img, g[f"{name}.epoch"]), f"kernel mode {mode}"
        rays.add(pt.ray_count()[0])
    assert len(rays) == 1, rays
    for mode in (3, 5):
        pt.set_kernel(mode)
        with pytest.raises(srt.SrtError):
            pt.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP)
    pt.close()


def test_image_uniform_image_on_one_context(srt, paths):
    """The mode is a launch parameter: on one committed context image -> uniform -> image gives the new fixture, the existing
    uniform golden (tests/golden/pt_cbox_envmap_40x32_d8_bvh.npz: its epoch image), and the new fixture again."""
    old = H.load_golden("pt_cbox_envmap_40x32_d8_bvh.npz")
    ow, oh, ospp, obase = (int(x) for x in old["epoch_meta"])
    odepth, oseed = int(old["meta"][2]), int(old["seed"])
    pt = make_pt(srt, E.path_scene("cbox_envmap"))
    uploaded = pt.scene_counts()
    for mode in ("image", "uniform", "image"):
        pt.set_env_sampling(mode)
        if mode == "image":
            pt.set_params(E.W, E.H, E.EPOCH_SPP, E.DEPTH, True)
            assert bits_equal(pt.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP), paths["cbox_envmap.epoch"]), mode
        else:
            pt.set_params(ow, oh, ospp, odepth, True)
            assert bits_equal(pt.render_epoch(oseed, obase, ospp), old["epoch"]), mode
    assert pt.scene_counts() != uploaded, "the tables' upload is counted"
    pt.close()


def test_mode_off_uploads_and_allocates_nothing(srt):
    """With the mode off - never set, or set and taken back before a launch - the upload counters and the live resources are those of a
    context that knows nothing of the switch."""
    from soft_rendering_toolsets_amd._pt_bindings import live_resources

    scene = E.path_scene("cbox_envmap")
    a = make_pt(srt, scene)
    a.render_epoch(E.SEED, 0, 2)
    counts, live = a.scene_counts(), live_resources()
    a.close()
    b = make_pt(srt, scene)
    b.set_env_sampling("image")
    b.set_env_sampling("uniform")
    b.render_epoch(E.SEED, 0, 2)
    assert b.scene_counts() == counts and live_resources() == live
    b.close()


def test_a_new_map_rebuilds_the_tables(srt, paths, components):
    pt = make_pt(srt, E.path_scene("cbox_envmap"))
    pt.set_env_sampling("image")
    pt.set_params(E.W, E.H, E.EPOCH_SPP, E.DEPTH, True)
    assert bits_equal(pt.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP), paths["cbox_envmap.epoch"])
    second = E.path_scene("cbox_envonly_sun")
    pt.build_scene(second)                                    # srt_pt_scene_begin ... srt_pt_set_env_map ... commit, the mode still on
    pt.set_camera(second["camera"])
    assert bits_equal(pt.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP), paths["cbox_envonly_sun.epoch"])
    assert bits_equal(pt.dump_env_sampler(from_device=True)["cdf"], components["sun16x8.cdf"])
    pt.close()


@pytest.mark.parametrize("name,what", [("cbox", "no environment light"), ("cbox_envsphere", "a uniform sphere"), ("cbox_envhemi", "a uniform hemisphere")])
def test_image_mode_without_a_map_is_refused_by_the_launch(srt, name, what):
    scene = pt_scene(name)
    pt = make_pt(srt, scene, 16, 16, 4)
    pt.set_env_sampling("image")                              # stored: the call itself does not look at the scene
    with pytest.raises(srt.SrtError, match="needs an environment map") as err:
        pt.render_epoch(1, 0, 1)
    assert what in str(err.value)
    with pytest.raises(srt.SrtError, match="needs an environment map"):
        pt.trace_samples(1, [0], [0], [0])
    with pytest.raises(ValueError):
        pt.set_env_sampling("cosine")
    pt.set_env_sampling("uniform")
    pt.render_epoch(1, 0, 1)
    pt.close()


def test_group_of_one_rank_equals_the_single_context(srt, paths):
    scene = E.path_scene("cbox_envmap")
    grp = srt.PathtracerGroup([0])
    grp.set_params(E.W, E.H, E.EPOCH_SPP, E.DEPTH, True)
    grp.build_scene(scene)
    grp.set_camera(scene["camera"])
    grp.set_env_sampling("image")
    assert all(m.env_sampling() == "image" for m in grp.members)
    assert bits_equal(grp.render_epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP), paths["cbox_envmap.epoch"])
    grp.close()


DROPIN_PT_FULL = os.path.join(H.ROOT, "integration", "_build", "libdropin_pt_full.so")


def test_the_class_samples_through_the_image_sampler(srt):
    """PT::Pathtracer::set_env_image_sampling inside the reference's scene layer (integration/harness/pt_full.cpp, scene variant 4: a
    sphere light with an emissive map, i.e. an Env_Map): the class's render equals the C interface's on the same scene under the same
    mode - the running mean of its epochs (samples_per_epoch = max(1, samples / (threads * 10)), rays/pathtracer.cpp:250-256) - and
    with the setter off again the uniform render.  (A scene without a map under the mode ends in the class's die(), as every refused
    call does there; the refusal itself is test_image_mode_without_a_map_is_refused_by_the_launch's.)"""
    if not os.path.exists(DROPIN_PT_FULL):
        pytest.skip("integration/_build/libdropin_pt_full.so is built in the authoring container (make -C integration)")
    srt.load_library()
    lib = ctypes.CDLL(DROPIN_PT_FULL)
    variant, w, h, depth, samples, threads = 4, 32, 24, 5, 23, 1              # 11 epochs of 2 samples and a short one
    cam, dump, n = np.zeros(18, np.float32), np.zeros(8 << 20, np.uint8), ctypes.c_uint64(0)

    def render():
        rgb = np.zeros((h, w, 3), np.float32)
        assert lib.dropin_pt_full_render(variant, w, h, samples, 0, depth, 1, threads, H.P(rgb), H.P(cam), H.P(dump), ctypes.c_uint64(dump.size),
                                         ctypes.byref(n)) == 0
        return rgb

    assert lib.dropin_pt_full_set_env_image_sampling(1) == 0, "the setter starts off"
    try:
        image = render()
    finally:
        assert lib.dropin_pt_full_set_env_image_sampling(0) == 1
    uniform = render()
    dims = (ctypes.c_uint32 * 2)()
    assert lib.dropin_pt_full_env_map(dims, None, ctypes.c_uint64(0)) == 0
    env = np.zeros((dims[1], dims[0], 3), np.float32)
    assert lib.dropin_pt_full_env_map(dims, H.P(env), ctypes.c_uint64(env.size)) == 0
    scene = H.parse_scene_dump(dump[: n.value].tobytes())
    assert "env" not in scene, "the dump has no record for an Env_Map"
    scene["env"] = {"type": 3, "image": env}
    scene["camera"] = {"iview": cam[:16].copy(), "vfov": float(cam[16]), "ar": float(cam[17])}
    pt = make_pt(srt, scene, w, h, depth)
    spe = max(1, samples // (threads * 10))
    for mode, got in (("image", image), ("uniform", uniform)):
        pt.set_env_sampling(mode)
        want = H.oracle_running_means(lambda s, k: pt.render_epoch(0, s, k), samples, spe, shape=(h, w, 3))[-1]   # the class's seed is 0
        assert bits_equal(got, want), f"the class's {mode} render differs from the C interface's"
    assert not bits_equal(image, uniform)
    pt.close()
    lib.dropin_pt_full_logged_rays.restype = ctypes.c_uint64
    lib.dropin_pt_full_logged_rays(None, ctypes.c_uint64(0))                  # (empty the harness's ray log for whoever comes next)
