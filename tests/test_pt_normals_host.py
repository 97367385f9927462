"""CPU: the normal-colors debug view (srt_pt_set_normal_colors; the reference's debug_data.normal_colors,
student/pathtracer.cpp:199) - everything that can be checked without a GPU.

  * tests/_normals_expected.py, the helper the GPU tests take their expectation from, builds trace_pixel's camera ray (SRT-RNG
    v1's first two draws, Camera::generate_ray, Ray::transform).  The ptlog_* fixtures hold rays the REFERENCE build logged: an
    entry with bounce 0 has the camera ray's hit position as its `point`, so the helper's ray for that (pixel, sample), put
    through the oracle's scene.hit, must give that position bit for bit.
  * Spectrum::direction as the helper restates it.
  * normal_sample() of csrc/pt_trace.h - what the view's kernels run per sample - compiled for the host (tests/host_emu/normals_host.cpp)
    gives the helper's values bit for bit, 2 draws and 1 ray per sample.
  * The C ABI declares, exports and binds the switch.
  * RenderCore forwards it to its group at begin(), before the first launch, and again after a toggle between two renders."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import _harness as H
import _normals_expected as N
from _cases import pt_scene

LIB = os.path.join(H.ROOT, "soft-rendering-toolsets_amd", "lib", "libsrt_hip.so")
PTLOGS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "ptlog_*.npz")))


def test_there_are_four_ray_log_fixtures():
    assert len(PTLOGS) == 4, PTLOGS


@pytest.mark.parametrize("fixture", PTLOGS)
def test_helper_camera_rays_hit_where_the_reference_logged(fixture):
    g = H.load_golden(fixture)
    w, h, depth, use_bvh, spp, base = (int(v) for v in g["meta"])
    seed, scene = int(g["seed"]), pt_scene(str(g["scene"]))
    first = g["bounce"] == 0
    assert first.any(), "the fixture logs no ray at a camera ray's hit"
    pixel, sample = g["pixel"][first].astype(np.int64), g["sample"][first]
    assert (sample >= base).all() and (sample < base + spp).all()
    org, dirs, bounds = N.camera_rays(scene["camera"], w, h, seed, pixel % w, pixel // w, sample)
    t = H.OraclePT(scene, w, h, depth, bool(use_bvh)).hit(org, dirs, bounds)
    assert (t[:, 0] != 0).all(), "a logged camera ray misses the scene"
    assert np.array_equal(np.ascontiguousarray(t[:, 2:5]).view(np.uint32), np.ascontiguousarray(g["point"][first]).view(np.uint32)), \
        "the helper's camera ray does not hit where the reference build's did (a draw, tanf or a fused operation is off)"


def test_direction_restatement():
    d = N.direction([[0, 0, 0], [0, -2, 0], [3, -4, 0], [1e-42, 0, 0], [1e-23, 1e-23, 1e-23]])
    assert np.isnan(d[0]).all(), "a zero normal is 0 / 0 in every channel"
    assert np.array_equal(d[1].view(np.uint32), np.array([0, 1, 0], np.float32).view(np.uint32)), "-0 / 2 = -0, |-0| = +0"
    assert np.array_equal(d[2], np.array([0.6, 0.8, 0.0], np.float32))
    # a denormal vector: x * x underflows to zero, the norm is 0 and the quotient inf or NaN - an invalid sample, not a crash
    assert d[3].shape == (3,) and not np.isfinite(d[3]).all()
    assert d[4].shape == (3,) and not np.isfinite(d[4]).all()
    assert np.array_equal(N.valid_mean(np.stack([d[:3], d[:3]]))[0], np.zeros(3, np.float32)), "a pixel with no valid sample is zero"
    assert np.array_equal(N.valid_mean(np.stack([d[:3], d[:3]]))[1], d[1])


def test_first_two_draws_are_unit_floats():
    a, b = N.first_two_draws(20260404, 1234, (1 << 28) - 1)
    assert a.dtype == np.float32 and 0.0 <= a < 1.0 and 0.0 <= b < 1.0 and a != b


class _EmuNormals(H.EmuPT):
    """normal_sample() of csrc/pt_trace.h compiled for the host (tests/host_emu/normals_host.cpp), one lane at a time."""

    def __init__(self, scene, use_bvh):
        self.lib = ctypes.CDLL(H.build_host_lib("normals_host", ["normals_host.cpp"], scene_layer=True))
        self.lib.emu_create.restype = ctypes.c_void_p
        self.h_ = ctypes.c_void_p(self.lib.emu_create())
        self.use_bvh = use_bvh
        self.scene = scene
        self.feed(scene)

    def samples(self, w, h, seed, xs, ys, ss):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        cam, env = self.scene["camera"], self.scene.get("env")
        iview = np.ascontiguousarray(cam["iview"], np.float32)
        rad = np.ascontiguousarray(env["radiance"], np.float32) if env else np.zeros(3, np.float32)
        rgb, draws, rays = np.zeros((len(xs), 3), np.float32), np.zeros(len(xs), np.uint32), np.zeros(len(xs), np.uint32)
        assert self.lib.emu_normal_samples(self.h_, H.P(iview), ctypes.c_float(cam["vfov"]), ctypes.c_float(cam["ar"]), w, h,
                                           int(env["type"]) if env else 0, H.P(rad), ctypes.c_uint64(seed), H.P(xs), H.P(ys), H.P(ss),
                                           ctypes.c_size_t(len(xs)), H.P(rgb), H.P(draws), H.P(rays)) == 0
        return rgb, draws, rays


@pytest.mark.parametrize("name,use_bvh", [("cbox", False), ("cbox", True), ("cbox_blob512_glass", True), ("cbox_envhemi", True),
                                          ("cbox_envsphere", True)])
def test_device_function_on_the_host_equals_the_helper(name, use_bvh):
    """The kernels' per-sample function, built from the device headers with g++ (no fused operations, as the HIP build), against
    the helper: every pixel of a 32 x 24 frame at the first, a middle and the last sample index; 2 draws and 1 ray per sample."""
    w, h, seed = 32, 24, 11
    scene = pt_scene(name)
    emu = _EmuNormals(scene, use_bvh)
    o = H.OraclePT(scene, w, h, 4, use_bvh)
    ys, xs = (a.reshape(-1).astype(np.uint32) for a in np.mgrid[0:h, 0:w])
    for s in (0, 64, (1 << 28) - 1):
        ss = np.full(w * h, s, np.uint32)
        want, hit = N.expected_samples(o, scene, w, h, seed, xs, ys, ss)
        assert hit.any() and (~hit).any()
        rgb, draws, rays = emu.samples(w, h, seed, xs, ys, ss)
        assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32)), f"{name}, sample {s}: {(rgb.view(np.uint32) != want.view(np.uint32)).any(axis=1).sum()} differ"
        assert (draws == 2).all() and (rays == 1).all()
    emu.close()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    return ctypes.CDLL(LIB)


def test_abi_declares_exports_and_binds_the_switch(lib):
    """As tests/test_abi.py inspects the library: the header's declarations, the shared object's symbols, the bindings."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "srt_pt.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+srt_pt_set_normal_colors\s*\(\s*srt_pt\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+srt_pt_group_set_normal_colors\s*\(\s*srt_pt_group\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    for s in ("srt_pt_set_normal_colors", "srt_pt_group_set_normal_colors"):
        assert hasattr(lib, s), f"{s} is not exported by libsrt_hip.so"
    import srt_amd  # noqa: F401  (loads the package under its importable name)
    from soft_rendering_toolsets_amd import _pt_bindings as B

    B.bind(lib)
    assert lib.srt_pt_set_normal_colors.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert lib.srt_pt_group_set_normal_colors.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert callable(getattr(B.Pathtracer, "set_normal_colors", None)) and callable(getattr(B.PathtracerGroup, "set_normal_colors", None))
    # NULL handles are refused, not dereferenced
    assert lib.srt_pt_set_normal_colors(None, 1) == -1 and lib.srt_pt_group_set_normal_colors(None, 1) == -1      # SRT_ERR_INVALID
    debug = open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()
    assert "-3" in debug and "srt_pt_set_normal_colors" in debug, "srt_pt_kernel_form's new value is documented in srt_pt_debug.h"


def _normals_driver():
    """tests/host_emu/pt_core_normals_driver.cpp + host/pathtracer_core.cpp, built with g++ against the driver's own stand-in ABI."""
    host = os.path.join(H.ROOT, "soft-rendering-toolsets_amd", "host")
    out = H.build_host_lib("pt_core_normals_driver", ["pt_core_normals_driver.cpp", os.path.join(host, "pathtracer_core.cpp")], device_headers=False,
                           extra=("-O1", "-D__HIP_PLATFORM_AMD__", "-I" + host, "-I/opt/rocm/include", "-L/opt/rocm/lib", "-lamdhip64", "-lpthread",
                                  "-Wl,-Bsymbolic", "-Wl,-rpath,/opt/rocm/lib"))
    d = ctypes.CDLL(out)
    d.normals_driver_run.restype = ctypes.c_size_t
    d.normals_driver_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
    return d


@pytest.mark.parametrize("first,second", [(0, 1), (1, 0), (1, 1)])
def test_render_core_forwards_the_switch_at_begin(first, second):
    buf = ctypes.create_string_buffer(1 << 14)
    n = _normals_driver().normals_driver_run(first, second, 100, buf, len(buf))
    assert 0 < n < len(buf)
    calls = buf.value.decode().split("\n")[:-1]
    assert "fatal" not in calls
    begins = [i for i, c in enumerate(calls) if c == "begin"]
    assert len(begins) == 2
    for k, want in enumerate((first, second)):
        part = calls[begins[k]:begins[k + 1] if k == 0 else len(calls)]
        sets = [i for i, c in enumerate(part) if c.startswith("set_normal_colors")]
        launches = [i for i, c in enumerate(part) if c.startswith("render_samples")]
        assert [part[i] for i in sets] == [f"set_normal_colors {want}"], part
        assert [part[i] for i in launches] == ["render_samples 0 64", "render_samples 64 36"], part
        assert sets[0] < launches[0], "the switch reaches the group before the first launch of the render"
        assert [c for c in part if c.startswith("launch_sees")] == [f"launch_sees_normal_colors {want}"] * 2
        assert sum(c == "fold" for c in part) == 2
