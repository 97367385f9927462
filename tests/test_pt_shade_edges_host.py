"""CPU: the shading code at the edges of its parameters (tests/_shade_edge_cases.py) - everything that can be checked without a GPU.

  * tests/golden/refbuild_shade_edges.npz holds what the REFERENCE build computed per sample on every case it runs to the end; the
    oracle, in both math modes, gives the same radiance bits (NaN equal to NaN) and draw counts.  Where oracle/_ref is built the
    reference itself is run again.  So the oracle is a valid yardstick on these scenes, which is what the GPU tests take it for.
  * path_sample() of csrc/pt_trace.h - what the lane-per-sample kernels run - compiled for the host (tests/host_emu/path_host.cpp)
    equals the oracle in radiance, draws and rays on every case, the two the reference aborts on included, and on the named scenes.
  * The reach guard: a case that does not change at least 5 % of the samples of its base scene does not reach its edge.
  * The same emulation as a stand-alone program under AddressSanitizer and UBSan, over every case."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _harness as H
import _shade_edge_cases as E
from _cases import pt_scene, scene_digest

NAMED = ("cbox", "cbox_lambertian", "cbox_refract", "cbox_spherelight", "cbox_nolight", "cbox_deltalights", "cbox_envmap")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def scene_of(name):
    return E.shade_edge_scene(name) if name in E.CASES else pt_scene(name)


_oracle = {}


def oracle_samples(name, base=False):
    """(rgb, draws, rays) of the oracle (SRT-MATH, what the kernels compute) on the cases' sample list; computed once per scene."""
    key = ("base", E.BASE[name]) if base else name
    if key not in _oracle:
        scene = E.base_scene(name) if base else scene_of(name)
        _oracle[key] = H.OraclePT(scene, E.W, E.H, E.DEPTH, True).trace_samples(E.SEED, *E.sample_list())
    return _oracle[key]


def test_the_case_list():
    assert len(E.CASES) == len(set(E.CASES)) == 56 and sorted(sum(E.FAMILIES.values(), [])) == sorted(E.CASES)
    assert set(E.ORACLE_ONLY) <= set(E.CASES) and len(E.REFERENCE_SET) == 54
    for name in E.CASES:                                               # deterministic: same name -> same arrays
        assert scene_digest(E.shade_edge_scene(name)) == scene_digest(E.shade_edge_scene(name))
    f, pi = np.float32, np.float32(np.pi)
    assert f(E.NEXT_ABOVE_1E15) > f(1e15) and np.nextafter(f(E.NEXT_ABOVE_1E15), f(0)) == f(1e15)
    # the albedo pair straddles the gate in the record the kernels read, albedo / PI_F, and is one float apart
    assert f(f(E.GATE_ALBEDO_AT) / pi) <= f(1e15) < f(f(E.GATE_ALBEDO_ABOVE) / pi)
    assert np.nextafter(f(E.GATE_ALBEDO_AT), f(np.inf)) == f(E.GATE_ALBEDO_ABOVE)


@pytest.fixture(scope="module")
def fixture():
    g = H.load_golden("refbuild_shade_edges.npz")
    w, h, depth, seed, n, stored = (int(v) for v in g["meta"])
    assert (w, h, depth, seed, n) == (E.W, E.H, E.DEPTH, E.SEED, E.NSAMPLES) and 0 < stored <= n
    assert [str(c) for c in g["cases"]] == E.REFERENCE_SET, "the fixture's cases are not the reference set"
    assert os.path.getsize(os.path.join(H.GOLDEN, "refbuild_shade_edges.npz")) < 300 * 1000
    return g, stored


@pytest.mark.parametrize("name", E.REFERENCE_SET)
def test_oracle_equals_the_reference_fixture(fixture, name):
    g, stored = fixture
    scene = E.shade_edge_scene(name)
    assert scene_digest(scene) == str(g[f"scene_sha256_{name}"]), "the case drifted from the fixture"
    r_rgb, r_draws = g[f"rgb_{name}"], g[f"draws_{name}"].astype(np.uint32)
    assert r_rgb.shape == (stored, 3) and r_draws.shape == (stored,)
    xs, ys, ss = E.sample_list()
    if H.ref_pt_lib() is not None:
        l_rgb, l_draws = H.RefPT(scene, E.W, E.H, E.DEPTH, True).trace_samples(E.SEED, xs, ys, ss)
        assert bits_equal(l_rgb[:stored], r_rgb).all() and np.array_equal(l_draws[:stored], r_draws)
    rgb, draws, _ = oracle_samples(name)
    assert bits_equal(rgb[:stored], r_rgb).all() and np.array_equal(draws[:stored], r_draws)
    libm = H.OraclePT(scene, E.W, E.H, E.DEPTH, True, math_mode=0).trace_samples(E.SEED, xs[:stored], ys[:stored], ss[:stored])
    assert bits_equal(libm[0], r_rgb).all() and np.array_equal(libm[1], r_draws)


class EmuPath(H.EmuPT):
    """path_sample() of csrc/pt_trace.h compiled for the host (tests/host_emu/path_host.cpp), one lane at a time: the feeder takes
    what EmuPT drops - delta lights, the environment light or map, a sphere light's mesh."""

    def __init__(self, scene, use_bvh=True):
        self.lib = ctypes.CDLL(H.build_host_lib("path_host", ["path_host.cpp"], scene_layer=True))
        self.lib.emu_create.restype = ctypes.c_void_p
        self.h_ = ctypes.c_void_p(self.lib.emu_create())
        self.use_bvh = use_bvh
        self.scene = scene
        self.feed(scene)

    def _add_sphere_light(self, radius, T, material, pos, nrm, idx):
        assert self.lib.emu_feed_sphere_light(self.h_, ctypes.c_float(radius), H.P(T), material, H.P(pos), H.P(nrm), len(pos), H.P(idx), len(idx)) == 0

    def _add_light(self, type_, radiance, angle_bounds, T):
        assert self.lib.emu_feed_light(self.h_, type_, H.P(radiance), H.P(angle_bounds), H.P(T)) == 0

    def _set_env(self, type_, radiance):
        assert self.lib.emu_feed_env_light(self.h_, type_, H.P(radiance)) == 0

    def _set_env_map(self, image):
        assert self.lib.emu_feed_env_map(self.h_, image.shape[1], image.shape[0], H.P(image)) == 0

    def samples(self, w, h, depth, seed, xs, ys, ss):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        cam = self.scene["camera"]
        iview = np.ascontiguousarray(cam["iview"], np.float32)
        rgb, draws, rays = np.zeros((len(xs), 3), np.float32), np.zeros(len(xs), np.uint32), np.zeros(len(xs), np.uint32)
        assert self.lib.emu_path_samples(self.h_, H.P(iview), ctypes.c_float(cam["vfov"]), ctypes.c_float(cam["ar"]), w, h, depth, ctypes.c_uint64(seed),
                                         H.P(xs), H.P(ys), H.P(ss), ctypes.c_size_t(len(xs)), H.P(rgb), H.P(draws), H.P(rays)) == 0
        return rgb, draws, rays


@pytest.mark.parametrize("name", E.CASES + list(NAMED))
def test_device_function_on_the_host_equals_the_oracle(name):
    """The kernels' per-sample function, built from the device headers with g++ (no fused operations, as the HIP build), against
    the oracle on the cases' sample list: radiance bits, draws and rays of every sample."""
    emu = EmuPath(scene_of(name))
    rgb, draws, rays = emu.samples(E.W, E.H, E.DEPTH, E.SEED, *E.sample_list())
    emu.close()
    o_rgb, o_draws, o_rays = oracle_samples(name)
    same = bits_equal(rgb, o_rgb).all(axis=1) & (draws == o_draws) & (rays == o_rays)
    assert same.all(), f"{name}: {int((~same).sum())} of {len(same)} samples differ; the first is sample {int(np.argmin(same))}"


def _differing(a, b):
    return ~bits_equal(a[0], b[0]).all(axis=1) | (a[1] != b[1]) | (a[2] != b[2])


@pytest.mark.parametrize("name", E.CASES)
def test_reach_guard(name):
    """A condition on the oracle alone: the case changes at least 5 % of the 600 samples of the scene it was cut from (radiance
    bits, draws or rays).  A case that does not is not reaching its edge: change the case, never the threshold."""
    share = float(_differing(oracle_samples(name), oracle_samples(name, base=True)).mean())
    print(f"reach {name}: {100.0 * share:.1f} %")
    assert share >= 0.05, f"{name} differs from {E.BASE[name]} in {100.0 * share:.1f} % of the samples"


@pytest.mark.parametrize("at,above", E.GATE_NEIGHBOURS)
def test_gate_neighbours_take_the_same_paths(at, above):
    """The two sides of the elision gate's bound are one float apart, so the renders the GPU tests compare across the gate differ
    in nothing but that float: every sample draws the same numbers and sends the same rays, the same channels are finite, and a
    finite channel moves by rounding alone.  (Bit-equal radiance cannot be asked for: the channel is a factor of every term it
    touches, and two neighbouring floats, at most 1 + 2^-23 apart, round those terms to different floats in a quarter of the
    samples.  Each of the up to 8 bounces of a path multiplies by the channel at most twice - evaluate and the scatter's
    attenuation - and rounds a handful of times: 8 * (2 * 2^-23 + 6 * 2^-24) < 5e-6 bounds the relative change of a term, and
    the terms of these scenes share their sign, so of a sum.)"""
    a, b = oracle_samples(at), oracle_samples(above)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(np.isfinite(a[0]), np.isfinite(b[0])) and np.array_equal(np.isnan(a[0]), np.isnan(b[0]))
    m = np.isfinite(a[0])
    rel = np.abs(a[0][m].astype(np.float64) - b[0][m]) / np.maximum(np.abs(a[0][m].astype(np.float64)), np.finfo(np.float32).tiny)
    print(f"gate {at}: {int(_differing(a, b).sum())} samples differ in radiance bits, largest relative change {rel.max():.3g}")
    assert rel.max() < 5e-6


class _FlatFile(H._SceneFeeder):
    """The feeder's calls as path_host.cpp's main() reads them: 32-bit words, {op, arguments} per call."""

    def __init__(self):
        self.parts = []

    def _put(self, *items):
        for x in items:
            if isinstance(x, np.ndarray):
                assert x.dtype.itemsize == 4
                self.parts.append(np.ascontiguousarray(x).tobytes())
            elif isinstance(x, float):
                self.parts.append(np.float32(x).tobytes())
            else:
                self.parts.append(np.uint32(x).tobytes())

    def _add_material(self, t, a, b, ior):
        self._put(1, t, a, b, ior)

    def _add_mesh(self, pos, nrm, idx, T, material, is_light):
        self._put(2, 0.0, material, int(is_light), T, len(pos), len(idx), pos, nrm, idx)

    def _add_sphere(self, radius, T, material):
        self._put(3, radius, material, T)

    def _add_sphere_light(self, radius, T, material, pos, nrm, idx):
        self._put(4, radius, material, 1, T, len(pos), len(idx), pos, nrm, idx)

    def _add_light(self, type_, radiance, angle_bounds, T):
        self._put(5, type_, radiance, angle_bounds, T)

    def _set_env(self, type_, radiance):
        self._put(6, type_, radiance)

    def _set_env_map(self, image):
        self._put(7, image.shape[1], image.shape[0], image)

    def _commit(self):
        self._put(8, 1)

    def _set_camera(self, iview, vfov, ar):
        self._put(9, iview, vfov, ar)

    def case(self, name, scene, expected):
        raw = name.encode()
        self._put(len(raw))
        self.parts.append(raw + b"\0" * (-len(raw) % 4))
        self.feed(scene)
        rgb, draws, rays = expected
        self._put(0, np.ascontiguousarray(rgb, np.float32), draws.astype(np.uint32), rays.astype(np.uint32))


def test_sanitized_program_evaluates_every_case(tmp_path):
    """path_host.cpp with its main(), built with -fsanitize=address,undefined and run as its own process over every case and named
    scene: the shading code reads nothing outside its tables (a one-texel environment map, a light list of any length) and does
    nothing undefined (float -> int conversions of out-of-range texel coordinates, shifts) at any of these parameters, and gives
    the oracle's values there as well."""
    prog = H.build_host_lib("path_sanitized", ["path_host.cpp"], scene_layer=True, program=True,
                            extra=("-g", "-DPATH_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    names = E.CASES + list(NAMED)
    xs, ys, ss = E.sample_list()
    ff = _FlatFile()
    ff._put(0x54534850, len(names), E.W, E.H, E.DEPTH, len(xs), E.SEED & 0xFFFFFFFF, E.SEED >> 32, xs, ys, ss)
    for name in names:
        ff.case(name, scene_of(name), oracle_samples(name))
    path = tmp_path / "shade_edges.bin"
    path.write_bytes(b"".join(ff.parts))
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"path_sanitized: ok ({len(names)} scenes" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
