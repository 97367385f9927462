"""GPU: every kernel form on the scenes of tests/_shade_edge_cases.py - one shading parameter at the edge of its range per scene:
glass iors at, below and far from 1, spot cones that are empty, inverted or wider than a circle, 1 to 7 delta lights (the wave
kernel sends their shadow rays in batches of three), black / negative / huge albedos and emissions, environment maps of one texel
row or column, materials on both sides of the elision gate's bound.  The expectation is the oracle's, bit for bit;
tests/test_pt_shade_edges_host.py holds the oracle to the reference build on the same scenes."""
import numpy as np
import pytest

import _harness as H
import _shade_edge_cases as E

pytestmark = pytest.mark.gpu

SPPS = (4, 1)            # units of 3 + 1 (pairs in the two-ray build), and bursts of one sample
EPOCH_SEED, EPOCH_BASE = 5, 9


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def has_lights(scene):
    return bool(scene.get("lights")) or bool(scene.get("env"))


_want = {}


def oracle_epoch(name, spp):
    if (name, spp) not in _want:
        _want[name, spp] = H.OraclePT(E.shade_edge_scene(name), E.W, E.H, E.DEPTH, True).epoch(EPOCH_SEED, EPOCH_BASE, spp)
    return _want[name, spp]


def context(srt):
    pt = srt.Pathtracer(0)
    pt.set_params(E.W, E.H, 1, E.DEPTH, True)
    return pt


def commit(pt, scene):
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_instrumented_kernel_equals_the_oracle(srt, family):
    """srt_pt_trace_samples (path_sample, one lane per sample) on the cases' sample list: per-sample radiance bits, draws and rays."""
    xs, ys, ss = E.sample_list()
    pt = context(srt)
    for name in E.FAMILIES[family]:
        scene = E.shade_edge_scene(name)
        commit(pt, scene)
        o_rgb, o_draws, o_rays = H.OraclePT(scene, E.W, E.H, E.DEPTH, True).trace_samples(E.SEED, xs, ys, ss)
        rgb, draws, rays = pt.trace_samples(E.SEED, xs, ys, ss)
        assert bits_equal(rgb, o_rgb), f"{name}: per-sample radiance differs from the oracle"
        assert np.array_equal(draws, o_draws) and np.array_equal(rays, o_rays), name
    pt.close()


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_every_form_equals_the_oracle(srt, family):
    """render_epoch in every kernel form, with srt_pt_set_elision off and on, at 4 and at 1 sample per pixel: the oracle's image bit
    for bit and one ray count per case.  A form may refuse a scene it is not built for, by the error the random-scene test
    tolerates; the auto form, lane per pixel and lane per sample take every scene."""
    pt = context(srt)
    for name in E.FAMILIES[family]:
        scene = E.shade_edge_scene(name)
        commit(pt, scene)
        lights = has_lights(scene)
        modes = (0, 1, 2, 4, 6) + (() if lights else (5,)) + ((7,) if family == "glass_mesh" else ())
        for spp in SPPS:
            want = oracle_epoch(name, spp)
            rays = set()
            for mode in modes:
                for elide in (False, True):
                    pt.set_kernel(mode)
                    pt.set_elision(elide)
                    pt.ray_count(reset=True); pt.rays_elided(reset=True)
                    try:
                        img = pt.render_epoch(EPOCH_SEED, EPOCH_BASE, spp)
                    except srt.SrtError as e:
                        # (the streamed form is built without point_lighting and says so for a scene with delta or environment lights)
                        assert "objects" in str(e) and mode not in (0, 1, 4) and lights, (name, mode, str(e))
                        continue
                    assert bits_equal(img, want), f"{name}: kernel mode {mode} (form {pt.kernel_form()}), elision {elide}, {spp} spp differs from the oracle"
                    rays.add(pt.ray_count()[0])
                    if lights or not elide:
                        assert pt.rays_elided() == 0, (name, mode, elide)
                    elif mode == 2:                          # the gate's verdict per case, as _shade_edge_cases.ELIDING derives it
                        assert (pt.rays_elided() > 0) == (name in E.ELIDING), (name, pt.rays_elided())
                    if family == "glass_mesh" and mode in (6, 7):
                        assert pt.kernel_form() == {6: 3, 7: 4}[mode], (name, mode, pt.kernel_form())
            assert len(rays) == 1 and next(iter(rays)) > 0, (name, spp, rays)
    pt.close()


def test_the_elision_gate_at_its_bounds(srt):
    """elision_provable (csrc/pt.hip) with srt_pt_set_elision on and the persistent sweeps: the two-ray build runs with a Lambertian or
    emission channel AT 1e15 and not with the next float above it, nor with a light whose emission has no positive luma; the image is
    the oracle's either way."""
    pt = context(srt)
    pt.set_kernel(2)
    pt.set_elision(True)
    for name in E.FAMILIES["gate"] + list(E.ORACLE_ONLY):
        commit(pt, E.shade_edge_scene(name))
        for spp in SPPS:
            pt.rays_elided(reset=True)
            assert bits_equal(pt.render_epoch(EPOCH_SEED, EPOCH_BASE, spp), oracle_epoch(name, spp)), (name, spp)
            elided = pt.rays_elided()
            assert (elided > 0) if name.endswith("_1e15") else elided == 0, (name, spp, elided)
    pt.close()


@pytest.mark.parametrize("at,above,material", [("gate_albedo_1e15", "gate_albedo_above", E.GATE_WALL),
                                               ("gate_emission_1e15", "gate_emission_above", E.LIGHT_MATERIAL)])
def test_the_gate_follows_update_materials(srt, at, above, material):
    """The gate is decided per render: srt_pt_update_materials moves the channel across the bound, in both directions, without a
    commit; the count of elided rays follows at the next render and the image is a fresh commit's."""
    scenes = {name: E.shade_edge_scene(name) for name in (at, above)}
    fresh = {}
    for name in (at, above):
        pt = context(srt)
        pt.set_kernel(2)
        pt.set_elision(True)
        commit(pt, scenes[name])
        fresh[name] = pt.render_epoch(EPOCH_SEED, EPOCH_BASE, 4)
        assert bits_equal(fresh[name], oracle_epoch(name, 4))
        pt.close()
    assert not bits_equal(fresh[at], fresh[above])           # (one float apart, but not the same image)
    for start, other in ((at, above), (above, at)):
        pt = context(srt)
        pt.set_kernel(2)
        pt.set_elision(True)
        commit(pt, scenes[start])
        pt.rays_elided(reset=True)
        assert bits_equal(pt.render_epoch(EPOCH_SEED, EPOCH_BASE, 4), fresh[start])
        assert (pt.rays_elided() > 0) == (start == at)
        for name in (other, start, other):
            pt.update_materials([material], [scenes[name]["materials"][material]])
            pt.rays_elided(reset=True)
            assert bits_equal(pt.render_epoch(EPOCH_SEED, EPOCH_BASE, 4), fresh[name]), (start, name)
            elided = pt.rays_elided()
            assert (elided > 0) if name == at else elided == 0, (start, name, elided)
        pt.close()
