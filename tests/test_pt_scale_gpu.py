"""GPU: the path tracer in worlds off unit scale (tests/_scale_cases.py) - scaled in the geometry or in the pose until the divides
of Triangle::hit and Ray::transform leave their exact fast path's window in some lanes of a wave, in all, or in none; translated;
projective.  Every kernel form against the oracle bit for bit (NaN matching NaN), which tests/test_pt_scale_host.py and the
fixtures of tests/golden/make_pt_golden.py hold to the reference build at the same scales.  Small images: a test takes seconds."""
import functools
import glob
import os

import numpy as np
import pytest

import _harness as H
import _scale_cases as SC
from _cases import pt_sample_list, pt_scene, scene_digest

pytestmark = pytest.mark.gpu

W, HGT, SPP = 32, 24, 4
MODES = (1, 2, 4, 5, 6, 7)
IDS = [SC.case_id(c) for c in SC.CASES]


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def make_pt(srt, scene, w, h, use_bvh, spp=1):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, spp, SC.DEPTH, use_bvh)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


@functools.lru_cache(maxsize=None)
def _fixtures():
    """{(scene name, use_bvh): path} of the reference-built fixtures made at the depth the cases use."""
    out = {}
    for path in sorted(glob.glob(os.path.join(H.GOLDEN, "pt_*.npz"))):
        g = np.load(path)
        if int(g["meta"][2]) == SC.DEPTH:
            out[(str(g["scene"]), bool(g["meta"][3]))] = path
    return out


def golden_of(name, use_bvh):
    """The reference-built fixture of the case, or None."""
    path = _fixtures().get((name, use_bvh))
    return np.load(path) if path else None


def every_form(srt, pt, want, seed, base, spp, what):
    """Every kernel mode that takes the scene, dead-ray elision off and on: the image is `want`, the ray counts agree."""
    rays, took = set(), []
    for mode in MODES:
        for elide in (False, True):
            pt.set_kernel(mode)
            pt.set_elision(elide)
            pt.ray_count(reset=True)
            try:
                img = pt.render_epoch(seed, base, spp)
            except srt.SrtError as e:       # a kernel that does not take the scene says so: too many objects, or a build without
                assert "objects" in str(e)  # point_lighting for a scene with lights; any other error fails the test
                continue
            assert bits_equal(img, want), f"{what}: kernel mode {mode}, elision {elide} differs"
            rays.add(pt.ray_count()[0])
            took.append(mode)
    pt.set_elision(False)
    pt.set_kernel(0)
    assert len(rays) == 1 and {1, 2, 4} <= set(took), (rays, took)    # (the lane-per-pixel, wave and lane-per-sample forms take every case)
    return took


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_epochs_every_kernel_form(srt, case):
    """4.1: render_epoch of every kernel mode, with and without elision, equals the oracle's epoch and - where the case has a
    fixture - the reference build's."""
    name, _, use_bvh = case
    scene = pt_scene(name)
    want = H.OraclePT(scene, W, HGT, SC.DEPTH, use_bvh).epoch(7, 5, SPP)
    pt = make_pt(srt, scene, W, HGT, use_bvh, SPP)
    took = every_form(srt, pt, want, 7, 5, SPP, "oracle")
    if "lights" not in scene and "env" not in scene:
        assert 5 in took                                 # (the flattened walk has no point_lighting: it refuses those scenes)
    g = golden_of(name, use_bvh)
    if g is not None and "epoch" in g:
        assert scene_digest(scene) == str(g["scene_sha256"])
        ew, eh, spp, base = (int(x) for x in g["epoch_meta"])
        pt.set_params(ew, eh, spp, SC.DEPTH, use_bvh)
        every_form(srt, pt, g["epoch"], int(g["seed"]), base, spp, "reference fixture")
    pt.close()


def test_the_fixtures_are_there():
    """Six of the cases have a reference-built fixture: the comparison above is not vacuous."""
    have = [name for name, _, use_bvh in SC.CASES if golden_of(name, use_bvh) is not None]
    assert len(have) >= 6, have


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_samples_counters_and_hits(srt, case):
    """4.2: trace_samples equals the oracle in radiance, RNG draws and rays per sample, and the instrumented kernel walks the same
    nodes, objects and triangles (srt_pt_counters).  4.3: scene.hit through the nested walk and through the flattened one
    (mode 5), rays and velocities carried into the world."""
    name, group, use_bvh = case
    scene = pt_scene(name)
    pt = make_pt(srt, scene, W, HGT, use_bvh)
    o = H.OraclePT(scene, W, HGT, SC.DEPTH, use_bvh)
    xs, ys, ss = pt_sample_list(31, W, HGT, 3000, max_sample=1 << 20)
    cnt = np.zeros(8, np.uint64)
    o_rgb, o_draws, o_rays = o.trace_samples(99, xs, ys, ss, cnt)
    rgb, draws, rays = pt.trace_samples(99, xs, ys, ss)
    assert bits_equal(rgb, o_rgb), "per-sample radiance differs from the oracle"
    assert np.array_equal(draws, o_draws) and np.array_equal(rays, o_rays)
    assert pt.counters() == dict(zip(H.COUNTER_NAMES, (int(v) for v in cnt)))
    for kind, seed in (("random_rays", 41), ("unnormalised_rays", 42)):
        org, d, b = SC.scaled_rays(kind, seed, 2048, scene)
        want = o.hit(org, d, b)
        if group not in ("degenerate", "projective", "moved-sparse"):
            assert int(want[:, 0].sum()) > 500, "the rays were not carried into the world"
        for mode in (0, 5):
            pt.set_kernel(mode)
            assert bits_equal(pt.hit(org, d, b), want), f"scene.hit of {kind} (kernel mode {mode}) differs from the oracle"
    pt.close()


@pytest.mark.parametrize("name", [f"{SC.BLOB}@geom:{SC.MIXED_GEOM[SC.BLOB][0]}", f"{SC.BLOB}@geom:{SC.MIXED_GEOM[SC.BLOB][1]}",
                                  f"{SC.BLOB}@geom:{SC.OUTSIDE_GEOM[1]}", f"{SC.BLOB_RANDOM}@move:b"])
def test_device_bvh_build_equals_host_build(srt, name):
    """4.4: BVH::build on the device (every tree, the BVH<Object> too) gives the host build's node boxes, links and primitive order
    where the SAH arithmetic sees scaled and shifted numbers, and both are the oracle's."""
    assert name in [c[0] for c in SC.CASES]
    scene = pt_scene(name)
    nobj = len(scene["objects"])
    o = H.OraclePT(scene, 8, 8, SC.DEPTH, True)
    pts = []
    for device in (False, True):
        pt = srt.Pathtracer(0)
        pt.set_params(8, 8, 1, SC.DEPTH, True)
        pt.set_bvh_builder(device, 1)
        pt.build_scene(scene)
        pts.append(pt)
    real = 0
    for k in range(-1, nobj):
        want = o.dump_bvh(k, cap=1 << 12)
        if want is None:
            continue
        n = nobj if k < 0 else int(want[1][0][1])
        for pt in pts:
            boxes, links, order = pt.dump_bvh(k, cap=1 << 12)
            assert bits_equal(boxes, want[0]) and np.array_equal(links, want[1]) and np.array_equal(order[:n], want[2][:n]), f"tree {k}"
        real += int(k >= 0 and len(want[0]) > 1)
    assert real >= 1, "no real BVH<Triangle> was compared"
    org, d, b = SC.scaled_rays("random_rays", 43, 1024, scene)
    assert bits_equal(pts[1].hit(org, d, b), o.hit(org, d, b))
    for pt in pts:
        pt.close()


@pytest.mark.parametrize("name", ["cbox@geom:-13", "cbox@geom:14"])
def test_particles_step_in_a_scaled_box(srt, name):
    """4.5: Scene_Particles::Particle::update on the device in a geometry-scaled box - the cloud, its speeds and the radius scaled
    alike - against the oracle's, three steps."""
    scene = pt_scene(name)
    s = scene["world_scale"]
    pt = make_pt(srt, scene, 8, 8, True)
    o = H.OraclePT(scene, 8, 8, SC.DEPTH, True)
    pos, vel, age = SC.scaled_particles(17, 4000, scene)
    radius = float(np.float32(0.015 * s))
    moving = (vel != 0).any(axis=1)
    ahead = o.hit(pos, vel, np.tile(np.array([0.0, np.inf], np.float32), (len(pos), 1)))[:, 0]
    assert ahead[moving].mean() > 0.5, "the cloud was not carried into the box"
    for step in range(3):
        want = o.particles_update(pos, vel, age, 0.01, radius)
        got = pt.particles_step(pos, vel, age, 0.01, radius)
        assert all(bits_equal(x, y) for x, y in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3]), f"step {step}"
        pos, vel, age = got[:3]
    assert 0 < int(got[3].sum()) < len(age)                       # some died, some live
    pt.close()


@pytest.mark.parametrize("name", [f"{SC.BLOB}@geom:{SC.MIXED_GEOM[SC.BLOB][1]}", f"{SC.BLOB}@pose:38"])
def test_streamed_forms_with_a_small_population(srt, name):
    """4.6: modes 6 and 7 with 256 path slots, far fewer than the units of the epoch, so that refills cross waves whose lanes
    disagree about the window.  (The streamed forms want a mesh with a real BVH<Triangle>: the blob scene, one mixed case of each
    window.)"""
    assert (name, "mixed", True) in SC.CASES
    scene = pt_scene(name)
    w, h, spp = 32, 24, 4
    want = H.OraclePT(scene, w, h, SC.DEPTH, True).epoch(9, 2, spp)
    pt = make_pt(srt, scene, w, h, True, spp)
    pt.set_stream_slots(256)
    for mode in (6, 7):
        for elide in (False, True):
            pt.set_kernel(mode)
            pt.set_elision(elide)
            assert pt.kernel_form() in (3, 4)
            assert bits_equal(pt.render_epoch(9, 2, spp), want), (mode, elide)
    pt.close()
