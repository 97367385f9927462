"""GPU: every kernel form on shared triangle / BVH<Triangle> ranges (srt_pt_add_instance) and on a re-posed scene
(srt_pt_repose).  S has instances; the oracle, which knows nothing of instances, is given S' = expand(S): the same call sequence
with srt_pt_add_mesh of the source's arrays in place of every instance.  Everything computed must be bit-equal; only storage
differs (srt_pt_scene_counts)."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
from _cases import particle_cloud, random_rays, unnormalised_rays

pytestmark = pytest.mark.gpu

NOBJ = 74
W, HT, DEPTH, SPP, SEED = 32, 24, 4, 2, 9


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def make_pt(srt, scene, w, h, depth, use_bvh=True):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, use_bvh)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def every_sample(w, h, spp):
    ys, xs, ss = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
    return xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32), ss.reshape(-1).astype(np.uint32)


@pytest.fixture(scope="module")
def particles():
    """S, S', the oracle on S' and what it computes once for the tests below."""
    S, S1, _ = IC.particles_shared()
    o = H.OraclePT(S1, W, HT, DEPTH, True)
    xs, ys, ss = every_sample(W, HT, SPP)
    return {"S": S, "S1": S1, "oracle": o, "samples": (xs, ys, ss), "want_samples": o.trace_samples(SEED, xs, ys, ss),
            "want_epoch": o.epoch(SEED, 0, SPP)}


@pytest.fixture(scope="module")
def pt_particles(srt, particles):
    pt = make_pt(srt, particles["S"], W, HT, DEPTH)
    yield pt
    pt.close()


def test_particles_every_sample(pt_particles, particles):
    """Radiance, RNG draws and rays of every pixel and sample of S against the oracle on S'."""
    pt = pt_particles
    rgb, draws, rays = pt.trace_samples(SEED, *particles["samples"])
    want_rgb, want_draws, want_rays = particles["want_samples"]
    assert np.array_equal(draws, want_draws) and np.array_equal(rays, want_rays)
    assert bits_equal(rgb, want_rgb)
    counts = pt.scene_counts()
    assert counts["objects"] == NOBJ and counts["blas_builds"] == 3           # one wall, the light, the particle mesh
    assert counts["device_bytes"] > 0 and counts["uploaded_bytes"] == counts["device_bytes"]


@pytest.mark.parametrize("mode", [0, 1, 4, 6])
def test_particles_epoch_every_form(pt_particles, particles, mode):
    """srt_pt_trace_samples has one kernel whatever the mode; the epoch image is where the forms differ: lane per pixel (1), lane
    per sample (4), the streamed form (6, and what auto takes: 74 objects are more than the sweeps hold)."""
    pt = pt_particles
    pt.set_kernel(mode)
    if mode == 0:
        assert pt.kernel_form() == 3
    got = pt.render_epoch(SEED, 0, SPP)
    pt.set_kernel(0)
    assert bits_equal(got, particles["want_epoch"]), f"kernel mode {mode}"


@pytest.fixture(scope="module")
def sweeps():
    S = IC.sweeps_scene()
    S1 = IC.expand(S)
    w = h = 32
    o = H.OraclePT(S1, w, h, 5, True)
    xs, ys, ss = every_sample(w, h, 2)
    return {"S": S, "S1": S1, "oracle": o, "samples": (xs, ys, ss), "want_samples": o.trace_samples(SEED, xs, ys, ss),
            "want_epoch": o.epoch(SEED, 0, 2)}


@pytest.fixture(scope="module")
def pt_sweeps(srt, sweeps):
    pt = make_pt(srt, sweeps["S"], 32, 32, 5)
    yield pt
    pt.close()


def test_sweeps_scene_every_sample(pt_sweeps, sweeps):
    pt = pt_sweeps
    assert len(sweeps["S"]["objects"]) <= 16
    rgb, draws, rays = pt.trace_samples(SEED, *sweeps["samples"])
    want_rgb, want_draws, want_rays = sweeps["want_samples"]
    assert np.array_equal(draws, want_draws) and np.array_equal(rays, want_rays)
    assert bits_equal(rgb, want_rgb)
    counts = pt.scene_counts()
    assert counts["blas_records"] > 0 and counts["blas_builds"] == 7          # five walls, the light, the blob - not its instance
    # scene.hit through the nested walk and (mode 5) the flattened walk, with both objects of the shared range in the way
    org, d, b = random_rays(3, 2048)
    want = sweeps["oracle"].hit(org, d, b)
    assert bits_equal(pt.hit(org, d, b), want)
    pt.set_kernel(5)
    got = pt.hit(org, d, b)
    pt.set_kernel(0)
    assert bits_equal(got, want)


@pytest.mark.parametrize("mode", [0, 2, 5, 6, 7])
def test_sweeps_scene_epoch_every_form(pt_sweeps, sweeps, mode):
    """Two objects on ONE BVH<Triangle>, the second rotated and non-uniformly scaled, in glass: the wave-uniform sweeps with inline
    walks (2), the flattened walk (5), the streamed form (6) and the streamed sweeps (7, and auto), whose walk queues go by mesh
    ordinal - two ordinals on one record range here."""
    pt = pt_sweeps
    pt.set_kernel(mode)
    form = pt.kernel_form()
    got = pt.render_epoch(SEED, 0, 2)
    pt.set_kernel(0)
    assert form == {0: 4, 2: 1, 5: 2, 6: 3, 7: 4}[mode]
    assert bits_equal(got, sweeps["want_epoch"]), f"kernel mode {mode}"


def test_hit_records(pt_particles, particles):
    """srt_pt_hit: 4096 seeded rays, half of them with un-normalised directions and bounds [0, inf]."""
    o1, d1, b1 = random_rays(11, 2048)
    o2, d2, b2 = unnormalised_rays(12, 2048)
    org, d, b = np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([b1, b2])
    got = pt_particles.hit(org, d, b)
    want = particles["oracle"].hit(org, d, b)
    assert np.count_nonzero(want[:, 0]) > 1000 and np.count_nonzero(want[:, 8] == 8) > 0     # some of them on the particles (material 8)
    assert bits_equal(got, want)


def test_particle_step(pt_particles, particles):
    pos, vel, age = particle_cloud(31, 512)
    got = pt_particles.particles_step(pos, vel, age, 0.01, 0.015)
    want = particles["oracle"].particles_update(pos, vel, age, 0.01, 0.015)
    assert all(bits_equal(x, y) for x, y in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3])


def test_normal_colors(srt, pt_particles, particles):
    """The normal-colors view of S equals the product's own view of S'."""
    copies = make_pt(srt, particles["S1"], W, HT, DEPTH)
    images = []
    for pt in (pt_particles, copies):
        pt.set_normal_colors(True)
        images.append(pt.render_epoch(SEED, 0, SPP))
        pt.set_normal_colors(False)
    more = copies.scene_counts()["triangles"] - pt_particles.scene_counts()["triangles"]
    copies.close()
    assert more == 1920 - 32 + 8                                                 # the 59 particle instances and four walls
    assert np.count_nonzero(images[0]) > 0 and bits_equal(images[0], images[1])


def test_device_builder(srt, particles):
    """set_bvh_builder(True, 16): the shared BVH<Triangle> (32 triangles - the only mesh of the scene above the threshold, so the
    one device BLAS build) and the BVH<Object> (74 objects) come from the device builder; the dumps equal the host build's."""
    S = particles["S"]
    dumps, counts = [], []
    for device in (False, True):
        pt = srt.Pathtracer(0)
        pt.set_params(W, HT, 1, DEPTH, True)
        pt.set_bvh_builder(device, 16)
        pt.build_scene(S)
        dumps.append(IC.all_dumps(pt, NOBJ))
        counts.append(pt.scene_counts())
        if device:
            pt.set_camera(S["camera"])
            image = pt.render_epoch(SEED, 0, SPP)
        pt.close()
    assert IC.dumps_equal(dumps[0], dumps[1])
    assert counts[0] == counts[1] and counts[1]["blas_builds"] == 3 and counts[1]["triangles"] == 2 + 2 + 32 + 2      # a wall, the light, the particle mesh, the light-list copy
    assert bits_equal(image, particles["want_epoch"])


def test_repose_on_the_device(srt, pt_particles, particles):
    """Render, repose 10 instances, render: the image of a fresh context (and of the oracle) on the new poses; back: the first
    image.  No triangle, normal, packed-triangle or BVH<Triangle>-record byte is uploaded by either repose."""
    S, S1 = particles["S"], particles["S1"]
    pt = pt_particles
    idx, Ts = IC.repose_case(S)
    idx, Ts = idx[1:11], Ts[1:11]
    assert all(S["objects"][i]["kind"] == "instance" for i in idx)
    first = pt.render_epoch(SEED, 0, SPP)
    assert bits_equal(first, particles["want_epoch"])
    before = pt.scene_counts()
    pt.repose(idx, Ts)
    moved = pt.render_epoch(SEED, 0, SPP)
    fresh = make_pt(srt, IC.with_poses(S, idx, Ts), W, HT, DEPTH)
    want = fresh.render_epoch(SEED, 0, SPP)
    same_trees = IC.dumps_equal(IC.all_dumps(pt, NOBJ), IC.all_dumps(fresh, NOBJ))
    fresh.close()
    want_oracle = H.OraclePT(IC.with_poses(S1, idx, Ts), W, HT, DEPTH, True).epoch(SEED, 0, SPP)
    org, d, b = random_rays(5, 1024)
    hits = pt.hit(org, d, b)
    pt.repose(idx, np.array([S["objects"][i]["T"] for i in idx], np.float32))
    back = pt.render_epoch(SEED, 0, SPP)
    after = pt.scene_counts()
    assert same_trees and not bits_equal(moved, first)
    assert bits_equal(moved, want) and bits_equal(moved, want_oracle)
    assert bits_equal(hits, H.OraclePT(IC.with_poses(S1, idx, Ts), W, HT, DEPTH, True).hit(org, d, b))
    assert bits_equal(back, first)
    assert after["uploaded_triangle_bytes"] == before["uploaded_triangle_bytes"] > 0
    assert after["uploaded_bytes"] > before["uploaded_bytes"] and after["blas_builds"] == before["blas_builds"]
    assert after["device_bytes"] == before["device_bytes"]


def test_repose_sweeps_scene(srt, pt_sweeps, sweeps):
    """Re-posing under the streamed sweeps: the instance moves to the other side of its source, so that object order - and with
    it the meshes' ordinals and the lazy bits of the top-level records - changes."""
    S, S1 = sweeps["S"], sweeps["S1"]
    pt = pt_sweeps
    n = len(S["objects"])
    T = IC.translate(S["objects"][n - 1]["T"], (0.5, -0.25, 0.3))
    pt.repose([n - 1], [T])
    assert pt.kernel_form() == 4
    got = pt.render_epoch(SEED, 0, 2)
    pt.set_kernel(2)
    got2 = pt.render_epoch(SEED, 0, 2)
    pt.set_kernel(0)
    pt.repose([n - 1], [S["objects"][n - 1]["T"]])
    back = pt.render_epoch(SEED, 0, 2)
    want = H.OraclePT(IC.with_poses(S1, [n - 1], [T]), 32, 32, 5, True).epoch(SEED, 0, 2)
    assert bits_equal(got, want) and bits_equal(got2, want)
    assert bits_equal(back, sweeps["want_epoch"])


def test_group(srt, particles):
    """A two-rank PathtracerGroup on one device renders S like the single context; repose and scene_counts reach every member."""
    S = particles["S"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    image = grp.render_epoch(SEED, 0, SPP)
    counts = grp.scene_counts()
    idx, Ts = IC.repose_case(S)
    grp.repose(idx, Ts)
    moved = grp.render_epoch(SEED, 0, SPP)
    grp.close()
    assert bits_equal(image, particles["want_epoch"])
    assert len(counts) == 2 and counts[0] == counts[1] and counts[0]["objects"] == NOBJ and counts[0]["blas_builds"] == 3
    want = H.OraclePT(IC.with_poses(particles["S1"], idx, Ts), W, HT, DEPTH, True).epoch(SEED, 0, SPP)
    assert bits_equal(moved, want)
