"""GPU: Sphere::hit where no render reaches (tests/_sphere_cases.py: exact and near tangents, the validity chain of the two-root
branch, special operands).  The wave kernel's batch form - sphere_hitN<3>, whose tangent root sits behind a ballot, and the distance
step of object_testN's sphere branch through sqrtN - returns what the plain per-ray form returns (srt_pt_math_sphere_batch); the plain
form, through srt_pt_hit's nested walk and the flattened one, returns the reference build's records
(tests/golden/refbuild_sphere_edges.npz) and the oracle's, which tests/test_pt_sphere_host.py holds to the reference build on the
same sets; and Particle::update, the other caller that sends such rays, equals the oracle's.  Bit for bit, NaN equal to NaN."""
import os

import numpy as np
import pytest

import _harness as H
import _sphere_cases as S
from _cases import scene_digest
from test_pt_sphere_host import SEED, assert_records_equal, constructed, randoms, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import srt_amd

    p = srt_amd.Pathtracer(0)
    p.set_params(8, 8, 1, 4, True)
    yield p
    p.close()


def assert_batch_is_plain(batch, plain, family):
    for key in ("hit", "t", "dist"):
        ok = (batch[key] == plain[key]) if key == "hit" else same(batch[key], plain[key])
        bad = np.argwhere(~ok)
        assert bad.size == 0, (key, len(bad), sorted({S.FAMILIES[f] for f in family[bad[:, 0]]}), bad[:5], batch[key][~ok][:5], plain[key][~ok][:5])


def test_batch_equals_plain_random(pt):
    radius, org, dirs, bounds = S.random_sets(53, 1 << 18)
    batch, plain, delta, tangent = pt.math_sphere_batch(radius, org, dirs, bounds)
    print("random sets: hits", int(plain["hit"].sum()), "of", plain["hit"].size, "- waves through the tangent branch:", int(tangent[::64].sum()))
    assert_batch_is_plain(batch, plain, np.zeros(len(radius), np.int64))
    assert 0.1 < plain["hit"].mean() < 0.9


def test_batch_equals_plain_constructed(pt):
    radius, org, dirs, bounds, family, _ = S.constructed_sets(SEED)
    batch, plain, delta, tangent = pt.math_sphere_batch(radius, org, dirs, bounds)
    with np.errstate(invalid="ignore"):
        zero = delta == 0
    waves = tangent[::64]
    print("constructed sets:", len(radius), "hits", int(plain["hit"].sum()), "of", plain["hit"].size, "- rays with delta == 0:", int(zero.sum()),
          "- waves through the tangent branch:", int(waves.sum()), "of", len(waves))
    assert_batch_is_plain(batch, plain, family)
    assert waves.sum() > 100, "too few waves took the tangent branch"
    assert (~waves).sum() > 32, "too few waves went without the tangent root"
    assert plain["hit"][zero].all() and batch["hit"][zero].all(), "a ray with delta == 0 is a hit, whatever its bounds"
    lanes = zero.any(axis=1)
    expect = np.array([lanes[w: w + 64].any() for w in range(0, len(lanes), 64)])
    assert np.array_equal(expect, waves), "the tangent branch is taken exactly by the waves that hold a lane with delta == 0"


def device_hits(pt, mode, rays, kind):
    pt.set_kernel(mode)

    def make(scene):
        pt.build_scene(scene)
        return pt

    try:
        return S.scene_hits(make, *rays, kind)
    finally:
        pt.set_kernel(0)


@pytest.mark.parametrize("mode", [0, 5])
def test_plain_equals_reference_fixture(pt, mode):
    """srt_pt_hit - sphere_hit in the walk, again in surface_of - on the fixture's two scenes: the reference build's records."""
    g = np.load(os.path.join(H.GOLDEN, "refbuild_sphere_edges.npz"))
    rays = S.rays_of(g["radius"], g["org"], g["dirs"], g["bounds"])
    family = np.repeat(g["family"], 3)
    for kind in S.SCENE_KINDS:
        assert str(g[f"scene_sha256_{kind}"]) == S.scenes_digest(rays[0], kind, scene_digest)
        assert_records_equal(device_hits(pt, mode, rays, kind), g[f"ref_{kind}"], family, f"kernel mode {mode} against the reference fixture, {kind} scene")


@pytest.mark.parametrize("mode", [0, 5])
def test_plain_equals_oracle_all_sets(pt, mode):
    for name, (sets, rays, rec) in (("constructed", constructed()), ("random", randoms())):
        family = np.repeat(sets[4], 3) if name == "constructed" else np.zeros(len(rays[0]), np.int64)
        for kind in S.SCENE_KINDS:
            assert_records_equal(device_hits(pt, mode, rays, kind), rec[kind], family, f"kernel mode {mode} against the oracle, {name} sets, {kind} scene")


def test_particles_on_tangent_paths(pt):
    """Scene_Particles::Particle::update sends Ray(position, velocity): the origins and un-normalised directions of family A, one step
    against the oracle's.  A tangent hit has cos_t == 0 exactly and flies on; a grazing one (delta a few ulps above zero) bounces."""
    (radius, org, dirs, bounds, family, _), rays, _ = constructed()
    a = np.flatnonzero(np.repeat(family, 3) == S.FAM["tangent_exact"])[:10000]
    rad, pos, vel = rays[0][a], rays[1][a], rays[2][a]
    age = np.random.default_rng(7).uniform(-0.005, 0.5, len(a)).astype(np.float32)
    dt, size = 0.01, 0.015
    bounced = alive = 0
    for r, idx in S.by_radius(rad):
        scene = S.sphere_scene(r, "identity")
        want = H.OraclePT(scene, 8, 8, 4, True).particles_update(pos[idx], vel[idx], age[idx], dt, size)
        pt.build_scene(scene)
        got = pt.particles_step(pos[idx], vel[idx], age[idx], dt, size)
        for k, what in enumerate(("position", "velocity", "age")):
            bad = np.flatnonzero(~same(got[k].reshape(len(idx), -1), want[k].reshape(len(idx), -1)).all(axis=1))
            assert bad.size == 0, (what, float(r), len(bad), bad[:5], got[k][bad[:3]], want[k][bad[:3]])
        assert np.array_equal(got[3], want[3])
        free = vel[idx] + np.array([0.0, -9.8 * dt, 0.0], np.float32)
        bounced += int((np.abs(want[1] - free) > 1e-3).any(axis=1).sum())
        alive += int(want[3].sum())
    print("particles:", len(a), "bounced", bounced, "alive", alive)
    assert bounced > len(a) // 20 and 0 < alive < len(a)
