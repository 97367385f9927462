"""CPU: Sphere::hit where no render reaches - exact and near tangents, the validity chain of the two-root branch, special operands
(tests/_sphere_cases.py).  The oracle's sphere_hit against what the reference build recorded for these rays
(tests/golden/refbuild_sphere_edges.npz) and, where oracle/_ref is present, against the reference build itself; the device headers'
sphere_hit and sphere_hitN compiled for the host (tests/host_emu/sphere_host.cpp) against the oracle; and the conditions on the
inputs that keep these tests - and tests/test_pt_sphere_gpu.py - from going hollow.  Everything bit for bit, NaN equal to NaN."""
import ctypes
import functools
import os

import numpy as np
import pytest

import _harness as H
import _sphere_cases as S
from _cases import scene_digest

SEED, RANDOM_SEED, RANDOM_SETS = S.FIXTURE_SEED, 52, 4096
FIELDS = (("hit", slice(0, 1)), ("distance", slice(1, 2)), ("position", slice(2, 5)), ("normal", slice(5, 8)))


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_records_equal(got, want, family, what):
    """(n, >= 8) scene.hit records {hit, distance, position, normal}: equal bit for bit, NaN == NaN; a failure names the families."""
    for name, cols in FIELDS:
        bad = np.flatnonzero(~same(got[:, cols], want[:, cols]).all(axis=1))
        assert bad.size == 0, (what, name, len(bad), sorted({S.FAMILIES[f] for f in family[bad]}), bad[:5], got[bad[:3]], want[bad[:3]])


def oracle_of(scene):
    return H.OraclePT(scene, 8, 8, 4, True)


@functools.lru_cache(maxsize=None)
def constructed():
    """The constructed sets, their rays, and the oracle's records of the rays on the one-sphere scenes of both kinds."""
    radius, org, dirs, bounds, family, step = S.constructed_sets(SEED)
    rays = S.rays_of(radius, org, dirs, bounds)
    rec = {kind: S.scene_hits(oracle_of, *rays, kind) for kind in S.SCENE_KINDS}
    return (radius, org, dirs, bounds, family, step), rays, rec


@functools.lru_cache(maxsize=None)
def randoms():
    sets = S.random_sets(RANDOM_SEED, RANDOM_SETS)
    rays = S.rays_of(*sets)
    return sets, rays, {kind: S.scene_hits(oracle_of, *rays, kind) for kind in S.SCENE_KINDS}


def share(mask, of=None):
    return float(mask.mean()) if of is None else float(mask[of].mean())


def test_the_inputs_reach_every_branch():
    """The conditions on the inputs, from the oracle's results: the tangent families hold every class of delta, a ray that
    delta_f32 calls a miss is one, one it calls tangent hits whatever its bounds say, and the validity chain's families hold each
    of its four outcomes.  (Over the chain's families together: no family of it can hold all four - a sphere behind the ray only
    misses.)"""
    (radius, org, dirs, bounds, family, step), rays, rec = constructed()
    hit = rec["identity"][:, 0] != 0
    fam3, step3 = np.repeat(family, 3), np.repeat(step, 3)
    delta = S.delta_f32(radius, org, dirs).reshape(-1)
    with np.errstate(invalid="ignore"):
        neg, zero, pos = delta < 0, delta == 0, delta > 0
    finite = np.isfinite(rays[0]) & np.isfinite(rays[1]).all(axis=1) & np.isfinite(rays[2]).all(axis=1)
    for name in ("tangent_exact", "tangent_near"):
        m = fam3 == S.FAM[name]
        shares = [share(c, m) for c in (neg, zero, pos)]
        print(f"{name}: {int(m.sum())} rays, delta < 0 / == 0 / > 0: " + " / ".join(f"{100 * s:.1f} %" for s in shares))
        assert min(shares) >= 0.03, (name, shares)
    a0 = (fam3 == S.FAM["tangent_exact"]) & (step3 == 0)
    assert a0.sum() >= 90 and zero[a0].all(), "a step-0 set of family A is not an exact tangent"
    assert not hit[neg].any(), "the oracle hits where delta_f32 < 0: delta_f32's operation order is not the oracle's"
    assert hit[zero & finite].all(), "the oracle misses a tangent ray: delta_f32's operation order is not the oracle's"
    with np.errstate(all="ignore"):                                        # t = k / s < 0: o.z = -k and d.z = s of one sign
        behind = zero & (fam3 == S.FAM["tangent_exact"]) & (rec["identity"][:, 1] > 0) & (np.repeat(org[:, 2], 3) * dirs.reshape(-1, 3)[:, 2] > 0)
    assert behind.sum() > 100, "no tangent ray whose tangent point lies behind it"
    nan_t = zero & hit & (rays[2] == 0).all(axis=1)
    assert nan_t.sum() > 100 and np.isnan(rec["identity"][nan_t, 1]).all(), "a zero direction: delta == 0, t = 0 / 0, a hit at distance NaN"
    # the validity chain: which roots are valid, by the restated chain - and the oracle's verdict agrees with the restatement
    v1, v2 = (v.reshape(-1) for v in S.root_validity(radius, org, dirs, bounds))
    chain = np.isin(fam3, [S.FAM[f] for f in S.CHAIN])
    assert pos[chain].all()
    outcomes = {"both": v1 & v2, "only near": v2 & ~v1, "only far": v1 & ~v2, "none": ~v1 & ~v2}
    print("validity chain:", int(chain.sum()), "rays -", ", ".join(f"{k} {100 * share(v, chain):.1f} %" for k, v in outcomes.items()))
    for k, v in outcomes.items():
        assert share(v, chain) >= 0.05, (k, share(v, chain))
        assert (hit[chain & v] == (k != "none")).all(), k
    t1, t2, _, _ = (a.reshape(-1) for a in S.roots_f32(radius, org, dirs))
    twins = pos & (t1 == t2)
    print("two roots that narrow to one float (t1 == t2):", int(twins.sum()), "rays, hits", int(hit[twins].sum()))
    assert twins.sum() > 100 and hit[twins].any() and not hit[twins].all()
    # the layout the GPU test counts on: waves (64 consecutive sets) with and without a tangent lane
    lanes = zero.reshape(-1, 3).any(axis=1)
    waves = lanes[: len(lanes) // 64 * 64].reshape(-1, 64).any(axis=1)
    tang = np.isin(family, [S.FAM["tangent_exact"], S.FAM["tangent_near"]])
    tw = waves[np.flatnonzero(tang[: len(waves) * 64: 64])]
    print(f"waves: {len(waves)}, with a tangent lane {int(waves.sum())}, without {int((~waves).sum())}; of the tangent families' {len(tw)}: {int(tw.sum())}")
    assert waves.sum() > 100 and (~waves).sum() > 32
    first = np.flatnonzero(tang)
    assert (np.diff(first) == 1).all(), "the tangent families are not contiguous"
    ordinary = np.flatnonzero(family == S.FAM["ordinary"])
    assert len(ordinary) >= 64 * 64 and (np.diff(ordinary) == 1).all()
    assert set(family.tolist()) == set(range(len(S.FAMILIES)))


def test_oracle_equals_the_reference_fixture():
    """What the reference build returned for the fixture's rays, on both scenes, is what the oracle returns today; the fixture's
    inputs are what the generator makes today, and its scenes are today's."""
    g = np.load(os.path.join(H.GOLDEN, "refbuild_sphere_edges.npz"))
    index, *sets = S.fixture_sets()
    radius, org, dirs, bounds, family, step = sets
    for key, a in zip(("index", "radius", "org", "dirs", "bounds", "family", "step"), [index] + sets):
        assert g[key].dtype == a.dtype and g[key].tobytes() == a.tobytes(), f"the fixture's {key} is not what tests/_sphere_cases.py generates"
    assert [str(f) for f in g["families"]] == list(S.FAMILIES) and set(family.tolist()) == set(range(len(S.FAMILIES)))
    rays = S.rays_of(radius, org, dirs, bounds)
    assert 3000 < len(rays[0]) <= 20000
    _, _, rec = constructed()
    ray_index = (3 * index[:, None] + np.arange(3)).reshape(-1)
    for kind in S.SCENE_KINDS:
        assert str(g[f"scene_sha256_{kind}"]) == S.scenes_digest(rays[0], kind, scene_digest)
        want = g[f"ref_{kind}"]
        assert 0.3 < (want[:, 0] != 0).mean() < 0.7
        assert_records_equal(rec[kind][ray_index], want, np.repeat(family, 3), f"oracle against the reference fixture, {kind} scene")


@pytest.mark.ref
@pytest.mark.skipif(H.ref_pt_lib() is None, reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("kind", S.SCENE_KINDS)
def test_oracle_equals_the_reference_build(kind):
    """Every constructed and random set through the reference build's own scene.hit."""
    ref_of = lambda scene: H.RefPT(scene, 8, 8, 4, True)
    sets, rays, rec = constructed()
    assert_records_equal(rec[kind], S.scene_hits(ref_of, *rays, kind), np.repeat(sets[4], 3), f"constructed sets, {kind} scene")
    sets, rays, rec = randoms()
    want = S.scene_hits(ref_of, *rays, kind)
    assert_records_equal(rec[kind], want, np.zeros(len(want), np.int64), f"random sets, {kind} scene")
    assert 0.1 < (want[:, 0] != 0).mean() < 0.9


_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("sphere_host", ["sphere_host.cpp"]))
    return _lib


def host_sphere(radius, org, dirs, bounds):
    """tests/host_emu/sphere_host.cpp on n sets: dict of (3n, ...) arrays, one row per ray."""
    n = len(radius)
    out = np.zeros((3 * n, 9), np.uint32)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (radius, org, dirs, bounds)]
    assert _host().sphere_host(*(H.P(a) for a in arrs), ctypes.c_size_t(n), H.P(out)) == 0
    f = lambda cols: out[:, cols].view(np.float32)
    return {"hit": out[:, 0] != 0, "t": f(slice(1, 2)), "delta": f(slice(2, 3)), "hitN": out[:, 3] != 0, "tN": f(slice(4, 5)),
            "distance": f(slice(5, 6)), "position": f(slice(6, 9))}


@pytest.mark.parametrize("which", ["constructed", "random"])
def test_device_headers_on_the_host(which):
    """sphere_hit of pt_device.h, compiled for the host: the oracle's verdict, and the oracle's distance and position from its t as
    object_hit and surface_of form them (the normal of a sphere at the origin is its position).  sphere_hitN<3> - the tangent root
    behind the ballot, here of the set's own three rays - returns sphere_hit's {hit, t} everywhere."""
    sets, rays, rec = constructed() if which == "constructed" else randoms()
    family = np.repeat(sets[4], 3) if which == "constructed" else np.zeros(len(rays[0]), np.int64)
    h = host_sphere(*sets[:4])
    want = rec["identity"]
    hit = want[:, 0] != 0
    got = np.concatenate([h["hit"][:, None].astype(np.float32), h["distance"], h["position"], h["position"]], axis=1)
    got[~hit & ~h["hit"]] = 0.0                                            # (a miss is the default Trace)
    assert_records_equal(got, want, family, f"sphere_hit on the host against the oracle, {which} sets")
    bad = np.flatnonzero((h["hitN"] != h["hit"]) | ~same(h["tN"], h["t"])[:, 0])
    assert bad.size == 0, ("sphere_hitN differs from sphere_hit", len(bad), sorted({S.FAMILIES[f] for f in family[bad]}), bad[:5])
    with np.errstate(invalid="ignore"):
        zero = h["delta"][:, 0] == 0
    print(f"{which}: {len(hit)} rays, hits {int(hit.sum())}, delta == 0 on {int(zero.sum())}")
    assert h["hit"][zero].all()                                            # the tangent branch checks nothing
    if which == "constructed":
        assert zero.sum() > 1000
    else:
        assert 0.1 < hit.mean() < 0.9
