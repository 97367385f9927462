"""GPU: the top-down sweep's min / max step behind its no-NaN guard (box_hit_minmax, topdown_step<true>, csrc/pt_trace.h; the guard and
the loop of csrc/pt_wave.h) and the sweeps' flag nibbles in the dead slot word.

srt_pt_math_topdown_minmax: seven-node trees, one per wave of 64 lanes, 1024 waves a launch; the guarded sweep against the sweep through
the old step alone, bit for bit per lane and node (flags, cur_far_t.x, both children's times), and the path every wave took against
what the guard's predicate says on the host: waves built to pass; waves with exactly one bad lane - an axis-parallel direction (an
infinite reciprocal), a NaN origin, a zero reciprocal; and a launch whose trees hold a non-finite box, or an inverted one: every
wave on the old step.

Renders, 64 x 64, 8 spp, depth 8: the wave forms (kernel modes 2, 3, two-ray batches, and 7 where a mesh has a real BVH<Triangle>)
against the lane-per-sample form, equal image bits and ray counts: the box, the Lambertian box, the box through a camera of aspect
ratio zero that looks down -z (every camera ray has direction.x == 0: the bursts' waves fall back, waves of bounces do not), the box
with a sphere of infinite radius (a non-finite box: the whole launch on the old step), and cornell_with_mesh(3) (the lazy and the
streamed sweeps carry their flags through the slots as well)."""
import numpy as np
import pytest

from _cases import pt_scene

pytestmark = pytest.mark.gpu

F = np.float32
WAVES = 1024
KINDS = ("passes", "axis-parallel lane", "NaN origin lane", "zero reciprocal lane")


def _trees(rng, W):
    """(W, 7, 16) uint32 records of complete trees: node q has children 2q+1, 2q+2 (q < 3) or two leaves; boxes are the unions of eight
    random leaf boxes."""
    c = rng.uniform(-0.8, 0.8, (W, 8, 3))
    e = rng.uniform(0.02, 0.3, (W, 8, 3))
    lo = {7 + k: (c[:, k] - e[:, k]).astype(F) for k in range(8)}
    hi = {7 + k: (c[:, k] + e[:, k]).astype(F) for k in range(8)}
    for q in range(6, -1, -1):
        lo[q] = np.minimum(lo[2 * q + 1], lo[2 * q + 2])
        hi[q] = np.maximum(hi[2 * q + 1], hi[2 * q + 2])
    rec = np.zeros((W, 7, 16), np.uint32)
    fl = rec.view(F)
    for q in range(7):
        l, r = 2 * q + 1, 2 * q + 2
        fl[:, q, 0:3], fl[:, q, 3:6], fl[:, q, 6:9], fl[:, q, 9:12] = lo[l], hi[l], lo[r], hi[r]
        rec[:, q, 12] = l if l < 7 else (~(l - 7)) & 0xFFFFFFFF     # a leaf: ~(its first object)
        rec[:, q, 13] = r if r < 7 else (~(r - 7)) & 0xFFFFFFFF
        rec[:, q, 14] = rec[:, q, 15] = 0 if l < 7 else 1
    return rec


def _rays(rng, W, all_pass=False):
    """(W * 64, 10) rays towards the boxes and the kind of each wave; a wave of a bad kind has exactly one lane outside the guard."""
    n = W * 64
    org = rng.uniform(-2, 2, (n, 3)).astype(F)
    d = (rng.uniform(-0.7, 0.7, (n, 3)).astype(F) - org).astype(F)
    d = np.where(d == 0, F(0.125), d)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    kind = rng.integers(0, len(KINDS), W)
    kind[:8] = np.arange(8) % len(KINDS)
    if all_pass:
        kind[:] = 0
    lane = rng.integers(0, 64, W)
    lane[:8] = (0, 0, 0, 0, 63, 63, 63, 63)
    axis = rng.integers(0, 3, W)
    bad = np.arange(W) * 64 + lane
    with np.errstate(divide="ignore"):
        k1 = bad[kind == 1]
        d[k1, axis[kind == 1]] = 0.0                      # an axis-parallel direction in the plane: 1 / 0 = inf
        inv = (F(1) / d).astype(F)
    org[bad[kind == 2], axis[kind == 2]] = np.nan
    inv[bad[kind == 3], axis[kind == 3]] = rng.choice(np.array([0.0, -0.0], F), int((kind == 3).sum()))
    cam = rng.random(n) < 0.5
    rb = np.stack([np.where(cam, F(0), F(0.001)), np.where(cam, F(np.inf), np.finfo(F).max)], axis=1).astype(F)
    return np.ascontiguousarray(np.concatenate([org, inv, rb, rb], axis=1), F), kind


def _predicate(rec, rays):
    """The guard on the host, per wave: every bound finite with lo <= hi, every lane's origin finite, its reciprocals finite and not zero."""
    box = rec.view(F)[:, :, :12].reshape(len(rec), 7, 2, 2, 3)            # node, side, lo / hi, axis
    with np.errstate(invalid="ignore"):
        boxes_ok = (np.isfinite(box).all(axis=(1, 2, 3, 4))) & (box[:, :, :, 0] <= box[:, :, :, 1]).all(axis=(1, 2, 3))
    org, inv = rays[:, 0:3], rays[:, 3:6]
    lane_ok = np.isfinite(org).all(axis=1) & np.isfinite(inv).all(axis=1) & (inv != 0).all(axis=1)
    return boxes_ok & lane_ok.reshape(-1, 64).all(axis=1)


def _run(rec, rays):
    import srt_amd

    pt = srt_amd.Pathtracer(0)
    try:
        return pt.math_topdown_minmax(rec, rays)
    finally:
        pt.close()


def _check(rec, rays, what):
    got, old, took = _run(rec, rays)
    diff = np.argwhere((got != old).any(axis=(1, 2))).ravel()
    assert diff.size == 0, (what, len(diff), diff[:5], got[diff[:2]], old[diff[:2]])
    want = _predicate(rec, rays)
    assert np.array_equal(took, want), (what, np.argwhere(took != want).ravel()[:8])
    flags = np.bincount(got[:, :, 0].ravel(), minlength=16)
    assert flags[[1, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14]].sum() == 0, flags
    return took, flags


def test_guarded_sweep_equals_the_old_step_and_takes_the_predicted_path():
    rng = np.random.default_rng(2024)
    rec = _trees(rng, WAVES)
    rays, kind = _rays(rng, WAVES)
    took, flags = _check(rec, rays, "finite trees")
    assert np.array_equal(took, kind == 0)                # exactly the waves without a bad lane
    assert 100 < took.sum() < WAVES - 100
    assert all(flags[f] > 1000 for f in (0, 2, 5, 11, 15)), flags
    print("waves on the min / max step:", int(took.sum()), "of", WAVES, "flag nibbles:", flags)


@pytest.mark.parametrize("what", ["infinite bound", "NaN bound", "inverted box"])
def test_a_launch_with_a_bad_box_stays_on_the_old_step(what):
    rng = np.random.default_rng(7)
    rec = _trees(rng, WAVES)
    rays, _ = _rays(rng, WAVES, all_pass=True)            # every lane inside the guard: the boxes alone decide
    fl = rec.view(F)
    node, side = rng.integers(0, 7, WAVES), rng.integers(0, 2, WAVES)
    axis = rng.integers(0, 3, WAVES)
    w = np.arange(WAVES)
    if what == "infinite bound":                          # what a sphere of infinite radius makes of the boxes above it
        fl[w, node, 6 * side + 3 + axis] = np.inf
        fl[w, node, 6 * side + axis] = -np.inf
    elif what == "NaN bound":
        fl[w, node, 6 * side + 3 * rng.integers(0, 2, WAVES) + axis] = np.nan
    else:
        lo, hi = fl[w, node, 6 * side + axis].copy(), fl[w, node, 6 * side + 3 + axis].copy()
        fl[w, node, 6 * side + axis], fl[w, node, 6 * side + 3 + axis] = hi, lo
    took, _ = _check(rec, rays, what)
    assert not took.any()


def _axis_parallel_camera(scene):
    s = dict(scene)
    iview = np.eye(4, dtype=F)
    iview[:3, 3] = (0.0, 0.5, 1.2)
    s["camera"] = {"iview": np.ascontiguousarray(iview.T.reshape(16)), "vfov": 60.0, "ar": 0.0}
    return s


def _infinite_sphere(scene):
    s = dict(scene)
    s["objects"] = list(s["objects"])
    assert s["objects"][5]["kind"] == "sphere"
    s["objects"][5] = dict(s["objects"][5], radius=np.inf)
    return s


RENDERS = {
    "box": (lambda: pt_scene("cbox"), (2, 3, "two-ray")),
    "lambertian-box": (lambda: pt_scene("cbox_lambertian"), (2, 3, "two-ray")),
    "axis-parallel-camera": (lambda: _axis_parallel_camera(pt_scene("cbox")), (2, 3, "two-ray")),
    "infinite-sphere": (lambda: _infinite_sphere(pt_scene("cbox")), (2, 3, "two-ray")),
    "mesh-512": (lambda: pt_scene("cbox_blob512_glass"), (2, 3, 7)),     # scenes.cornell_with_mesh(3)
}


@pytest.mark.parametrize("name", list(RENDERS))
def test_wave_forms_equal_lane_per_sample(name):
    import srt_amd

    make, modes = RENDERS[name]
    scene = make()
    p = srt_amd.Pathtracer(0)
    p.set_params(64, 64, 8, 8, True)
    p.build_scene(scene)
    p.set_camera(scene["camera"])
    try:
        p.set_kernel(4)
        p.ray_count(reset=True)
        want = p.render_epoch(0, 0, 8)
        want_rays = p.ray_count(reset=True)[0]
        assert want_rays > 64 * 64 * 8 and np.isfinite(want).any()
        for mode in modes:
            p.set_kernel(2 if mode == "two-ray" else mode)
            p.set_elision(mode == "two-ray")
            got = p.render_epoch(0, 0, 8)
            rays = p.ray_count(reset=True)[0]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{name}: kernel mode {mode} differs from mode 4 in {int((~same).sum())} values"
            assert rays == want_rays, f"{name}: kernel mode {mode} counted {rays} rays, mode 4 {want_rays}"
    finally:
        p.close()
