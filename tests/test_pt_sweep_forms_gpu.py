"""GPU: the sweeps of the wave kernel in the forms csrc/pt_wave.h and csrc/pt_trace.h give them - BBox::hit with both products
per axis and the select on the results (box_hit_inv), the bottom-up sweep on the two-word hit (packed_fold, packed_combine).

  * box_hit_inv against box_hit_rec, the form the per-lane traversals keep (the bound selected first), through
    srt_pt_math_box_sweep: {hit, times.x, times.y} bit for bit, NaN == NaN as in the other parity tests, on random sets in and
    around the unit box and on sets built around every special operand.
  * images: the wave form (kernel mode 2; mode 7, the streamed sweeps, where a mesh has a real BVH<Triangle>) against the
    lane-per-sample form (mode 4), which walks the trees per lane and shares none of the sweep code: equal bits, equal ray counts.

BVH<Object> is built with max_leaf_size 1 (rays/object.h), so a BVH<Object> leaf never holds more than one object and its root is
a leaf only for a one-object scene; the ordered fold over several objects (the `Q == 0` fold) is what List<Object> runs
(use_bvh = False).  The scenes below therefore go through both containers."""
import itertools

import numpy as np
import pytest

from _cases import pt_scene

pytestmark = pytest.mark.gpu

F = np.float32
NAN, INF = F(np.nan), F(np.inf)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def pt(srt):
    p = srt.Pathtracer(0)
    yield p
    p.close()


def _same(got, want):
    for key in ("hit", "tx", "ty"):
        a, b = got[key], want[key]
        ok = (a == b) if key == "hit" else ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
        bad = np.argwhere(~ok)
        assert bad.size == 0, (key, len(bad), bad[:5].ravel(), a[~ok][:5], b[~ok][:5])


def random_box_sets(seed, n):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-1.0, 1.0, (n, 3))
    box = np.concatenate([np.minimum(a, b), np.maximum(a, b)], axis=1).astype(F)
    box[: n // 4] = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], F)               # the unit box itself
    org = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3)).astype(F)
    d[rng.random((n, 3)) < 0.05] = 0.0                                            # axis-parallel rays: 1 / 0 = inf
    d[rng.random((n, 3)) < 0.02] = -0.0
    with np.errstate(divide="ignore"):
        inv = (F(1.0) / d).astype(F)
    times = np.sort(rng.uniform(0.0, 4.0, (n, 2)), axis=1).astype(F)
    wide = rng.random(n) < 0.5
    times[wide] = (0.0, INF)                                                      # the camera's dist_bounds
    return box, org, inv, times


def constructed_box_sets():
    """Per axis every pairing of a reciprocal direction {+-inf (direction +-0 or denormal), +-huge, both signs of ordinary values, NaN}
    with an origin {inside, on the lower face, on the upper face (0 * inf), outside on either side, NaN}; the box (unit, degenerate
    min == max on one / every axis, off-centre) and the incoming times (wide, narrow, tx > ty, NaN) cycle along; then a NaN in each
    of the 14 operands of a ray that hits."""
    with np.errstate(divide="ignore", over="ignore"):
        inv_of = [F(1.0) / F(v) for v in (0.0, -0.0, 1e-40, -1e-40, 1e-38, -1e-38)]    # +inf, -inf, +inf, -inf (denormals), +-huge
    invs = inv_of + [F(1.0), F(-1.0), F(2.5), F(-0.3), NAN]
    orgs = [F(0.2), F(-0.5), F(0.5), F(-2.0), F(2.0), NAN]
    axis = list(itertools.product(invs, orgs))
    idx = np.array(list(itertools.product(range(len(axis)), repeat=3)))
    inv = np.array([[axis[j][0] for j in row] for row in idx], F)
    org = np.array([[axis[j][1] for j in row] for row in idx], F)
    boxes = np.array([[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], [-0.5, -0.5, 0.5, 0.5, 0.5, 0.5], [0.2, -0.5, 0.5, 0.2, -0.5, 0.5],
                      [-0.5, -2.0, -0.25, 2.0, 0.5, 0.75], [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]], F)
    times = np.array([[0.0, INF], [0.1, 5.0], [3.0, 1.0], [NAN, 1.0], [0.0, NAN], [0.0, 0.0], [0.7, 0.7]], F)
    n = len(idx)
    k = np.arange(n)
    box, tm = boxes[k % len(boxes)], times[(k // len(boxes)) % len(times)]
    base = np.array([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5, 0.1, 0.2, -2.0, 10.0, -8.0, 1.0, 0.0, 100.0], F)
    nan_rows = np.tile(base, (15, 1))
    for j in range(14):
        nan_rows[j, j] = NAN
    return (np.concatenate([box, nan_rows[:, 0:6]]), np.concatenate([org, nan_rows[:, 6:9]]), np.concatenate([inv, nan_rows[:, 9:12]]),
            np.concatenate([tm, nan_rows[:, 12:14]]))


def test_box_random_sets(pt):
    box, org, inv, times = random_box_sets(41, 1 << 18)
    new, rec = pt.math_box_sweep(box, org, inv, times)
    print("random sets: hits", int(rec["hit"].sum()), "of", rec["hit"].size, "- times narrowed:", int((rec["tx"] != times[:, 0]).sum()))
    assert 0.05 < rec["hit"].mean() < 0.95            # both verdicts
    assert (rec["tx"] != times[:, 0]).any() and (rec["ty"] != times[:, 1]).any()
    _same(new, rec)


def test_box_constructed_sets(pt):
    box, org, inv, times = constructed_box_sets()
    new, rec = pt.math_box_sweep(box, org, inv, times)
    print("constructed sets:", len(box), "hits", int(rec["hit"].sum()), "NaN times out", int(np.isnan(rec["tx"]).sum()))
    assert rec["hit"].any() and not rec["hit"].all()
    assert rec["hit"][-15:].all()      # the base ray hits, and so does every copy with a NaN operand: BBox::hit's early-outs are `>` comparisons
    _same(new, rec)


# ------------------------------------------------------------------------------------------------
# images
# ------------------------------------------------------------------------------------------------
def _colmajor_translate(t, s=1.0):
    m = np.eye(4, dtype=F)
    m[0, 0] = m[1, 1] = m[2, 2] = F(s)
    m[:3, 3] = t
    return np.ascontiguousarray(m.T.reshape(16))


def three_objects():
    """The floor, a sphere and the light of the Cornell box."""
    s = pt_scene("cbox_lambertian")
    s["objects"] = [s["objects"][4], s["objects"][5], s["objects"][7]]
    return s


def light_only():
    s = pt_scene("cbox_lambertian")
    s["objects"] = [s["objects"][7]]
    return s


def twelve_small():
    """Floor and light of the Cornell box, six small spheres and four small quads; two of the quads lie in one plane and overlap
    (equal distances where they do: Trace::min keeps the later one; their centres differ, or BVH::build would never separate them)
    and most rays miss most objects."""
    from soft_rendering_toolsets_amd import scenes

    s = pt_scene("cbox_lambertian")
    floor, light = s["objects"][4], s["objects"][7]
    objs = [floor]
    rng = np.random.default_rng(12)
    for k in range(6):
        t = (rng.uniform(-0.4, 0.4), rng.uniform(0.1, 0.7), rng.uniform(-0.4, 0.3))
        objs.append({"kind": "sphere", "radius": 0.07 + 0.01 * k, "T": _colmajor_translate(t), "material": k % 5})
    p, n, i = scenes.flat_mesh(scenes._SQUARE_POS, scenes._SQUARE_TRIS)
    quads = [(-0.2, 0.3, 0.1), (0.25, 0.5, -0.2), (0.2, 0.42, 0.0), (0.2625, 0.42, 0.0)]
    for k, t in enumerate(quads):
        objs.append({"kind": "mesh", "pos": p, "nrm": n, "idx": i, "T": _colmajor_translate(t, 0.3), "material": (k + 1) % 5, "is_light": False})
    objs.append(light)
    s["objects"] = objs
    assert len(objs) == 12
    return s


IMAGE_CASES = [
    # name, scene, use_bvh, (w, h), wave-form modes
    ("cbox", lambda: pt_scene("cbox"), True, (64, 64), (2,)),
    ("cbox_lambertian", lambda: pt_scene("cbox_lambertian"), True, (64, 64), (2,)),
    ("three_objects_list", three_objects, False, (64, 64), (2,)),           # the fold over every object (Q == 0)
    ("light_only_root_leaf", light_only, True, (64, 64), (2,)),            # one object: the BVH<Object> root is a leaf
    ("twelve_small_bvh", twelve_small, True, (64, 64), (2,)),               # eleven interior nodes: the combine at every depth
    ("twelve_small_list", twelve_small, False, (64, 64), (2,)),             # the twelve-object fold: ties and misses on both sides
    ("cbox_blob512_glass", lambda: pt_scene("cbox_blob512_glass"), True, (32, 32), (2, 7)),   # lazy leaf (mode 2) and the streamed sweeps
]


@pytest.mark.parametrize("name,make,use_bvh,wh,modes", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_wave_form_equals_lane_per_sample(srt, name, make, use_bvh, wh, modes):
    scene = make()
    w, h = wh
    p = srt.Pathtracer(0)
    p.set_params(w, h, 1, 4, use_bvh)
    p.build_scene(scene)
    p.set_camera(scene["camera"])
    try:
        p.set_kernel(4)
        p.ray_count(reset=True)
        want = p.render_epoch(0, 0, 6)
        want_rays = p.ray_count(reset=True)[0]
        assert want_rays > 0 and np.isfinite(want).any()
        for mode in modes:
            p.set_kernel(mode)
            got = p.render_epoch(0, 0, 6)
            rays = p.ray_count(reset=True)[0]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{name}: kernel mode {mode} differs from mode 4 in {int((~same).sum())} values"
            assert rays == want_rays, f"{name}: kernel mode {mode} counted {rays} rays, mode 4 {want_rays}"
    finally:
        p.close()
