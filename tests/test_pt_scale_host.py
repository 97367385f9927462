"""CPU: the path tracer's worlds off unit scale (tests/_scale_cases.py) - conditions on the inputs, the host emulation of the
traversal headers, and the host-only context.

The kernels choose code by the magnitude of their operands: Triangle::hit divides on an exact fast path only while |det|, |nu|,
|nv|, |nt| lie in [2^-40, 2^40] (csrc/pt_device.h:div_in_range, one ballot per wave), sqrtN has a window of its own, the
wave-uniform Mat4 * Vec3 skips the perspective divide while w == 1, and the flattened walk drops a stack frame on an argument
about finite reciprocals.  The cases put those choices on both sides; this module checks that they do (the share conditions),
that the paths stay real (the liveness conditions), and everything that needs no device.  tests/test_pt_scale_gpu.py renders."""
import ctypes
import functools

import numpy as np
import pytest

import _harness as H
import _scale_cases as SC
from _cases import camera_rays, pt_sample_list, pt_scene
from _refit_cases import tree_cost_numpy
from test_pt_tri_verdict_host import _host as tri_verdict_lib, _run as tri_verdict_run

F32 = np.float32
W, HGT = 24, 18
IDS = [SC.case_id(c) for c in SC.CASES]
DUMP_CAP = 1 << 12


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


# ------------------------------------------------------------------------------------------------
# Share conditions
# ------------------------------------------------------------------------------------------------
def _f32_point(m, v):
    """Mat4 * Vec3 in float32, the operation order of csrc/pt_device.h:mat_point; m[row, col]."""
    o = [((m[j, 0] * v[:, 0] + m[j, 1] * v[:, 1]) + m[j, 2] * v[:, 2]) + m[j, 3] * F32(1.0) for j in range(4)]
    return np.stack([o[0] / o[3], o[1] / o[3], o[2] / o[3]], 1)


def _f32_rotate(m, v):
    return np.stack([((m[j, 0] * v[:, 0] + m[j, 1] * v[:, 1]) + m[j, 2] * v[:, 2]) + m[j, 3] * F32(0.0) for j in range(3)], 1)


def window_share(scene, w, h):
    """Shares of pairs inside the exact-division window, by the product's own div_in_range (tests/host_emu/tri_verdict_host.cpp),
    for one camera ray per pixel (jitter 0.5, 0.5) carried into each object's space the way Ray::transform does it (float32; the
    inverse matrix from float64):
      "tri"    (ray, object-space triangle) pairs of Triangle::hit's divide, every triangle of every mesh (out[0]);
      "xform"  (ray, posed object) pairs of Ray::transform's own divide, the rotated direction over its norm.
    Ray::transform normalises the direction, so with unit geometry the triangle test sees unit rays at EVERY pose scale: what a
    scale in the pose crosses is the second window, what a scale in the geometry crosses is the first."""
    org, d, _ = camera_rays(scene["camera"], w, h, jitters=((0.5, 0.5),))
    inside = {"tri": 0, "xform": 0}
    total = {"tri": 0, "xform": 0}
    with np.errstate(all="ignore"):
        for o in scene["objects"]:
            T = np.asarray(o["T"], F32).reshape(4, 4).T.astype(np.float64)
            iT = np.linalg.inv(T).astype(F32)
            oo = _f32_point(iT, org)
            rd = _f32_rotate(iT, d)
            dn = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
            if not np.array_equal(T, np.eye(4)):                                                  # has_trans
                out = np.zeros(len(rd), np.uint32)
                num, den = np.ascontiguousarray(rd, F32), np.ascontiguousarray(dn, F32)
                assert tri_verdict_lib().div_window_host(H.P(num), H.P(den), ctypes.c_size_t(len(rd)), H.P(out)) == 0
                inside["xform"] += int(out.sum())
                total["xform"] += len(rd)
            if o["kind"] != "mesh":
                continue
            od = rd / dn[:, None]
            v = np.asarray(o["pos"], F32)[np.asarray(o["idx"], np.uint32).reshape(-1, 3)]
            tri = np.concatenate([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], 1)             # p0, e1, e2
            n, m = len(oo), len(tri)
            out = tri_verdict_run(np.repeat(tri, n, axis=0), np.tile(oo, (m, 1)), np.tile(np.tile(od, (1, 3)), (m, 1)),
                                  np.tile(np.array([0, np.inf] * 3, F32), (n * m, 1)))
            inside["tri"] += int((out[:, 0, 0] != 0).sum())
            total["tri"] += n * m
    return {k: inside[k] / total[k] for k in inside}


@functools.lru_cache(maxsize=None)
def _share(name):
    return window_share(pt_scene(name), W, HGT)


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_share_of_pairs_inside_the_division_window(case):
    """A condition on the inputs, not a measurement: a mixed case has 5 % to 95 % of its pairs inside the window its scaling
    moves, an outside case none, the unit scene all of both.  A case that misses its band gets another exponent, not another band."""
    name, group, _ = case
    shares = _share(name)
    share = shares[SC.window_of(name)]
    print(f"{name}: share of pairs inside the window: Triangle::hit {shares['tri']:.4f}, Ray::transform {shares['xform']:.4f}")
    if group == "mixed":
        assert 0.05 <= share <= 0.95
    elif group == "outside":
        assert share == 0.0
    elif group == "unit":
        assert shares == {"tri": 1.0, "xform": 1.0}
    if "@pose:" in name:
        assert shares["tri"] == 1.0                  # Ray::transform normalises: unit rays meet unit triangles at any pose scale


# ------------------------------------------------------------------------------------------------
# Liveness conditions
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_samples(name, use_bvh):
    o = H.OraclePT(pt_scene(name), W, HGT, SC.DEPTH, use_bvh)
    xs, ys, ss = pt_sample_list(5, W, HGT, 400)
    return o.trace_samples(5, xs, ys, ss)


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_paths_stay_real(case):
    """From the oracle alone: at least 90 % of the samples finite and 10 or more RNG draws per sample on average (a camera ray
    that only escapes draws 2).  The degenerate cases are exempt: EPS_F is absolute, little is left of their paths.
    lone_blob_env cannot reach 10 draws anywhere - where it stands in the unit world it has 2.2, most rays of the box's camera
    pass its one object - so its moved forms are held to the finite share and to what the unmoved scene draws."""
    name, group, use_bvh = case
    rgb, draws, _ = _oracle_samples(name, use_bvh)
    finite, mean_draws = float(np.isfinite(rgb).all(axis=1).mean()), float(draws.mean())
    print(f"{name}: {finite:.3f} finite, {mean_draws:.1f} draws per sample")
    if group == "moved-sparse":
        unmoved = float(_oracle_samples(name.split("@")[0], use_bvh)[1].mean())
        assert finite >= 0.9 and mean_draws >= unmoved
    elif group != "degenerate":
        assert finite >= 0.9 and mean_draws >= 10.0


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_oracle_equals_reference_build(case):
    """Where the reference build is present: the oracle's radiance, draw ledger and scene.hit equal the reference's in every
    world, so nothing here needs a tolerance.  (The committed fixtures of a subset hold it elsewhere: tests/test_pt_oracle.py.)"""
    if H.ref_pt_lib() is None:
        return
    name, _, use_bvh = case
    scene = pt_scene(name)
    ref = H.RefPT(scene, W, HGT, SC.DEPTH, use_bvh)
    xs, ys, ss = pt_sample_list(5, W, HGT, 400)
    rgb, draws = ref.trace_samples(5, xs, ys, ss)
    got = H.OraclePT(scene, W, HGT, SC.DEPTH, use_bvh, math_mode=0).trace_samples(5, xs, ys, ss)
    assert bits_equal(got[0], rgb) and np.array_equal(got[1], draws)
    got = _oracle_samples(name, use_bvh)
    assert bits_equal(got[0], rgb) and np.array_equal(got[1], draws)
    org, d, b = SC.scaled_rays("random_rays", 6, 1024, scene)
    assert bits_equal(H.OraclePT(scene, W, HGT, SC.DEPTH, use_bvh).hit(org, d, b), ref.hit(org, d, b))


# ------------------------------------------------------------------------------------------------
# Host emulation of the traversal headers
# ------------------------------------------------------------------------------------------------
def _records_equal(a, b):
    """{hit, distance bits, object slot, triangle} records: equal, the distance as a float with a NaN equal to a NaN (at 2^50 some
    distances are NaN, and the sign bit of a NaN is the host compiler's choice, not the device's)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(a[:, [0, 2, 3]], b[:, [0, 2, 3]]) and bits_equal(a[:, 1].copy().view(F32), b[:, 1].copy().view(F32))


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_flat_walk_equals_nested_and_oracle(case):
    """tests/test_pt_flat_host.py's loop over the worlds: nested walk == flattened walk == the oracle's scene.hit for every batch
    slot, with rays carried into the world.  It holds the flattened walk's no-frame shortcut to account where the slab products
    (b - o) * inv overflow or underflow."""
    name, group, use_bvh = case
    scene = pt_scene(name)
    emu = H.EmuPT(scene, use_bvh)
    oracle = H.OraclePT(scene, 8, 8, 8, use_bvh)
    hits = 0
    for kind, seed in (("random_rays", 11), ("unnormalised_rays", 12)):
        org, dirs, bounds = SC.scaled_rays(kind, seed, 2000, scene)
        o = oracle.hit(org, dirs, bounds)
        for slot in range(3):
            nested, flat = emu.hit(org, dirs, bounds, slot)
            assert _records_equal(nested, flat), f"{kind} slot {slot}: flattened walk differs from the nested form"
            assert np.array_equal(nested[:, 0], o[:, 0].astype(np.uint32))
            assert bits_equal(nested[:, 1].view(F32)[nested[:, 0] == 1], o[:, 1][nested[:, 0] == 1]), "distances differ from the oracle"
        hits += int(o[:, 0].sum())
        n = 600
        d3 = dirs[:3 * n].reshape(n, 9)
        got = emu.hit3(org[:n], d3, bounds[:n])
        for s in range(3):
            want, _ = emu.hit(org[:n], np.ascontiguousarray(d3[:, 3 * s:3 * s + 3]), bounds[:n], 0)
            assert _records_equal(got[:, s], want)
    if group not in ("degenerate", "projective") and "lone_blob" not in name:
        assert hits > 1000, "the rays were not carried into the world"          # (the unit box: 1215 of the 4000)
    emu.close()


# ------------------------------------------------------------------------------------------------
# Host-only context
# ------------------------------------------------------------------------------------------------
def _host_pt(srt, use_bvh=True):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, SC.DEPTH, use_bvh)
    return pt


def _dumps_equal_oracle(srt, pt, oracle, nobj):
    """Both tree levels of the product's host build against the oracle's; returns the product's dumps by slot."""
    dumps = {}
    for k in range(-1, nobj):
        want = oracle.dump_bvh(k, cap=DUMP_CAP)
        if want is None:
            with pytest.raises(srt.SrtError):
                pt.dump_bvh(k, cap=DUMP_CAP)
            continue
        boxes, links, order = pt.dump_bvh(k, cap=DUMP_CAP)
        n = nobj if k < 0 else int(want[1][0][1])
        assert bits_equal(boxes, want[0]) and np.array_equal(links, want[1]) and np.array_equal(order[:n], want[2][:n]), f"tree {k}"
        dumps[k] = (boxes, links, order)
    return dumps


# SAH figures of the cases whose costs are pinned to a recorded value: srt_pt_scene_tree_cost (-1) and, by insertion index,
# srt_pt_mesh_tree_cost of the non-light meshes.  A scale in the pose scales every box of the BVH<Object> exactly, so the ratios of
# areas - the cost - are the unit scene's; BBox::transform uses the affine part of a matrix only, so a projective row leaves them
# the unit scene's too; a scale in the geometry does not: a flat wall's box is given an absolute thickness.
RECORDED_COSTS = {
    'cbox': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@geom:-15': {-1: 1.6250952526193714, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox_blob512_glass@geom:-15': {-1: 1.6250952526366091, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0, 6: 21.926084341948247},
    'cbox_deltalights@geom:-15': {-1: 1.6250952526193714, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox_spherelight@geom:-15': {-1: 1.6250952527409135, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@geom:21': {-1: 7.38745767257545, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox_blob512_glass@geom:21': {-1: 7.549331468361233, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0, 6: 21.926084341948247},
    'cbox_deltalights@geom:21': {-1: 7.38745767257545, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox_spherelight@geom:21': {-1: 8.407470699565229, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@pose:42': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@pose:-42': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@pose:50': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@geom:-20': {-1: 1.7500031451444151, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@proj:spheres': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@proj:walls': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'cbox@proj:mixed': {-1: 7.674739926742686, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0},
    'random303@proj:mixed': {-1: 8.202275813401915, 0: 2.0, 1: 2.0, 2: 2.0, 3: 2.0, 4: 2.0, 6: 6.20100536334419, 8: 9.901367751949197, 10: 2.0, 11: 6.179169295686764},
}


@pytest.mark.parametrize("case", SC.CASES, ids=IDS)
def test_host_build_equals_oracle_and_tree_costs(srt, case):
    name, group, use_bvh = case
    scene = pt_scene(name)
    nobj = len(scene["objects"])
    pt = _host_pt(srt, use_bvh)
    pt.build_scene(scene)
    if not use_bvh:                                   # list mode: no trees to dump or to cost
        with pytest.raises(srt.SrtError):
            pt.scene_tree_cost()
        pt.close()
        return
    dumps = _dumps_equal_oracle(srt, pt, H.OraclePT(scene, 8, 8, SC.DEPTH, True), nobj)
    assert -1 in dumps
    slot_of = {int(dumps[-1][2][k]) - 1: k for k in range(nobj)}                  # insertion index -> slot
    costs = {-1: pt.scene_tree_cost()}
    for index, o in enumerate(scene["objects"]):
        if o["kind"] == "mesh" and not o["is_light"]:
            costs[index] = pt.mesh_tree_cost(index)
    for index, cost in costs.items():
        boxes, links, _ = dumps[-1 if index < 0 else slot_of[index]]
        assert np.isfinite(cost) and cost > 0.0
        assert abs(cost - tree_cost_numpy(boxes, links)) <= 1e-12 * cost, (index, cost)
    print(f"{name!r}: {costs!r},")
    if not group.startswith(("mixed", "moved")):
        assert costs == RECORDED_COSTS[name]
    pt.close()


@pytest.mark.parametrize("name", SC.REFUSED)
def test_refused_commits(srt, name):
    """What the reference's BVH build does not finish - its plane loop stalls on the axis-aligned Cornell box once it is translated
    or scaled by a factor that is no power of two, and on geometry of 2^-38 - the oracle refuses (-2) and so does the product:
    an SrtError, no hang, and the context commits the next scene as if nothing had happened.  No device."""
    scene = pt_scene(name)
    with pytest.raises(AssertionError, match="oracle commit failed"):
        H.OraclePT(scene, 8, 8, SC.DEPTH, True)
    pt = _host_pt(srt)
    with pytest.raises(srt.SrtError):
        pt.build_scene(scene)
    with pytest.raises(srt.SrtError):
        pt.scene_tree_cost()                          # nothing is committed
    unit = pt_scene("cbox")
    pt.build_scene(unit)
    _dumps_equal_oracle(srt, pt, H.OraclePT(unit, 8, 8, SC.DEPTH, True), len(unit["objects"]))
    pt.close()
    lst = _host_pt(srt, use_bvh=False)                # the same scene without BVHs has no plane loop to stall
    lst.build_scene(scene)
    lst.close()


# ------------------------------------------------------------------------------------------------
# The functions themselves
# ------------------------------------------------------------------------------------------------
def test_world_functions():
    """pose_scaled / geom_scaled / translated / projective do what their names say, exactly, and leave their argument alone."""
    from _cases import scene_digest

    base = pt_scene("cbox_spherelight")
    before = scene_digest(base)
    rows = lambda T: np.asarray(T, F32).reshape(4, 4).T
    g, p, t = SC.geom_scaled(base, 2.0 ** 14), SC.pose_scaled(base, 2.0 ** -13), SC.translated(base, (8, -16, 4))
    for k, o in enumerate(base["objects"]):
        m = rows(o["T"])
        assert np.array_equal(rows(g["objects"][k]["T"])[:3, :3], m[:3, :3]) and np.array_equal(rows(g["objects"][k]["T"])[:3, 3], m[:3, 3] * F32(2.0 ** 14))
        assert np.array_equal(rows(p["objects"][k]["T"])[:3], m[:3] * F32(2.0 ** -13)) and np.array_equal(rows(p["objects"][k]["T"])[3], m[3])
        assert np.array_equal(rows(t["objects"][k]["T"])[:3, 3], (m[:3, 3].astype(np.float64) + [8, -16, 4]).astype(F32))
        if o["kind"] == "mesh":
            assert np.array_equal(g["objects"][k]["pos"], o["pos"] * F32(2.0 ** 14)) and g["objects"][k]["nrm"] is o["nrm"]
            assert p["objects"][k]["pos"] is o["pos"]
        else:
            assert F32(g["objects"][k]["radius"]) == F32(o["radius"]) * F32(2.0 ** 14) and p["objects"][k]["radius"] == o["radius"]
    lm = base["objects"][8]["light_mesh"]["pos"]
    assert np.array_equal(g["objects"][8]["light_mesh"]["pos"], lm * F32(2.0 ** 14))
    assert np.array_equal(rows(g["camera"]["iview"])[:3, 3], rows(base["camera"]["iview"])[:3, 3] * F32(2.0 ** 14))
    assert np.array_equal(rows(p["camera"]["iview"])[:3], rows(base["camera"]["iview"])[:3] * F32(2.0 ** -13))
    d = pt_scene("cbox_deltalights@geom:-13")
    assert np.array_equal(rows(d["lights"][0]["T"])[:3, 3], rows(pt_scene("cbox_deltalights")["lights"][0]["T"])[:3, 3] * F32(2.0 ** -13))
    pr = pt_scene("cbox@proj:mixed")
    assert np.array_equal(rows(pr["objects"][3]["T"])[3], np.array([0.25, 0, 0, 1], F32)) and np.array_equal(rows(pr["objects"][5]["T"])[3], np.array([0, 0, 0, 2], F32))
    assert np.array_equal(rows(pr["objects"][4]["T"])[3], np.array([0, 0, 0, 1], F32))
    assert scene_digest(base) == before
    assert scene_digest(pt_scene("random303@posef:0.37@move:b")) == scene_digest(pt_scene("random303@posef:0.37@move:b"))
    # rays: origins go with the world, a tenth stays axis-aligned, the tight bounds scale, velocities scale
    from _cases import random_rays, unnormalised_rays
    org, dd, b = SC.scaled_rays("random_rays", 3, 1000, g)
    o0, d0, b0 = random_rays(3, 1000)
    assert np.array_equal(org, o0 * F32(2.0 ** 14)) and np.array_equal(dd, d0) and ((dd[:100] != 0).sum(axis=1) == 1).all()
    assert np.array_equal(b[:, 0], b0[:, 0] * F32(2.0 ** 14)) and np.isfinite(b).all() and (b[:, 1] >= b0[:, 1]).all()
    org, dd, b = SC.scaled_rays("unnormalised_rays", 3, 1000, SC.translated(g, (1, 2, 3)))
    o0, d0, b0 = unnormalised_rays(3, 1000)
    assert np.array_equal(org, (o0.astype(np.float64) * 2.0 ** 14 + [1, 2, 3]).astype(F32)) and np.array_equal(dd, d0 * F32(2.0 ** 14)) and np.array_equal(b, b0)
