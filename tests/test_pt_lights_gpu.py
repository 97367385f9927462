"""GPU: srt_pt_set_dynamic_lights - area lights re-posed (srt_pt_repose, srt_pt_repose_device) and deformed (srt_pt_update_mesh,
srt_pt_refit_mesh, their device forms, skins) without a commit.  After every step the context must compute, bit for bit, what
the oracle computes on the fresh description (IC.with_poses / scenes.with_vertices: the oracle knows nothing of the switch), under
every kernel form, and its light tables read back from the device must equal its host mirror and a freshly committed context's."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _light_cases as LC
import _skin_cases as SC
import _update_cases as UC
from test_pt_update_gpu import DEPTH, HT, SEED, SPP, W, bits_equal, check_against, every_sample, make_pt, reference

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
MODES = (0, 2, 5, 6, 7)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def committed_T(S, index):
    return np.ascontiguousarray(S["objects"][index]["T"], np.float32).reshape(16)


def make_lit(srt, scene, when="before", **kw):
    """A context with the switch set before the commit or after it."""
    if when == "before":
        pt = srt.Pathtracer(0)
        pt.set_params(kw.get("w", W), kw.get("h", HT), 1, kw.get("depth", DEPTH), kw.get("use_bvh", True))
        pt.set_dynamic_lights(True)
        if kw.get("builder") is not None:
            pt.set_bvh_builder(*kw["builder"])
        pt.build_scene(scene)
        pt.set_camera(scene["camera"])
        return pt
    pt = make_pt(srt, scene, **kw)
    pt.set_dynamic_lights(True)
    return pt


def check_lights(srt, pt, desc, use_bvh=True):
    """dump_lights(True) against the context's own mirror and against a context freshly committed on `desc`."""
    dev = pt.dump_lights(True)
    assert LC.lights_equal(dev, pt.dump_lights(False))
    fresh = make_pt(srt, desc, use_bvh=use_bvh)
    want = fresh.dump_lights(True)
    fresh.close()
    assert LC.lights_equal(dev, want)
    return dev


def tensor_of(keep, a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    torch.cuda.synchronize()
    keep.append(t)
    return t


# ---- 6: the Cornell box's light re-posed ----
@pytest.fixture(scope="module")
def cornell():
    """sweeps_scene() (the Cornell box, a 512-triangle blob and an instance of it), the quad's poses, and the oracle's results on
    each description: the light alone, and the light together with the mirror sphere and the instance.  Computed once."""
    S = IC.sweeps_scene()
    P = LC.poses(committed_T(S, LC.CBOX_LIGHT))
    inst = len(S["objects"]) - 1
    others = {5: IC.translate(committed_T(S, 5), (0.05, 0.1, -0.05)), inst: IC.translate(committed_T(S, inst), (0.3, -0.2, 0.2))}
    lists = {}
    for name in ("translation", "rotation * scale"):
        lists[("alone", name)] = ([LC.CBOX_LIGHT], [P[name]])
        lists[("list", name)] = ([5, LC.CBOX_LIGHT, inst], [others[5], P[name], others[inst]])
    descs = {k: IC.with_poses(S, *v) for k, v in lists.items()}
    return {"S": S, "P": P, "lists": lists, "descs": descs, "first": reference(S), "refs": {k: reference(d) for k, d in descs.items()}}


@pytest.mark.parametrize("when", ["before", "after"])
@pytest.mark.parametrize("how", ["repose", "repose_device", "list"])
def test_cornell_light_reposed(srt, cornell, how, when):
    """The quad through the translation and the rotation * scale; the identity puts it on the floor with the floor's centre - a
    description no commit terminates on - and is refused with everything left as it was; then back to the committed pose."""
    S = cornell["S"]
    pt = make_lit(srt, S, when)
    keep = []
    first = pt.render_epoch(SEED, 0, SPP)
    assert bits_equal(first, cornell["first"]["epoch"])
    lights0 = pt.dump_lights(True)

    def repose(indices, Ts):
        if how == "repose_device":
            pt.repose_device(indices, tensor_of(keep, np.asarray(Ts, np.float32).reshape(-1, 16)).data_ptr())
        else:
            pt.repose(indices, Ts)

    changed = 0
    for name in ("translation", "rotation * scale"):
        key = ("list" if how == "list" else "alone", name)
        repose(*cornell["lists"][key])
        check_against(pt, cornell["refs"][key], MODES)
        dev = check_lights(srt, pt, cornell["descs"][key])
        assert not LC.lights_equal(dev, lights0)
        changed += not bits_equal(cornell["refs"][key]["epoch"], first)
    assert changed >= 1
    kept_image, kept_lights = pt.render_epoch(SEED, 0, SPP), pt.dump_lights(True)
    with pytest.raises(srt.SrtError, match="does not terminate") as e:
        repose([LC.CBOX_LIGHT], [cornell["P"]["identity"]])
    assert e.value.status == UNSUPPORTED
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), kept_image) and LC.lights_equal(pt.dump_lights(True), kept_lights)
    indices = cornell["lists"][("list" if how == "list" else "alone", "translation")][0]
    repose(indices, [committed_T(S, i) for i in indices])
    back, lights = pt.render_epoch(SEED, 0, SPP), pt.dump_lights(True)
    pt.close()
    assert bits_equal(back, first) and LC.lights_equal(lights, lights0)


@pytest.mark.parametrize("how", ["repose", "repose_device"])
def test_cornell_light_reposed_in_a_list_scene(srt, how):
    """Committed without BVHs the quad takes all three poses, the identity (has_trans 1 -> 0) included, and comes back (0 -> 1)."""
    S = IC.scenes_module().cornell_box("cbox")
    pt = make_lit(srt, S, "after", use_bvh=False)
    keep = []
    first = pt.render_epoch(SEED, 0, SPP)
    seen = []
    for name, T in LC.poses(committed_T(S, LC.CBOX_LIGHT)).items():
        if how == "repose_device":
            pt.repose_device([LC.CBOX_LIGHT], tensor_of(keep, T).data_ptr())
        else:
            pt.repose([LC.CBOX_LIGHT], [T])
        desc = IC.with_poses(S, [LC.CBOX_LIGHT], [T])
        o = H.OraclePT(desc, W, HT, DEPTH, False)
        rgb, draws, rays = pt.trace_samples(SEED, *every_sample(W, HT, SPP))
        want = o.trace_samples(SEED, *every_sample(W, HT, SPP))
        assert np.array_equal(draws, want[1]) and np.array_equal(rays, want[2]) and bits_equal(rgb, want[0]), name
        assert bits_equal(pt.render_epoch(SEED, 0, SPP), o.epoch(SEED, 0, SPP)), name
        seen.append(int(check_lights(srt, pt, desc, use_bvh=False)["heads"][0, 0]))
    assert seen == [1, 1, 0]
    pt.repose([LC.CBOX_LIGHT], [committed_T(S, LC.CBOX_LIGHT)])
    back = pt.render_epoch(SEED, 0, SPP)
    pt.close()
    assert bits_equal(back, first)


# ---- 7: two mesh lights and a sphere light ----
def test_only_the_listed_lights_change(srt):
    """Lights 0 (the Cornell quad), 1 (an emissive sphere) and 2 (a second quad): the sphere alone goes into the identity
    (has_trans 1 -> 0, on the device, in a scene with BVHs), then the second quad alone moves; the rows of the others stay."""
    S = LC.three_light_scene()
    pt = make_lit(srt, S)
    keep = []
    d0 = pt.dump_lights(True)
    assert d0["heads"][:, 3].tolist() == [7, 9, 10] and d0["heads"][:, 0].tolist() == [1, 1, 1]
    I = np.eye(4, dtype=np.float32).reshape(16)
    pt.repose_device([9], tensor_of(keep, I).data_ptr())
    S1 = IC.with_poses(S, [9], [I])
    check_against(pt, reference(S1), MODES)
    d1 = check_lights(srt, pt, S1)
    assert d1["heads"][:, 0].tolist() == [1, 0, 1]
    assert LC.rows_equal(LC.light_rows(d1, 0), LC.light_rows(d0, 0)) and LC.rows_equal(LC.light_rows(d1, 2), LC.light_rows(d0, 2))
    assert not LC.rows_equal(LC.light_rows(d1, 1), LC.light_rows(d0, 1))
    T = LC.poses(committed_T(S, 10))["rotation * scale"]
    pt.repose([10], [T])
    S2 = IC.with_poses(S1, [10], [T])
    check_against(pt, reference(S2), MODES)
    d2 = check_lights(srt, pt, S2)
    pt.close()
    assert LC.rows_equal(LC.light_rows(d2, 0), LC.light_rows(d0, 0)) and LC.rows_equal(LC.light_rows(d2, 1), LC.light_rows(d1, 1))
    assert not LC.rows_equal(LC.light_rows(d2, 2), LC.light_rows(d1, 2))


# ---- 8: a deforming light ----
@pytest.fixture(scope="module")
def blob(scenes):
    """The Cornell box with an emissive 125-triangle blob, its deformations, and the oracle's results on each description."""
    S = LC.blob_light_scene()
    D = LC.blob_light_deformations()
    descs = {name: scenes.with_vertices(S, LC.BLOB_LIGHT, p, n) for name, (p, n) in D.items()}
    return {"S": S, "D": D, "descs": descs, "first": reference(S), "refs": {name: reference(d) for name, d in descs.items()}}


@pytest.mark.parametrize("how", ["update_host_builder", "update_device_builder", "update_device_arrays", "refit", "refit_device"])
def test_deforming_light(srt, blob, how):
    S = blob["S"]
    builder = (True, 64) if how in ("update_device_builder", "update_device_arrays") else (False,)
    pt = make_lit(srt, S, "after" if how == "refit" else "before", builder=builder)
    keep = []
    first = pt.render_epoch(SEED, 0, SPP)
    assert bits_equal(first, blob["first"]["epoch"])
    refit = how.startswith("refit")

    def deform(p, n):
        if how in ("update_device_arrays", "refit_device"):
            tp, tn = tensor_of(keep, p), tensor_of(keep, n)
            (pt.refit_mesh_device if refit else pt.update_mesh_device)(LC.BLOB_LIGHT, tp.data_ptr(), tn.data_ptr(), len(p))
        else:
            (pt.refit_mesh if refit else pt.update_mesh)(LC.BLOB_LIGHT, p, n)

    for name, (p, n) in blob["D"].items():
        before = pt.scene_counts()
        deform(p, n)
        after = pt.scene_counts()
        assert after["triangles"] == before["triangles"] and after["blas_builds"] == before["blas_builds"] + (0 if refit else 1), name
        if how in ("update_device_arrays", "refit_device"):
            assert after["uploaded_bytes"] - before["uploaded_bytes"] < after["device_bytes"], name
        # (a refitted tree is another tree than the oracle builds: the hit records of single rays are left to the refit tests)
        check_against(pt, blob["refs"][name], MODES, hit_modes=() if refit else (0, 5))
        check_lights(srt, pt, blob["descs"][name])
    deform(*UC.original(S, LC.BLOB_LIGHT))
    back = pt.render_epoch(SEED, 0, SPP)
    check_lights(srt, pt, S)
    pt.close()
    assert bits_equal(back, first)


def light_blob_rig():
    """A three-joint chain through the emissive blob (object space) and two sets of angles."""
    base, extents = [0.0, -0.13, 0.01], [[0, 0.09, 0]] * 3
    joints = SC.chain(base, extents, [0.15, 0.16, 0.15])
    return joints, [SC.chain_posed(base, extents, a) for a in ([[0, 0, 10], [8, 0, -15], [0, 12, 20]], [[4, 25, -6], [-10, 0, 12], [15, -8, 0]])]


@pytest.mark.parametrize("how", ["pose", "pose_refit"])
def test_skinned_light(srt, scenes, blob, how):
    """A skin on the emissive blob: each pose against the oracle on scenes.with_vertices of the skin's own vertices; a skin on a
    light fails with update_mesh's refusal once the switch is cleared."""
    S = blob["S"]
    pos, nrm = UC.original(S, LC.BLOB_LIGHT)
    joints, posed = light_blob_rig()
    pt = make_lit(srt, S, "after")
    with pytest.raises(srt.SrtError, match="is an area light"):
        off = make_pt(srt, S)
        try:
            off.create_skin(LC.BLOB_LIGHT, pos, nrm, joints)
        finally:
            off.close()
    skin = pt.create_skin(LC.BLOB_LIGHT, pos, nrm, joints)
    assert np.diff(skin.map()[0].astype(np.int64)).max() >= 1
    for k, m in enumerate(posed):
        flat = k == 1
        p, n = skin.vertices(m, flat_normals=flat)
        assert not np.isnan(p).any() and not np.isnan(n).any() and not bits_equal(p, pos)
        (skin.pose if how == "pose" else skin.pose_refit)(m, flat_normals=flat)
        desc = scenes.with_vertices(S, LC.BLOB_LIGHT, p, n)
        check_against(pt, reference(desc), MODES, hit_modes=(0, 5) if how == "pose" else ())
        check_lights(srt, pt, desc)
    kept = pt.dump_lights(True)
    pt.set_dynamic_lights(False)
    with pytest.raises(srt.SrtError, match="is an area light: its light-list copy") as e:
        (skin.pose if how == "pose" else skin.pose_refit)(posed[0])
    assert e.value.status == INVALID and LC.lights_equal(pt.dump_lights(True), kept)
    skin.close(); pt.close()


# ---- 9: refusals ----
def test_refusals_on_the_device(srt):
    lib = srt.load_library()
    S = LC.three_light_scene()
    S["objects"].append(LC.blob_light_scene()["objects"][LC.BLOB_LIGHT])       # object 11: the emissive blob
    blob_i, sphere, nobj = 11, 9, 12
    pt = make_lit(srt, S, builder=(False,))
    keep = []
    image, lights, counts = pt.render_epoch(SEED, 0, SPP), pt.dump_lights(True), pt.scene_counts()
    T = LC.poses(committed_T(S, LC.CBOX_LIGHT))["translation"]
    p, n = UC.original(S, blob_i)
    lp, ln = UC.original(S, LC.CBOX_LIGHT)
    bad = p.copy()
    bad[17, 1] = np.inf
    one = UC.one_point(S, blob_i)
    T3 = tensor_of(keep, np.stack([T, T, T]))
    tbad, tn = tensor_of(keep, bad), tensor_of(keep, n)
    u32 = lambda *v: np.array(v, np.uint32)
    cases = [("a duplicate", lambda: lib.srt_pt_repose(pt._ctx, H.P(u32(7, 5, 7)), H.P(np.stack([T, T, T])), 3), INVALID),
             ("a duplicate, device", lambda: lib.srt_pt_repose_device(pt._ctx, None, H.P(u32(7, 5, 7)), T3.data_ptr(), 3), INVALID),
             ("out of range", lambda: lib.srt_pt_repose(pt._ctx, H.P(u32(7, nobj)), H.P(np.stack([T, T])), 2), INVALID),
             ("out of range, device", lambda: lib.srt_pt_repose_device(pt._ctx, None, H.P(u32(7, nobj)), T3.data_ptr(), 2), INVALID),
             ("update of the sphere light", lambda: lib.srt_pt_update_mesh(pt._ctx, sphere, H.P(lp), H.P(ln), len(lp)), INVALID),
             ("refit of the sphere light", lambda: lib.srt_pt_refit_mesh(pt._ctx, sphere, H.P(lp), H.P(ln), len(lp)), INVALID),
             ("a non-finite refit position", lambda: lib.srt_pt_refit_mesh(pt._ctx, blob_i, H.P(bad), H.P(n), len(p)), INVALID),
             ("a non-finite refit position, device", lambda: lib.srt_pt_refit_mesh_device(pt._ctx, None, blob_i, tbad.data_ptr(), tn.data_ptr(), len(p)), INVALID),
             ("one point", lambda: lib.srt_pt_update_mesh(pt._ctx, blob_i, H.P(one[0]), H.P(one[1]), len(p)), UNSUPPORTED)]
    for what, call, status in cases:
        assert call() == status, what
        assert bits_equal(pt.render_epoch(SEED, 0, SPP), image) and LC.lights_equal(pt.dump_lights(True), lights), what
    assert pt.scene_counts()["blas_builds"] == counts["blas_builds"]
    # the switch cleared: the light is refused with the message it always had
    pt.set_dynamic_lights(False)
    with pytest.raises(srt.SrtError, match="is an area light: its light tables depend on its pose, commit the scene again"):
        pt.repose([LC.CBOX_LIGHT], [T])
    with pytest.raises(srt.SrtError, match="is an area light: its light-list copy and light tables depend on its vertices, commit the scene again"):
        pt.update_mesh(blob_i, p, n)
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), image) and LC.lights_equal(pt.dump_lights(True), lights)
    pt.close()
    # the deep chain on a light
    from test_pt_lights_host import emissive_chain_scene

    S2, (cp, cn) = emissive_chain_scene()
    pt = make_lit(srt, S2, builder=(False,))
    image, lights = pt.render_epoch(SEED, 0, SPP), pt.dump_lights(True)
    assert lib.srt_pt_update_mesh(pt._ctx, 6, H.P(cp), H.P(cn), len(cp)) == UNSUPPORTED
    again, after = pt.render_epoch(SEED, 0, SPP), pt.dump_lights(True)
    pt.close()
    assert bits_equal(again, image) and LC.lights_equal(after, lights)


# ---- 10: a group ----
def test_group(srt, blob):
    S = blob["S"]
    p, n = blob["D"]["D2"]
    T = LC.poses(committed_T(S, LC.CBOX_LIGHT))["rotation * scale"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    with pytest.raises(srt.SrtError, match="is an area light"):
        grp.repose([LC.CBOX_LIGHT], [T])
    grp.set_dynamic_lights(True)
    first = grp.render_epoch(SEED, 0, SPP)
    grp.repose([LC.CBOX_LIGHT], [T])
    grp.update_mesh(LC.BLOB_LIGHT, p, n)
    moved = grp.render_epoch(SEED, 0, SPP)
    same = LC.lights_equal(grp.members[0].dump_lights(True), grp.members[1].dump_lights(True))
    grp.close()
    single = make_lit(srt, S)
    single.repose([LC.CBOX_LIGHT], [T])
    single.update_mesh(LC.BLOB_LIGHT, p, n)
    want = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert bits_equal(first, blob["first"]["epoch"]) and bits_equal(moved, want) and not bits_equal(moved, first) and same
