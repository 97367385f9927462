"""GPU: the Animate mode's timeline evaluated by kernels (pt_anim.hip) - transforms_device and posed_at_device against what the
reference recorded (tests/golden/anim_*.npz), Timeline.repose_refit / repose against repose_refit / repose of the recorded matrices,
Skin.pose_at / pose_refit_at against Skin.pose / pose_refit of the recorded joint_to_posed, the steady state's upload figures, and the
group forms.  Every comparison is bit for bit on float32 viewed as uint32, NaN matching NaN.  Device arrays are torch tensors passed
by data_ptr()."""
import ctypes

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _instance_cases as IC
import _skin_cases as SC
import _update_cases as UC

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, STATE = -1, -5
W, HT, DEPTH, SPP, SEED = 32, 24, 6, 3, 9


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def objects():
    return AC.load_objects()


@pytest.fixture(scope="module")
def particles(objects):
    """The 74-object particle scene and a timeline's worth of it: the recorded objects a scene can take as they are, on particle
    instances (the first is the particles' source mesh), and the indices into TIMES the scene tests use."""
    S = IC.particles_shared()[0]
    objs = AC.scene_objects(objects)
    assert 12 <= len(objs) <= IC.PARTICLE_COUNT
    idx = np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + len(objs), dtype=np.uint32)
    return {"S": S, "objs": objs, "idx": idx, "tracks": AC.sub_tracks(objects, objs), "times": (4, 9, 11)}   # an interior interval, the last interval, beyond the end


@pytest.fixture(scope="module")
def blob():
    """cbox+blob512, the committed three-joint rig through the blob (skin_blob_chain3.npz) and its recorded keys."""
    S = UC.blob_scene()
    g, joints = SC.load_fixture("blob_chain3")
    return {"S": S, "g": g, "joints": joints, "rig": AC.load_rig("blob_chain3"), "times": (2, 6, 11)}


def make_pt(srt, scene, device=0, use_bvh=True):
    pt = srt.Pathtracer(device)
    pt.set_params(W, HT, 1, DEPTH, use_bvh)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def every_sample():
    ys, xs, ss = np.meshgrid(np.arange(HT), np.arange(W), np.arange(SPP), indexing="ij")
    return xs.reshape(-1).astype(np.uint32), ys.reshape(-1).astype(np.uint32), ss.reshape(-1).astype(np.uint32)


def top_dump(pt, nobj):
    boxes, links, order = pt.dump_bvh(-1, cap=2 * nobj + 2)
    return boxes, links, order[:nobj]


def same_scene(a, b, nobj):
    """Images, every sample's radiance with its draw and ray counts, every dumped tree and the BVH<Object>'s cost."""
    ra, rb = a.trace_samples(SEED, *every_sample()), b.trace_samples(SEED, *every_sample())
    assert AC.bits_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    assert AC.bits_equal(a.render_epoch(SEED, 0, SPP), b.render_epoch(SEED, 0, SPP))
    assert IC.dumps_equal(IC.all_dumps(a, nobj), IC.all_dumps(b, nobj))
    ta, tb = top_dump(a, nobj), top_dump(b, nobj)
    assert AC.bits_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1]) and np.array_equal(ta[2], tb[2])
    assert a.scene_tree_cost() == b.scene_tree_cost()


def set_rig(skin, rig):
    skin.set_rig(*[rig[k] for k in ("parent", "base", "rest_pose", "knot_offsets", "knot_times", "knot_quats")])


def test_hypotf_on_the_device_equals_the_host(srt):
    """srt_hypotf compiled for gfx950 against the same function compiled for the host (which test_pt_anim_host.py pins to libm):
    random bit patterns, the renderer's range, the corners."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, (2, 1 << 19), dtype=np.uint64).astype(np.uint32).view(F)
    near = rng.uniform(-1.5, 1.5, (2, 1 << 19)).astype(F)
    corners = np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 1e-45, 3.4e38, 1.17549435e-38, 2.0 ** -75, 2.0 ** 64], F)
    cx, cy = (a.reshape(-1) for a in np.meshgrid(corners, corners))
    x, y = (np.ascontiguousarray(np.concatenate(p)) for p in ((bits[0], near[0], cx), (bits[1], near[1], cy)))
    pt = srt.Pathtracer(0)
    got = pt.math_hypot(x, y)
    pt.close()
    want = np.zeros(len(x), F)
    AC.anim_emu().anim_emu_hypot(H.P(x), H.P(y), ctypes.c_uint64(len(x)), H.P(want))
    assert AC.mismatches(got, want) == 0


def test_transforms_device_equals_the_reference(srt, torch, objects):
    """All 70 recorded objects - a full wave and a partial one - at every time; the host form on the same context too."""
    S = IC.particles_shared()[0]
    pt = make_pt(srt, S)
    idx = np.array([k for k, o in enumerate(S["objects"]) if not o.get("is_light")][:AC.NOBJECTS], np.uint32)
    tl = pt.create_timeline(idx, (objects["track_offsets"], objects["knot_times"], objects["knot_values"]))
    d = torch.zeros((len(objects["times"]), AC.NOBJECTS + 1, 16), device="cuda:0")      # (one record of room behind each frame: it stays zero)
    for i, t in enumerate(objects["times"]):
        tl.transforms_device(float(t), d[i].data_ptr())
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    bad = {float(t): (AC.mismatches(got[i, :AC.NOBJECTS], objects["trans"][i]), AC.mismatches(tl.transforms(t), objects["trans"][i])) for i, t in enumerate(objects["times"])}
    tl.close()
    pt.close()
    assert not any(a or b for a, b in bad.values()), bad
    assert not got[:, AC.NOBJECTS].any()


@pytest.mark.parametrize("name", AC.RIGS)
def test_posed_at_equals_the_reference(srt, torch, name):
    """joint_to_posed of every joint at every time from the joint kernels and from the host form; and the skinned vertices of
    vertices_at_device against the reference's posed_mesh()."""
    g, joints = SC.load_fixture(name)
    rig = AC.load_rig(name)
    S = SC.single_mesh_scene(g["pos"], g["nrm"], g["idx"])
    pt = srt.Pathtracer(0)
    pt.set_params(8, 8, 1, 4, False)
    pt.build_scene(S)
    skin = pt.create_skin(0, g["pos"], g["nrm"], joints)
    lib = srt.load_library()
    out = np.zeros((len(joints), 16), F)
    assert lib.srt_pt_skin_posed(skin._h, 0.5, H.P(out)) == STATE and lib.srt_pt_skin_pose_at(skin._h, None, 0.5, 0) == STATE      # no rig yet
    before = pt.scene_counts()["uploaded_bytes"]
    set_rig(skin, rig)
    nj, nk, nv = len(joints), len(rig["knot_times"]), len(g["pos"])
    assert pt.scene_counts()["uploaded_bytes"] - before == 4 * nj + 12 + 12 * nj + 4 * (nj + 1) + 20 * nk
    nt = len(rig["times"])
    d = torch.zeros((nt, nj, 16), device="cuda:0")
    dp, dn = torch.zeros((nt, nv, 3), device="cuda:0"), torch.zeros((nt, nv, 3), device="cuda:0")
    for i, t in enumerate(rig["times"]):
        skin.posed_at_device(float(t), d[i].data_ptr())
        skin.vertices_at_device(float(t), dp[i].data_ptr(), dn[i].data_ptr())
    torch.cuda.synchronize()
    got, pos, nrm = d.cpu().numpy(), dp.cpu().numpy(), dn.cpu().numpy()
    bad = {float(t): (AC.mismatches(got[i], rig["posed"][i]), AC.mismatches(skin.posed_at(t), rig["posed"][i]), AC.mismatches(pos[i], rig["mesh_pos"][i]))
           for i, t in enumerate(rig["times"])}
    skin.close()
    pt.close()
    assert not any(any(v) for v in bad.values()), bad
    assert all(AC.bits_equal(n, g["nrm"]) for n in nrm)                                 # smooth normals: skin does not touch them


@pytest.mark.parametrize("how", ["repose_refit", "repose"])
def test_timeline_reposes_like_the_recorded_matrices(srt, objects, particles, how):
    """Timeline.repose_refit(t) / repose(t) and then a render: the scene of repose_refit / repose with the recorded matrices."""
    S, idx, objs = particles["S"], particles["idx"], particles["objs"]
    nobj = len(S["objects"])
    pt, other = make_pt(srt, S), make_pt(srt, S)
    tl = pt.create_timeline(idx, particles["tracks"])
    for i in particles["times"]:
        getattr(tl, how)(float(objects["times"][i]))
        getattr(other, how)(idx, objects["trans"][i][objs])
        same_scene(pt, other, nobj)
    tl.close()
    pt.close(); other.close()


def test_timeline_steady_state_uploads_nothing(srt, objects, particles):
    """A second and a third repose_refit at other times add 0 bytes to the upload counter, and the pending count rises without a
    settle; the scene is then the third time's."""
    S, idx, objs = particles["S"], particles["idx"], particles["objs"]
    T = objects["times"]
    pt, other = make_pt(srt, S), make_pt(srt, S)
    tl = pt.create_timeline(idx, particles["tracks"])
    tl.repose_refit(float(T[2]))                            # the first call makes the tables and sends the list
    c0, count0 = pt.scene_counts()["uploaded_bytes"], pt.top_refit_count()                # (settles)
    assert pt.top_refit_pending() == (0, 0)
    tl.repose_refit(float(T[6]))
    assert pt.top_refit_pending() == (1, len(idx))
    tl.repose_refit(float(T[8]))
    assert pt.top_refit_pending() == (2, len(idx))
    assert pt.scene_counts()["uploaded_bytes"] - c0 == 0 and pt.top_refit_pending() == (0, 0) and pt.top_refit_count() == count0 + 2
    for i in (2, 6, 8):
        other.repose_refit(idx, objects["trans"][i][objs])
    same_scene(pt, other, len(S["objects"]))
    # stale once the scene is committed again
    pt.build_scene(S)
    with pytest.raises(srt.SrtError) as e:
        tl.repose_refit(0.5)
    assert e.value.status == STATE
    tl.close()
    pt.close(); other.close()


def test_refused_set_rig_keeps_the_rig_and_a_stale_skin_is_refused(srt, torch, blob):
    """srt_pt_skin_set_rig on a real skin: every refusal - NULL arguments, a parent out of order, bad offsets, bad times - leaves the
    rig the skin had, so pose_at still gives the scene of the recorded matrices.  Then the scene is committed again: the skin is
    stale and each of the six rig entry points returns SRT_ERR_STATE, with the new commit left as it is."""
    S, g, rig = blob["S"], blob["g"], blob["rig"]
    nobj, nj, nv = len(S["objects"]), len(blob["joints"]), len(g["pos"])
    lib = srt.load_library()
    pt, other = make_pt(srt, S), make_pt(srt, S)
    skin, skin2 = (p.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"]) for p in (pt, other))
    set_rig(skin, rig)
    parent, extent, base, rest, koff, ktimes, kquats = AC.rig_arrays(rig)
    good = {"parent": parent, "base": base, "rest": rest, "koff": koff, "ktimes": ktimes, "kquats": kquats}

    def call(**change):
        a = dict(good, **change)
        return lib.srt_pt_skin_set_rig(skin._h, *[None if a[k] is None else H.P(a[k]) for k in ("parent", "base", "rest", "koff", "ktimes", "kquats")])

    uploaded = pt.scene_counts()["uploaded_bytes"]
    for name in good:
        assert call(**{name: None}) == INVALID, name
    behind, below, down, late, nan, same = parent.copy(), parent.copy(), koff.copy(), koff.copy(), ktimes.copy(), ktimes.copy()
    behind[1], below[2] = 1, -2
    down[1], down[2] = down[2] + 1, down[1]
    late[0] = 1
    keyed = int(np.nonzero(np.diff(koff) >= 2)[0][0])
    nan[koff[keyed] + 1], same[koff[keyed] + 1] = np.nan, same[koff[keyed]]
    for change in ({"parent": behind}, {"parent": below}, {"koff": np.ascontiguousarray(down)}, {"koff": late}, {"ktimes": nan}, {"ktimes": same}):
        assert call(**change) == INVALID, change
    assert pt.scene_counts()["uploaded_bytes"] == uploaded                              # a refused call uploads nothing
    i = blob["times"][1]
    t = float(rig["times"][i])
    assert AC.bits_equal(skin.posed_at(t), rig["posed"][i])
    skin.pose_at(t)
    skin2.pose(rig["posed"][i])
    same_scene(pt, other, nobj)
    skin2.close(); other.close()
    # a second, valid set_rig replaces the rig: no keys at all, every joint at its rest pose
    rest_only = np.zeros(nj + 1, np.uint32)
    assert call(koff=rest_only) == 0
    e_euler, e_posed = AC.emu_rig(parent, extent, base, rest, rest_only, ktimes, kquats, t)
    assert AC.bits_equal(e_euler, rest) and AC.bits_equal(skin.posed_at(t), e_posed)
    # stale: the scene is committed again
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    fresh = make_pt(srt, S)
    d_posed, d_pos, d_nrm = torch.zeros((nj, 16), device="cuda:0"), torch.zeros((nv, 3), device="cuda:0"), torch.zeros((nv, 3), device="cuda:0")
    out = np.zeros((nj, 16), F)
    torch.cuda.synchronize()
    assert call() == STATE and "stale" in lib.srt_last_error().decode()
    assert lib.srt_pt_skin_posed(skin._h, t, H.P(out)) == STATE
    assert lib.srt_pt_skin_posed_device(skin._h, None, t, ctypes.c_void_p(d_posed.data_ptr())) == STATE
    assert lib.srt_pt_skin_vertices_at_device(skin._h, None, t, 0, ctypes.c_void_p(d_pos.data_ptr()), ctypes.c_void_p(d_nrm.data_ptr())) == STATE
    assert lib.srt_pt_skin_pose_at(skin._h, None, t, 0) == STATE and lib.srt_pt_skin_pose_refit_at(skin._h, None, t, 1) == STATE
    torch.cuda.synchronize()
    assert not out.any() and not d_posed.any().item() and not d_pos.any().item() and not d_nrm.any().item()
    same_scene(pt, fresh, nobj)
    skin.close()
    pt.close(); fresh.close()


@pytest.mark.parametrize("how", ["pose", "pose_refit"])
def test_skin_pose_at_equals_pose_of_the_recorded_matrices(srt, blob, how):
    """Skin.pose_at(t) / pose_refit_at(t) leave the scene that Skin.pose / pose_refit of the recorded joint_to_posed leave; flat normals
    on the second time.  A frame sends no joint matrix up: 64 B per joint less than the call that takes `posed`."""
    S, g, rig = blob["S"], blob["g"], blob["rig"]
    nobj, nj = len(S["objects"]), len(blob["joints"])
    pt, other = make_pt(srt, S), make_pt(srt, S)
    skin, skin2 = (p.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"]) for p in (pt, other))
    set_rig(skin, rig)
    deltas = []
    for n, i in enumerate(blob["times"]):
        flat = n == 1
        a0, b0 = pt.scene_counts(), other.scene_counts()
        getattr(skin, how + "_at")(float(rig["times"][i]), flat_normals=flat)
        getattr(skin2, how)(rig["posed"][i], flat_normals=flat)
        a1, b1 = pt.scene_counts(), other.scene_counts()
        deltas.append((b1["uploaded_bytes"] - b0["uploaded_bytes"]) - (a1["uploaded_bytes"] - a0["uploaded_bytes"]))
        assert a1["refits"] - a0["refits"] == b1["refits"] - b0["refits"] == (1 if how == "pose_refit" else 0)
        assert a1["blas_builds"] - a0["blas_builds"] == b1["blas_builds"] - b0["blas_builds"] == (0 if how == "pose_refit" else 1)
        same_scene(pt, other, nobj)
    skin.close(); skin2.close()
    pt.close(); other.close()
    assert deltas == [64 * nj] * len(deltas), deltas


def test_groups(srt, objects, particles, blob):
    """Two ranks on one device: TimelineGroup and SkinGroup give every rank the same t, and the image is the single context's."""
    S, idx, objs = particles["S"], particles["idx"], particles["objs"]
    i = particles["times"][0]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    tl = grp.create_timeline(idx, particles["tracks"])
    assert len(tl.timelines) == 2 and AC.bits_equal(tl.transforms(float(objects["times"][i])), objects["trans"][i][objs])
    tl.repose_refit(float(objects["times"][i]))
    refit = grp.render_epoch(SEED, 0, SPP)
    tl.repose(float(objects["times"][i]))
    rebuilt = grp.render_epoch(SEED, 0, SPP)
    tl.close(); grp.close()
    single = make_pt(srt, S)
    single.repose_refit(idx, objects["trans"][i][objs])
    want_refit = single.render_epoch(SEED, 0, SPP)
    single.repose(idx, objects["trans"][i][objs])
    want_rebuilt = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert AC.bits_equal(refit, want_refit) and AC.bits_equal(rebuilt, want_rebuilt)
    # skins
    B, g, rig = blob["S"], blob["g"], blob["rig"]
    k = blob["times"][1]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(B)
    grp.set_camera(B["camera"])
    skins = grp.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"])
    set_rig(skins, rig)
    assert AC.bits_equal(skins.posed_at(float(rig["times"][k])), rig["posed"][k])
    skins.pose_at(float(rig["times"][k]))
    posed = grp.render_epoch(SEED, 0, SPP)
    skins.pose_refit_at(float(rig["times"][blob["times"][2]]), flat_normals=True)
    refitted = grp.render_epoch(SEED, 0, SPP)
    counts = grp.scene_counts()
    skins.close(); grp.close()
    single = make_pt(srt, B)
    skin = single.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"])
    skin.pose(rig["posed"][k])
    want_posed = single.render_epoch(SEED, 0, SPP)
    skin.pose_refit(rig["posed"][blob["times"][2]], flat_normals=True)
    want_refitted = single.render_epoch(SEED, 0, SPP)
    skin.close(); single.close()
    assert AC.bits_equal(posed, want_posed) and AC.bits_equal(refitted, want_refitted) and counts[0] == counts[1]
