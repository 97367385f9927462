"""GPU: Skeleton::do_ik / step_ik by one kernel launch (pt_ik.hip) - Skin.step_ik and step_ik_device against the poses the reference
recorded after every call (tests/golden/ik_*.npz), set_time on the current pose, posed_current and vertices_current_device against
the recorded joint_to_posed and posed_mesh(), the frame step_ik_device -> pose_current -> render_epoch_device on one stream against a
fresh commit of the recorded vertices, the `_at` calls left as they were, the group form and every refusal.  Beyond the recorded
sizes - the LDS form with every wave busy, 256 / 257 joints, lanes with many joints, up to 1024 handles with hundreds on one joint,
keyed rigs of more than one block - the generated rigs of _ik_cases.py against the host definitions (srt_pt_rig_step_ik_host,
srt_pt_rig_posed_host), which the recordings pin to the reference.  Every comparison is bit for bit on float32 viewed as uint32, NaN
matching NaN.  Device arrays are torch tensors passed by data_ptr()."""
import ctypes

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _ik_cases as IK
import _instance_cases as IC
import _skin_cases as SC
import _update_cases as UC

pytestmark = pytest.mark.gpu

F = np.float32
INVALID, UNSUPPORTED, STATE = -1, -4, -5
W, HT, DEPTH, SPP, SEED = 32, 24, 6, 2, 9


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def blob(srt):
    """cbox+blob512, the committed three-joint rig through the blob, its IK record, and the epoch image of a fresh commit of the
    reference's recorded vertices.  Computed once, left unchanged."""
    S = UC.blob_scene()
    g, joints = SC.load_fixture("blob_chain3")
    ik = IK.load("blob_chain3")
    fresh = make_pt(srt, IC.scenes_module().with_vertices(S, UC.BLOB_OBJECT, ik["mesh_pos"], g["nrm"]))
    want = fresh.render_epoch(SEED, 0, SPP)
    fresh.close()
    return {"S": S, "g": g, "joints": joints, "ik": ik, "want": want}


def make_pt(srt, scene, device=0):
    pt = srt.Pathtracer(device)
    pt.set_params(W, HT, 1, DEPTH, True)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


@pytest.fixture(scope="module")
def lib(srt):
    return srt.load_library()


def rigged_skin(srt, case):
    """(context, skin, case) of a rig on a one-mesh scene - a recorded rig by name, or a case dict with a fixture's inputs
    (IK.generated, IK.generated_keyed): the committed skin fixture's mesh and joints where there is one, the small blob and joints made
    from the rig otherwise."""
    name = case if isinstance(case, str) else None
    ik = IK.load(name) if name else case
    if name in IK.MESHED:
        g, joints = SC.load_fixture(name)
        pos, nrm, idx = g["pos"], g["nrm"], g["idx"]
    else:
        pos, nrm, idx = SC.small_blob_mesh()
        joints = IK.skin_joints(ik)
    pt = srt.Pathtracer(0)
    pt.set_params(8, 8, 1, 4, True)
    pt.build_scene(SC.single_mesh_scene(pos, nrm, idx))
    skin = pt.create_skin(0, pos, nrm, joints)
    skin.set_rig(*IK.rig_arrays(ik))
    if name or "handle_joints" in ik:                         # (a keyed rig of IK.generated_keyed has no handles)
        skin.set_ik_handles(ik["handle_joints"])
    return pt, skin, ik


def device_inputs(torch, ik):
    """The record's targets and enabled bytes per call as tensors, on the device before anything is enqueued."""
    inputs = [(torch.from_numpy(np.ascontiguousarray(ik["targets"][c], F)).to("cuda:0"), torch.from_numpy(np.ascontiguousarray(ik["enabled"][c], np.uint8)).to("cuda:0"))
              for c in range(len(ik["targets"]))]
    torch.cuda.synchronize()
    return inputs


def replay(skin, ik, inputs=None, stream=0):
    """The fixture's calls, one per step of the generator: the host form, or with device_inputs() the device form on `stream`."""
    for c in range(len(ik["targets"])):
        if not np.isnan(ik["set_times"][c]):
            skin.set_time(float(ik["set_times"][c]), stream=stream)
        if inputs is None:
            skin.step_ik(ik["targets"][c], ik["enabled"][c])
        else:
            skin.step_ik_device(inputs[c][0].data_ptr(), inputs[c][1].data_ptr(), stream=stream)
        yield c


@pytest.mark.parametrize("name", IK.RIGS)
def test_step_ik_equals_the_reference(srt, torch, name):
    """Skin.step_ik K times - Skin.set_time first where the record has a time: joint_pose() after every call, then posed_current from
    the host and from the joint kernels and, for the two meshed rigs, the skinned vertices.  deep262 has more joints than the
    workgroup has lanes and than LDS holds: the strided loops, the barriers across waves and the device scratch."""
    pt, skin, ik = rigged_skin(srt, name)
    nj, nv = skin.njoints, skin.nverts
    assert AC.bits_equal(skin.joint_pose(), ik["rest_pose"])
    bad = [AC.mismatches(skin.joint_pose(), ik["pose"][c]) for c in replay(skin, ik)]
    d_posed, d_pos, d_nrm = torch.zeros((nj + 1, 16), device="cuda:0"), torch.zeros((nv, 3), device="cuda:0"), torch.zeros((nv, 3), device="cuda:0")
    skin.posed_current_device(d_posed.data_ptr())
    skin.vertices_current_device(d_pos.data_ptr(), d_nrm.data_ptr())
    torch.cuda.synchronize()
    posed = (AC.mismatches(skin.posed_current(), ik["posed"]), AC.mismatches(d_posed.cpu().numpy()[:nj], ik["posed"]))
    verts = AC.mismatches(d_pos.cpu().numpy(), ik["mesh_pos"]) if name in IK.MESHED else 0
    room = d_posed[nj].any().item()
    skin.close(); pt.close()
    assert not any(bad) and posed == (0, 0) and verts == 0 and not room, (bad, posed, verts)


@pytest.mark.parametrize("name", IK.RIGS)
def test_step_ik_device_equals_the_reference(srt, torch, name):
    """Targets and enabled bytes in torch tensors: after every call, and with all K calls enqueued back to back on a stream of their
    own; then a call with no handle enabled on poses of -0, NaN and an angle beyond the sin / cos restatement: every bit stays."""
    pt, skin, ik = rigged_skin(srt, name)
    uploaded = pt.scene_counts()["uploaded_bytes"]
    inputs = device_inputs(torch, ik)
    bad = [AC.mismatches(skin.joint_pose(), ik["pose"][c]) for c in replay(skin, ik, inputs)]
    assert pt.scene_counts()["uploaded_bytes"] == uploaded                            # the device form sends nothing up
    skin.set_joint_pose(ik["rest_pose"])
    assert AC.bits_equal(skin.joint_pose(), ik["rest_pose"])
    st = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for _ in replay(skin, ik, inputs, stream=st.cuda_stream):
        pass
    back_to_back = AC.mismatches(skin.joint_pose(), ik["pose"][-1])
    odd = np.array(ik["rest_pose"], F)
    odd[0] = [-0.0, np.nan, 1e9]
    skin.set_joint_pose(odd)
    d_t = torch.from_numpy(np.ascontiguousarray(ik["targets"][0], F)).to("cuda:0")
    d_e = torch.zeros(len(ik["handle_joints"]), dtype=torch.uint8, device="cuda:0")
    skin.step_ik_device(d_t.data_ptr(), d_e.data_ptr())
    kept_bits = np.array_equal(skin.joint_pose().view(np.uint32), odd.view(np.uint32))
    # enabled = NULL: every handle, as a tensor of ones
    skin.set_joint_pose(ik["rest_pose"])
    skin.step_ik_device(d_t.data_ptr())
    every = skin.joint_pose()
    skin.set_joint_pose(ik["rest_pose"])
    skin.step_ik(ik["targets"][0], np.full(len(d_e), 7, np.uint8))
    same = AC.bits_equal(every, skin.joint_pose())
    skin.close(); pt.close()
    assert not any(bad) and back_to_back == 0 and kept_bits and same, (bad, back_to_back, kept_bits, same)


@pytest.mark.parametrize("name", IK.GENERATED)
def test_generated_rigs_equal_the_host_definition(srt, torch, lib, name):
    """The generated rigs (IK.GENERATED_SIZES: around one wave, around the LDS form's last size, a lane with three joints and with
    sixteen, 1024 handles, a root under every handle) against srt_pt_rig_step_ik_host: joint_pose() after each of the three calls
    through Skin.step_ik, after each through step_ik_device, and after the three enqueued back to back on a stream of their own;
    then posed_current from the host and from the joint kernels against srt_pt_rig_posed_host of the last pose.  Mismatching words
    per comparison; every one is zero."""
    g = IK.generated(name)
    want = IK.generated_poses(lib, name)
    want_posed = IK.posed_host(lib, g, 0.0, rest=want[-1])[1]
    pt, skin, _ = rigged_skin(srt, g)
    nj = skin.njoints
    assert AC.bits_equal(skin.joint_pose(), g["rest_pose"])
    host_form = [AC.mismatches(skin.joint_pose(), want[c]) for c in replay(skin, g)]
    skin.set_joint_pose(g["rest_pose"])
    inputs = device_inputs(torch, g)
    uploaded = pt.scene_counts()["uploaded_bytes"]
    device_form = [AC.mismatches(skin.joint_pose(), want[c]) for c in replay(skin, g, inputs)]
    sent = pt.scene_counts()["uploaded_bytes"] - uploaded                              # the device form sends nothing up
    skin.set_joint_pose(g["rest_pose"])
    st = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    for _ in replay(skin, g, inputs, stream=st.cuda_stream):
        pass
    back_to_back = AC.mismatches(skin.joint_pose(), want[-1])
    d_posed = torch.zeros((nj + 1, 16), device="cuda:0")
    skin.posed_current_device(d_posed.data_ptr())
    torch.cuda.synchronize()
    posed = (AC.mismatches(skin.posed_current(), want_posed), AC.mismatches(d_posed.cpu().numpy()[:nj], want_posed))
    room = d_posed[nj].any().item()
    skin.close(); pt.close()
    print(name, "mismatching words:", host_form, device_form, back_to_back, posed)
    assert host_form == [0, 0, 0] and device_form == [0, 0, 0] and sent == 0 and back_to_back == 0 and posed == (0, 0) and not room, \
        (host_form, device_form, sent, back_to_back, posed, room)


@pytest.mark.parametrize("name", ["gen256_1024", "gen1000_1024"])
def test_every_handle_of_1024(srt, torch, lib, name):
    """enabled = NULL with the handle tables full, in the LDS form and on scratch: the host form with a byte of one per handle."""
    g = IK.generated(name)
    nh = len(g["handle_joints"])
    assert nh == IK.MAX_HANDLES
    st, want = IK.step_host(lib, g["parent"], g["extent"], g["rest_pose"], g["handle_joints"], g["targets"][1], np.ones(nh, np.uint8))
    assert st == 0 and not AC.bits_equal(want, IK.generated_poses(lib, name)[0])
    pt, skin, _ = rigged_skin(srt, g)
    skin.step_ik(g["targets"][1])
    host_form = AC.mismatches(skin.joint_pose(), want)
    skin.set_joint_pose(g["rest_pose"])
    d_t = torch.from_numpy(np.ascontiguousarray(g["targets"][1], F)).to("cuda:0")
    torch.cuda.synchronize()
    skin.step_ik_device(d_t.data_ptr())
    device_form = AC.mismatches(skin.joint_pose(), want)
    skin.close(); pt.close()
    assert (host_form, device_form) == (0, 0)


@pytest.mark.parametrize("nj", IK.KEYED_SIZES)
def test_keyed_rigs_at_size(srt, torch, lib, nj):
    """Skeleton::set_time and the rig's matrices at a time, beyond one block of either kernel: half the joints keyed with every knot
    count, at every time of the timeline tests.  set_time(t) gives the keyed joints srt_pt_rig_posed_host's Euler angles and leaves
    the others the bits they had (a pose that is not the rest pose); posed_at(t) and posed_at_device(t) are its matrices."""
    g = IK.generated_keyed(nj)
    keyed = np.diff(g["knot_offsets"].astype(np.int64)) > 0
    pt, skin, _ = rigged_skin(srt, g)
    skin.set_joint_pose(g["had"])
    d_posed = torch.zeros((nj + 1, 16), device="cuda:0")
    bad = []
    for t in AC.TIMES:
        euler, posed = IK.posed_host(lib, g, t)
        skin.set_time(float(t))
        pose = skin.joint_pose()
        skin.posed_at_device(float(t), d_posed.data_ptr())
        torch.cuda.synchronize()
        bad.append((AC.mismatches(pose[keyed], euler[keyed]), int(np.sum(pose[~keyed].view(np.uint32) != g["had"][~keyed].view(np.uint32))),
                    AC.mismatches(skin.posed_at(float(t)), posed), AC.mismatches(d_posed.cpu().numpy()[:nj], posed)))
    room = d_posed[nj].any().item()
    skin.close(); pt.close()
    assert bad == [(0, 0, 0, 0)] * len(AC.TIMES) and not room, bad


@pytest.mark.parametrize("how", ["inplace", "update", "refit"])
def test_frame_on_one_stream(srt, torch, blob, how):
    """set_time / step_ik_device (the record's K calls) -> pose_current(how) -> render_epoch_device -> untile_device on one stream with
    no synchronisation in between: the epoch image is that of a fresh commit of the reference's posed_mesh() vertices."""
    S, g, ik = blob["S"], blob["g"], blob["ik"]
    pt = make_pt(srt, S)
    skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"])
    skin.set_rig(*IK.rig_arrays(ik))
    skin.set_ik_handles(ik["handle_joints"])
    local_tiles, _, floats_per_tile = pt.tile_info()
    tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
    inputs = device_inputs(torch, ik)
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    for _ in replay(skin, ik, inputs, stream=s):
        pass
    skin.pose_current(how, stream=s)
    pt.render_epoch_device(s, SEED, 0, SPP, tiles.data_ptr())
    pt.untile_device(s, tiles.data_ptr(), image.data_ptr())
    st.synchronize()
    if how == "inplace":
        assert pt.mesh_refit_pending() == (1, 1)                                      # nothing has settled: the host's record was not needed
    got = image.cpu().numpy().reshape(HT, W, 3)
    again = pt.render_epoch(SEED, 0, SPP)
    pose = skin.joint_pose()
    skin.close(); pt.close()
    assert AC.bits_equal(got, blob["want"]) and AC.bits_equal(again, blob["want"]) and AC.bits_equal(pose, ik["pose"][-1])


def test_at_calls_do_not_see_the_current_pose(srt, torch):
    """posed_at and vertices_at_device give the same bits before and after IK has changed the current pose, and pose_at leaves the
    current pose alone."""
    pt, skin, ik = rigged_skin(srt, "blob_chain3")
    nv, t = skin.nverts, 1.7
    d = [torch.zeros((nv, 3), device="cuda:0") for _ in range(4)]
    posed0 = skin.posed_at(t)
    skin.vertices_at_device(t, d[0].data_ptr(), d[1].data_ptr())
    for _ in replay(skin, ik):
        pass
    moved = skin.joint_pose()
    skin.vertices_at_device(t, d[2].data_ptr(), d[3].data_ptr())
    skin.pose_at(t)
    skin.pose_refit_at(0.5)
    torch.cuda.synchronize()
    same = AC.bits_equal(posed0, skin.posed_at(t)) and AC.bits_equal(d[0].cpu().numpy(), d[2].cpu().numpy()) and AC.bits_equal(d[1].cpu().numpy(), d[3].cpu().numpy())
    kept = AC.bits_equal(skin.joint_pose(), moved) and AC.bits_equal(moved, ik["pose"][-1]) and AC.bits_equal(skin.posed_current(), ik["posed"])
    skin.close(); pt.close()
    assert same and kept and not AC.bits_equal(posed0, ik["posed"])


def test_group(srt, blob):
    """Two ranks on one device: SkinGroup forwards every call to each skin; the poses are the record's on both and the image is the
    fresh commit's."""
    S, g, ik = blob["S"], blob["g"], blob["ik"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    skins = grp.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"])
    skins.set_rig(*IK.rig_arrays(ik))
    skins.set_ik_handles(ik["handle_joints"])
    skins.set_joint_pose(ik["rest_pose"])
    for c in range(len(ik["targets"])):
        if not np.isnan(ik["set_times"][c]):
            skins.set_time(float(ik["set_times"][c]))
        skins.step_ik(ik["targets"][c], ik["enabled"][c])
    poses = [k.joint_pose() for k in skins.skins]
    posed = skins.posed_current()
    skins.pose_current("inplace")
    inplace = grp.render_epoch(SEED, 0, SPP)
    skins.pose_current("refit", flat_normals=False)
    refit = grp.render_epoch(SEED, 0, SPP)
    skins.close(); grp.close()
    assert len(poses) == 2 and all(AC.bits_equal(p, ik["pose"][-1]) for p in poses) and AC.bits_equal(posed, ik["posed"])
    assert AC.bits_equal(inplace, blob["want"]) and AC.bits_equal(refit, blob["want"])


def test_refusals(srt, torch, blob):
    """No rig, no handles, a joint out of range, too many handles, NULL arguments, another `how`, and a stale skin: each refused with its
    status, with the handles, the pose and the scene left as they were."""
    S, g, ik = blob["S"], blob["g"], blob["ik"]
    lib = srt.load_library()
    nj, nh, nv = len(blob["joints"]), len(ik["handle_joints"]), len(g["pos"])
    pt = make_pt(srt, S)
    skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], blob["joints"])
    h = skin._h
    z = ctypes.c_void_p(0)
    hj, tg = np.ascontiguousarray(ik["handle_joints"], np.uint32), np.ascontiguousarray(ik["targets"][0], F)
    out, posed = np.zeros((nj, 3), F), np.zeros((nj, 16), F)
    d_t, d_p, d_n = torch.from_numpy(tg).to("cuda:0"), torch.zeros((nv, 3), device="cuda:0"), torch.zeros((nv, 3), device="cuda:0")
    d_posed = torch.zeros((nj, 16), device="cuda:0")
    dp = lambda t: ctypes.c_void_p(t.data_ptr())                                      # noqa: E731

    def every_call():
        return (lib.srt_pt_skin_set_ik_handles(h, H.P(hj), nh), lib.srt_pt_skin_set_joint_pose(h, H.P(out)), lib.srt_pt_skin_joint_pose(h, H.P(out)),
                lib.srt_pt_skin_set_time(h, z, ctypes.c_float(0.5)), lib.srt_pt_skin_step_ik(h, H.P(tg), None), lib.srt_pt_skin_step_ik_device(h, z, dp(d_t), None),
                lib.srt_pt_skin_posed_current(h, H.P(posed)), lib.srt_pt_skin_posed_current_device(h, z, dp(d_posed)),
                lib.srt_pt_skin_vertices_current_device(h, z, 0, dp(d_p), dp(d_n)), lib.srt_pt_skin_pose_current(h, z, 0, 2))

    assert every_call() == (STATE,) * 10 and "no rig" in lib.srt_last_error().decode()   # no rig yet
    skin.set_rig(*IK.rig_arrays(ik))
    assert lib.srt_pt_skin_step_ik(h, H.P(tg), None) == STATE and "handles" in lib.srt_last_error().decode()   # a rig, no handles
    assert lib.srt_pt_skin_step_ik_device(h, z, dp(d_t), None) == STATE
    skin.set_ik_handles(hj)
    # refused handle lists: the skin keeps what it had
    assert lib.srt_pt_skin_set_ik_handles(h, None, nh) == INVALID
    for wrong in (nj, 2 ** 32 - 1):
        assert lib.srt_pt_skin_set_ik_handles(h, H.P(np.array([0, wrong], np.uint32)), 2) == INVALID
    many = np.zeros(IK.MAX_HANDLES + 1, np.uint32)
    assert lib.srt_pt_skin_set_ik_handles(h, H.P(many), len(many)) == UNSUPPORTED and "1024" in lib.srt_last_error().decode()
    assert lib.srt_pt_skin_step_ik(h, None, None) == INVALID and lib.srt_pt_skin_step_ik_device(h, z, None, None) == INVALID
    assert lib.srt_pt_skin_set_joint_pose(h, None) == INVALID and lib.srt_pt_skin_joint_pose(h, None) == INVALID
    assert lib.srt_pt_skin_posed_current(h, None) == INVALID and lib.srt_pt_skin_posed_current_device(h, z, None) == INVALID
    assert lib.srt_pt_skin_vertices_current_device(h, z, 0, None, dp(d_n)) == INVALID
    assert lib.srt_pt_skin_pose_current(h, z, 0, 3) == INVALID and lib.srt_pt_skin_pose_current(h, z, 0, -1) == INVALID
    assert AC.bits_equal(skin.joint_pose(), ik["rest_pose"])
    bad = [AC.mismatches(skin.joint_pose(), ik["pose"][c]) for c in replay(skin, ik)]   # the handles and the pose were left alone
    assert not any(bad), bad
    # the limit itself is accepted, and an empty list clears
    skin.set_ik_handles(np.arange(IK.MAX_HANDLES) % nj)
    skin.set_ik_handles([])
    assert lib.srt_pt_skin_step_ik(h, H.P(tg), None) == STATE
    # a new set_rig starts from its rest pose and has no handles
    skin.set_ik_handles(hj)
    skin.set_rig(*IK.rig_arrays(ik))
    assert AC.bits_equal(skin.joint_pose(), ik["rest_pose"]) and lib.srt_pt_skin_step_ik(h, H.P(tg), None) == STATE
    # stale: the scene is committed again
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    fresh = make_pt(srt, S)
    torch.cuda.synchronize()
    d_p.zero_(); d_n.zero_(); d_posed.zero_()
    out[:], posed[:] = 0, 0
    assert every_call() == (STATE,) * 10 and "stale" in lib.srt_last_error().decode()
    torch.cuda.synchronize()
    assert not out.any() and not posed.any() and not d_p.any().item() and not d_n.any().item() and not d_posed.any().item()
    assert AC.bits_equal(pt.render_epoch(SEED, 0, SPP), fresh.render_epoch(SEED, 0, SPP))
    skin.close()
    pt.close(); fresh.close()
