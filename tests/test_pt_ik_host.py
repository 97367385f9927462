"""CPU: Skeleton::do_ik / step_ik as the product restates it (csrc/pt_ik.h) against what the reference recorded
(tests/golden/ik_*.npz, made by tests/golden/make_ik_golden.py): srt_pt_rig_step_ik_host after every recorded call, joint_to_posed
after the last one, the first iteration's intermediate values from the host emulation, the cases that leave the poses' bits alone,
the summation order, every refusal a host can reach, and a sanitized stand-alone program over the handle check, the CSR and the
solve; then the generated rigs the GPU tests run (IK.generated, IK.generated_keyed): the conditions that make them worth running,
and the host definitions against the host emulations on them.  Every comparison is on float32 viewed as uint32, NaN matching NaN; there are no tolerances."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _ik_cases as IK

F = np.float32
INVALID, UNSUPPORTED, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def lib(srt):
    return srt.load_library()


def posed_host(lib, g, pose, base=None):
    """Skeleton::joint_to_posed of every joint under `pose`: srt_pt_rig_posed_host with `pose` as the rest pose and no keys."""
    n = len(g["parent"])
    parent, extent = np.ascontiguousarray(g["parent"], np.int32), np.ascontiguousarray(g["extent"], F)
    base = np.ascontiguousarray(g["base"] if base is None else base, F)
    rest, koff = np.ascontiguousarray(pose, F), np.zeros(n + 1, np.uint32)
    posed = np.zeros((n, 16), F)
    assert lib.srt_pt_rig_posed_host(n, H.P(parent), H.P(extent), H.P(base), H.P(rest), H.P(koff), H.P(np.zeros(1, F)), H.P(np.zeros(4, F)), ctypes.c_float(0.0),
                                     None, H.P(posed)) == 0
    return posed


def mat_point(m, p):
    """Mat4 * Vec3 (lib/mat4.h:149-156) in float32, one rounding per operator: ((x col0 + y col1) + z col2) + 1 col3, then three divisions by w."""
    x, y, z = (F(v) for v in p)
    r = [F(F(F(F(x * m[a]) + F(y * m[4 + a])) + F(z * m[8 + a])) + F(F(1.0) * m[12 + a])) for a in range(4)]
    return np.array([r[0] / r[3], r[1] / r[3], r[2] / r[3]], F)


def test_abi_and_bindings(srt, lib):
    names = ("srt_pt_skin_set_ik_handles", "srt_pt_skin_set_joint_pose", "srt_pt_skin_joint_pose", "srt_pt_skin_set_time", "srt_pt_skin_step_ik",
             "srt_pt_skin_step_ik_device", "srt_pt_skin_posed_current", "srt_pt_skin_posed_current_device", "srt_pt_skin_vertices_current_device",
             "srt_pt_skin_pose_current")
    text = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for name in names:
        assert getattr(lib, name) is not None and name + "(" in text, name
    assert "6875 degrees" in text and "1024 handles" in text
    assert lib.srt_pt_rig_step_ik_host is not None and "srt_pt_rig_step_ik_host(" in open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()
    methods = ("set_ik_handles", "set_joint_pose", "joint_pose", "set_time", "step_ik", "step_ik_device", "posed_current", "pose_current")
    for cls in (srt.Skin, srt.SkinGroup):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(srt.Skin.vertices_current_device) and srt.Skin.HOW == {"update": 0, "refit": 1, "inplace": 2}


@pytest.mark.parametrize("name", IK.RIGS)
def test_fixture_holds_the_cases(name):
    """What make_ik_golden.py asserted when it recorded, checked again on the committed file."""
    g = IK.load(name)
    K, nj = g["pose"].shape[:2]
    chains = IK.chains(g["parent"], g["handle_joints"])
    assert all(p < k for k, p in enumerate(g["parent"]))
    assert np.isfinite(g["pose"]).all() and np.isfinite(g["pose_before"]).all() and np.abs(g["pose"]).max() < 1000 and np.abs(g["pose_before"]).max() < 1000
    reached = np.zeros(nj, bool)
    for c in range(K):
        assert bool(g["did"][c]) == bool(g["enabled"][c].any())
        for h, chain in enumerate(chains):
            if g["enabled"][c][h]:
                reached[chain] = True
    moved = np.abs(g["pose"] - g["pose_before"]).max(axis=2).sum(axis=0)
    assert reached.any() and np.all(moved[reached] > IK.LEAST_MOVED.get(name, 1.0)) and np.all(moved[~reached] == 0)
    assert IK.LEAST_MOVED.get(name, 1.0) >= (0.05 if name == "wide200" else 1.0)
    if name == "wide200":
        IK.check_wide(g)
    if name in IK.MESHED:
        import _skin_cases as SC

        skin = SC.load_fixture(name)[0]
        assert np.array_equal(g["order"], skin["order"]) and AC.bits_equal(g["extent"], skin["extent"]) and g["mesh_pos"].shape == skin["pos"].shape
    if name == "blob_chain3":
        keyed = np.diff(g["knot_offsets"]) > 0
        assert 0 < keyed.sum() < nj and np.isfinite(g["set_times"]).any() and np.isnan(g["set_times"]).any()
        assert list(g["handle_joints"]) == [nj - 1] and len(chains[0]) == 3
        rig = AC.load_rig(name)                                  # the keys are those of the timeline tests' rig
        assert AC.bits_equal(g["knot_times"], rig["knot_times"]) and AC.bits_equal(g["knot_quats"], rig["knot_quats"]) and AC.bits_equal(g["rest_pose"], rig["rest_pose"])
    if name == "blob128_tree5":
        hj, par = list(g["handle_joints"]), g["parent"]
        sets = [set(c) for c in chains]
        assert (par < 0).sum() == 2 and len(hj) != len(set(hj)) and any(par[j] < 0 for j in hj)
        assert any(sets[a] & sets[b] and hj[a] not in sets[b] and hj[b] not in sets[a] for a in range(len(hj)) for b in range(a))
        assert any(not e.any() for e in g["enabled"]) and any(e.any() and not e.all() for e in g["enabled"])
    if name == "deep262":
        assert nj > IK.BLOCK and nj > IK.LDS_JOINTS and max(len(c) for c in chains) >= 20 and len(chains) >= 3


@pytest.mark.parametrize("name", IK.RIGS)
def test_step_ik_host_equals_the_reference(lib, name):
    """Every joint's pose after every one of the K recorded calls - Skeleton::set_time first where the fixture has a time - and
    joint_to_posed after the last."""
    g = IK.load(name)
    got = IK.replay_host(lib, g)
    bad = [AC.mismatches(got[c], g["pose"][c]) for c in range(len(got))]
    assert not any(bad), bad
    assert AC.bits_equal(posed_host(lib, g, got[-1]), g["posed"])
    # several calls in one: the recorded calls that share targets and flags with no set_time between them do not exist, so the
    # `calls` argument is held to its own single calls
    c = len(got) - 1
    _, twice = IK.step_host(lib, g["parent"], g["extent"], g["pose_before"][c], g["handle_joints"], g["targets"][c], g["enabled"][c], calls=2)
    _, again = IK.step_host(lib, g["parent"], g["extent"], g["pose"][c], g["handle_joints"], g["targets"][c], g["enabled"][c])
    assert AC.bits_equal(twice, again)


@pytest.mark.parametrize("name", IK.RIGS)
def test_intermediate_values(lib, name):
    """The host emulation of pt_ik.h (g++ -ffp-contract=off): origin and axes of every joint an enabled handle reaches and `current`
    of every enabled handle's joint, in the first iteration of the first call - against Mat4 * Vec3 in float32 on the matrices of
    srt_pt_rig_posed_host with a zero base (Joint::joint_to_posed: skeleton space), which the reference's records pin - and the
    pose after the whole call."""
    g = IK.load(name)
    c = int(np.nonzero(g["did"])[0][0])
    e = IK.emu_one_call(g, c)
    assert AC.bits_equal(e["pose"], g["pose"][c])
    J = posed_host(lib, g, g["pose_before"][c], base=[0, 0, 0])
    chains = IK.chains(g["parent"], g["handle_joints"])
    reached = sorted({j for h, ch in enumerate(chains) if g["enabled"][c][h] for j in ch})
    tips = sorted({int(g["handle_joints"][h]) for h in range(len(chains)) if g["enabled"][c][h]})
    assert list(np.nonzero(e["active"])[0]) == reached and list(np.nonzero(e["active"] & 2)[0]) == tips
    bad = 0
    with np.errstate(all="ignore"):
        for j in reached:
            bad += AC.mismatches(e["origin"][j], mat_point(J[j], (0, 0, 0)))
            for a in range(3):
                bad += AC.mismatches(e["axes"][j][a], mat_point(J[j], np.eye(3)[a]))
        for j in tips:
            bad += AC.mismatches(e["current"][j], mat_point(J[j], g["extent"][j]))
    assert bad == 0
    others = np.setdiff1d(np.arange(len(g["parent"])), reached)
    assert not e["origin"][others].any() and not e["axes"][others].any()           # nothing is computed for a joint no handle reaches


def test_csr_lists_ascend_and_hold_the_chains():
    g = IK.load("deep262")
    n, hj = len(g["parent"]), np.ascontiguousarray(g["handle_joints"], np.uint32)
    parent = np.ascontiguousarray(g["parent"], np.int32)
    off, lst = np.zeros(n + 1, np.uint32), np.zeros(n * len(hj), np.uint32)
    emu = IK.ik_emu()
    emu.ik_emu_csr.restype = ctypes.c_uint32
    total = emu.ik_emu_csr(H.P(parent), n, H.P(hj), len(hj), H.P(off), H.P(lst), len(lst))
    chains = IK.chains(parent, hj)
    assert total == sum(len(c) for c in chains) == off[-1] and off[0] == 0
    for j in range(n):
        assert list(lst[off[j]:off[j + 1]]) == [h for h, c in enumerate(chains) if j in c]


@pytest.mark.parametrize("name", IK.RIGS)
def test_disabled_and_no_handles_keep_the_bits(lib, name):
    """do_ik returns before step_ik when no handle is enabled: not one bit of a pose changes - negative zeros, NaNs and angles beyond
    the sin / cos restatement included, since nothing is computed."""
    g = IK.load(name)
    pose = np.array(g["rest_pose"], F)
    pose[0] = [-0.0, np.nan, 1e9]
    nh = len(g["handle_joints"])
    st, out = IK.step_host(lib, g["parent"], g["extent"], pose, g["handle_joints"], g["targets"][0], np.zeros(nh, np.uint8), calls=3)
    assert st == 0 and np.array_equal(out.view(np.uint32), pose.view(np.uint32))
    st, out = IK.step_host(lib, g["parent"], g["extent"], pose, [], np.zeros((0, 3), F), None, calls=2)
    assert st == 0 and np.array_equal(out.view(np.uint32), pose.view(np.uint32))
    # enabled = NULL is every handle enabled
    ones = np.ones(nh, np.uint8)
    a = IK.step_host(lib, g["parent"], g["extent"], g["rest_pose"], g["handle_joints"], g["targets"][0], None)[1]
    b = IK.step_host(lib, g["parent"], g["extent"], g["rest_pose"], g["handle_joints"], g["targets"][0], ones)[1]
    assert AC.bits_equal(a, b) and not AC.bits_equal(a, g["rest_pose"])
    # any nonzero byte enables
    b = IK.step_host(lib, g["parent"], g["extent"], g["rest_pose"], g["handle_joints"], g["targets"][0], ones * 255)[1]
    assert AC.bits_equal(a, b)


def test_reversed_handle_order_differs(lib):
    """A joint's gradient is summed in handle order and floats do not associate: the tree rig, and wide200 with 64 handles under
    one root, with the handle list reversed - the same handles, targets and flags - end on other bits, so the fixtures can tell a
    wrong summation order."""
    for name in ("blob128_tree5", "wide200"):
        g = IK.load(name)
        c = 0
        fwd = IK.step_host(lib, g["parent"], g["extent"], g["pose_before"][c], g["handle_joints"], g["targets"][c], g["enabled"][c])[1]
        rev = IK.step_host(lib, g["parent"], g["extent"], g["pose_before"][c], g["handle_joints"][::-1], g["targets"][c][::-1], g["enabled"][c][::-1])[1]
        assert AC.bits_equal(fwd, g["pose"][c]) and not AC.bits_equal(rev, g["pose"][c]), name
        assert np.abs(rev - g["pose"][c]).max() < 1e-2, name                          # (the same solve but for the rounding)


@pytest.mark.parametrize("name", IK.GENERATED)
def test_generated_rigs_hold_their_conditions(lib, name):
    """What test_pt_ik_gpu.py relies on in a generated rig, asserted on the data and on srt_pt_rig_step_ik_host's poses: the shape of
    the hierarchy and of the handle list, finite poses below 1000 degrees, every reached joint moved, every other bit kept, another
    result for the reversed handle list.  Conditions on the seed: one that misses takes another seed (IK._SEEDS), not another bound."""
    g = IK.generated(name)
    nj, nh = IK.GENERATED_SIZES[IK.GENERATED.index(name)]
    par, hj, en = g["parent"], g["handle_joints"], g["enabled"]
    chains = IK.chains(par, hj)
    assert len(par) == nj <= IK.MAX_JOINTS and len(hj) == nh <= IK.MAX_HANDLES and g["targets"].shape == (3, nh, 3) and en.shape == (3, nh)
    assert all(p < k for k, p in enumerate(par)) and (par < 0).sum() >= 2 and max(len(c) for c in chains) <= IK.MAX_DEPTH + 1 and g["depth"].max() <= IK.MAX_DEPTH
    length = np.linalg.norm(g["extent"].astype(np.float64), axis=1)
    assert length.min() > 0.199 and length.max() < 0.501 and np.abs(g["rest_pose"]).max() <= 30 and np.abs(g["targets"]).max() <= 2
    # handles with repeats, one on a root, one root above all of them; the three masks
    assert len(set(hj.tolist())) < nh and par[hj[0]] < 0 and len(chains[0]) == 1 and {c[-1] for c in chains} == {int(hj[0])}
    assert en[0].all() and en[1].sum() == nh // 2 and not en[2, 64:128].any() and en[2, :64].all() and en[2, 128:].all()
    # a CSR list as long as the handle list (the root's): 64 handles and more wherever the rig has that many
    held = np.bincount(np.concatenate(chains), minlength=nj)
    assert held.max() == nh and (nh < 64 or held.max() >= 64) and np.bincount(hj).max() >= max(2, nh // 8)
    # a handle's chain with joints of two 64-lane groups of the workgroup: its matrices and `current` cross waves
    if nj > 64:
        assert max(len(IK.waves(c)) for c in chains) >= 2
    if nj > IK.BLOCK:
        assert any(len({j % IK.BLOCK for j in c}) < len(c) for c in chains)           # and a chain with two joints of one lane
    poses = np.concatenate([g["rest_pose"][None], IK.generated_poses(lib, name)])
    assert np.isfinite(poses).all() and np.abs(poses).max() < 1000
    reached = np.zeros(nj, bool)
    for c in range(3):
        for h in np.nonzero(en[c])[0]:
            reached[chains[h]] = True
    moved = np.abs(np.diff(poses, axis=0)).max(axis=2).sum(axis=0)
    assert reached.any() and not reached.all() and moved[reached].min() > 0.01, moved[reached].min()
    assert np.array_equal(poses[-1][~reached].view(np.uint32), g["rest_pose"][~reached].view(np.uint32))
    for c in range(3):                                       # call by call: a joint no enabled handle of this call reaches keeps its bits
        off = np.ones(nj, bool)
        for h in np.nonzero(en[c])[0]:
            off[chains[h]] = False
        assert np.array_equal(poses[c + 1][off].view(np.uint32), poses[c][off].view(np.uint32))
    rev = IK.step_host(lib, par, g["extent"], g["rest_pose"], hj[::-1], g["targets"][0][::-1], en[0][::-1])[1]
    assert not AC.bits_equal(rev, poses[1]) and np.abs(rev - poses[1]).max() < 1e-2


@pytest.mark.parametrize("name", IK.GENERATED)
def test_generated_rigs_equal_the_emulation(lib, name):
    """srt_pt_rig_step_ik_host against the independent g++ build of the same header, one call on each generated rig."""
    g = IK.generated(name)
    e = IK.emu_one_call(g, 0, pose=g["rest_pose"])
    assert AC.mismatches(e["pose"], IK.generated_poses(lib, name)[0]) == 0


@pytest.mark.parametrize("nj", IK.KEYED_SIZES)
def test_keyed_rigs_equal_the_emulation(lib, nj):
    """srt_pt_rig_posed_host on the keyed rigs of test_pt_ik_gpu.py against the host emulation of pt_anim.h, at every time; half the
    joints keyed, every knot count present, a keyed joint in the last block of 64."""
    g = IK.generated_keyed(nj)
    counts = np.diff(g["knot_offsets"].astype(np.int64))
    assert (counts > 0).sum() == nj // 2 and set(counts.tolist()) == set(AC.KNOTS) and (counts[64 * ((nj - 1) // 64):] > 0).any()
    assert not AC.bits_equal(g["had"], g["rest_pose"])
    rig = (np.ascontiguousarray(g["parent"], np.int32), g["extent"], g["base"], g["rest_pose"], g["knot_offsets"], g["knot_times"], g["knot_quats"])
    for t in AC.TIMES:
        euler, posed = IK.posed_host(lib, g, t)
        e_euler, e_posed = AC.emu_rig(*rig, t)
        assert AC.mismatches(euler, e_euler) == 0 and AC.mismatches(posed, e_posed) == 0, float(t)
        assert np.isfinite(posed).all()


def test_refusals_leave_the_pose_alone(lib):
    g = IK.load("blob128_tree5")
    parent, extent = np.ascontiguousarray(g["parent"], np.int32), np.ascontiguousarray(g["extent"], F)
    hj, tg = np.ascontiguousarray(g["handle_joints"], np.uint32), np.ascontiguousarray(g["targets"][0], F)
    n, nh = len(parent), len(hj)
    pose0 = np.array(g["rest_pose"], F)

    def call(njoints=n, parent=parent, extent=extent, hj=hj, tg=tg, nh=nh, pose=True):
        p = pose0.copy()
        st = lib.srt_pt_rig_step_ik_host(njoints, None if parent is None else H.P(parent), None if extent is None else H.P(extent), H.P(p) if pose else None,
                                         None if hj is None else H.P(hj), None if tg is None else H.P(tg), None, nh, 1)
        assert np.array_equal(p.view(np.uint32), pose0.view(np.uint32))
        return st

    assert call(parent=None) == INVALID and call(extent=None) == INVALID and call(pose=False) == INVALID and call(hj=None) == INVALID and call(tg=None) == INVALID
    behind, below = parent.copy(), parent.copy()
    behind[1], below[2] = 1, -2
    assert call(parent=behind) == INVALID and call(parent=below) == INVALID
    for wrong in (n, n + 7, 2 ** 32 - 1):
        bad = hj.copy()
        bad[-1] = wrong
        assert call(hj=bad) == INVALID and "joint" in lib.srt_last_error().decode()
    many = np.zeros(IK.MAX_HANDLES + 1, np.uint32)
    assert call(hj=many, tg=np.zeros((len(many), 3), F), nh=len(many)) == UNSUPPORTED
    assert call(njoints=IK.MAX_JOINTS + 1) == UNSUPPORTED
    # the limit itself is served
    most = (np.arange(IK.MAX_HANDLES) % n).astype(np.uint32)
    st, out = IK.step_host(lib, parent, extent, pose0, most, np.tile(F([2, 1, -1]), (len(most), 1)), None)
    assert st == 0 and np.isfinite(out).all() and not AC.bits_equal(out, pose0)
    # a NULL skin is refused by every entry point of the interface
    z = ctypes.c_void_p(0)
    buf = np.zeros(64, F)
    assert lib.srt_pt_skin_set_ik_handles(None, H.P(hj), nh) == INVALID and lib.srt_pt_skin_set_joint_pose(None, H.P(buf)) == INVALID
    assert lib.srt_pt_skin_joint_pose(None, H.P(buf)) == INVALID and lib.srt_pt_skin_set_time(None, z, ctypes.c_float(0.5)) == INVALID
    assert lib.srt_pt_skin_step_ik(None, H.P(tg), None) == INVALID and lib.srt_pt_skin_step_ik_device(None, z, H.P(tg), None) == INVALID
    assert lib.srt_pt_skin_posed_current(None, H.P(buf)) == INVALID and lib.srt_pt_skin_posed_current_device(None, z, H.P(buf)) == INVALID
    assert lib.srt_pt_skin_vertices_current_device(None, z, 0, H.P(buf), H.P(buf)) == INVALID and lib.srt_pt_skin_pose_current(None, z, 0, 2) == INVALID


def _flat_file(path):
    with open(path, "wb") as f:
        f.write(np.array([len(IK.RIGS)], np.uint32).tobytes())
        for name in IK.RIGS:
            g = IK.load(name)
            K, nj = g["pose"].shape[:2]
            f.write(np.array([nj, len(g["handle_joints"]), K], np.uint32).tobytes())
            for a, t in ((g["parent"], np.int32), (g["extent"], F), (g["handle_joints"], np.uint32), (g["targets"], F), (g["enabled"], np.uint8),
                         (g["pose_before"], F), (g["pose"], F)):
                f.write(np.ascontiguousarray(a, t).tobytes())


def test_sanitized_program(tmp_path):
    """-fsanitize=address,undefined over the handle-table check, the CSR construction and the host solve: the fixtures, no handles, a
    handle on every joint, the maximum handle count, one past it, joints out of range.  A program of its own, run as its own process."""
    exe = IK.sanitized_program()
    path = str(tmp_path / "ik.bin")
    _flat_file(path)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ik_sanitized: ok" in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
