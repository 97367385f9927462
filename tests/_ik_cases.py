"""Rigs, handles and targets of the IK tests (test_pt_ik_host.py, test_pt_ik_gpu.py, tests/golden/make_ik_golden.py).

cases() is what make_ik_golden.py runs through the reference (its own Skeleton::set_time, do_ik / step_ik and joint_to_posed) and
records as tests/golden/ik_<name>.npz - in the caller's joint and handle order here, in Skeleton::for_joints order and in the order
do_ik visited the handles there; the tests read everything back from the fixtures, so that what is solved is what was recorded.
generated() and generated_keyed() are seeded rigs at the sizes no recording has - they never go through the reference; the tests
hold the kernels to the host definitions on them.  Everything here is data.  Lengths are a few units: at the blob's 0.1-unit scale the targets are, because tau = 0.02 on a gradient
of |bone| * |current - target| barely moves a joint otherwise."""
import ctypes
import os

import numpy as np

import _anim_cases as AC
import _harness as H

F = np.float32
NAN = float("nan")
RIGS = ("blob_chain3", "blob128_tree5", "deep262", "wide200")
MESHED = ("blob_chain3", "blob128_tree5")
# degrees a joint that an enabled handle reaches has to move over a fixture's calls: the hand-made rigs pull a few joints hard;
# wide200 has the generated rigs' magnitudes, where 64 handles share the pull on 200 joints
LEAST_MOVED = {"wide200": 0.05}
BLOCK = 256             # kIkBlock: the lanes of the kernel's workgroup
LDS_JOINTS = 256        # kIkLdsJoints: beyond, the per-joint values live in device scratch
MAX_HANDLES = 1024      # kIkMaxHandles
MAX_JOINTS = 4096       # kSkinMaxJoints


def _deep_rig():
    """262 joints - more than the workgroup has lanes and more than LDS holds: a chain 24 deep from the first root, a second root, the
    rest hung at random under what is there.  Extents of 0.4 .. 0.9 units, rest poses within +-30 degrees."""
    rng = np.random.default_rng(262)
    n = 262
    parent = [-1] + list(range(0, 23)) + [-1]
    while len(parent) < n:
        parent.append(int(rng.integers(0, len(parent))))
    d = rng.normal(size=(n, 3))
    extent = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.4, 0.9, (n, 1))).astype(F)
    rest = rng.uniform(-30, 30, (n, 3)).astype(F)
    depth = [0] * n
    for j in range(n):
        depth[j] = 0 if parent[j] < 0 else depth[parent[j]] + 1
    leaf = int(np.argmax(depth[25:])) + 25                  # the deepest joint of the random part
    return {"parent": parent, "extent": extent, "radius": [0.25] * n, "base": [0.3, -0.2, 0.1], "rest": rest, "keys": {},
            "handles": [23, leaf, 24, 100, 23],               # the deep tip twice, a random leaf, the second root (a chain of one), one inside
            "set_times": [NAN, NAN, NAN],
            "targets": [[[3, 5, -2], [-4, 2, 3], [1, -3, 2], [2, 2, 4], [-2, 6, 1]], [[4, 3, 1], [-3, 4, 2], [2, -2, -3], [1, 4, 3], [0, 5, -3]],
                        [[2, 6, 2], [-5, 1, 1], [3, 1, -2], [3, 3, 2], [-1, 4, 4]]],
            "enabled": [[1, 1, 1, 1, 1], [1, 1, 1, 1, 0], [1, 1, 1, 1, 1]]}


def _wide_rig():
    """200 joints at most 16 deep - the LDS form with joints in all four waves - under 64 handles with repeats, root 0 above all of
    them; a third of the joints keyed; a set_time before the first and the third call.  The magnitudes of the generated rigs."""
    rng = np.random.default_rng(200)
    n, nh = 200, 64
    g = _rig(rng, n, cap=16)
    keys = {}
    for k, j in enumerate(np.sort(rng.permutation(n)[:n // 3])):
        count = (1, 2, 3, 6)[k % 4]
        keys[int(j)] = (AC.KNOTS[count], [AC.quat_of_euler(rng.uniform(-30, 30, 3)) for _ in range(count)])
    enabled = np.ones((3, nh), np.uint8)
    enabled[1] = rng.permutation(nh) < nh // 2
    return {"parent": [int(p) for p in g["parent"]], "extent": g["extent"], "radius": [0.25] * n, "base": [0.3, -0.2, 0.1], "rest": g["rest_pose"], "keys": keys,
            "handles": [int(j) for j in _handles(rng, g["parent"], g["depth"], nh)], "set_times": [0.9, NAN, 2.75],
            "targets": rng.uniform(-2, 2, (3, nh, 3)).astype(F), "enabled": enabled}


def cases():
    import _skin_cases as SC

    rigs = SC.rigs()
    c3, t5 = rigs["blob_chain3"], rigs["blob128_tree5"]
    rest3, keys3 = AC.rig_keys("blob_chain3", 3)
    return {
        # one handle on the tip; joints 0 and 2 keyed (the keys of anim_rig_blob_chain3): set_time, then IK, then IK alone, ...
        "blob_chain3": {"mesh": c3["mesh"], "parent": c3["parent"], "extent": np.array(c3["extent"], F), "radius": c3["radius"], "base": c3["base"],
                        "rest": rest3, "keys": keys3, "handles": [2], "set_times": [0.9, NAN, 2.75, NAN],
                        "targets": [[[8, 6, -5]], [[-7, 9, 4]], [[6, -8, 7]], [[9, 5, 6]]], "enabled": [[1], [1], [1], [1]]},
        # two roots (0 and 4); handles on the sibling branches 1 and 2 -> 3 under joint 0; two handles on joint 3; one on the root 4 (a
        # chain of one); the last handle never enabled; the second call with every handle disabled
        "blob128_tree5": {"mesh": t5["mesh"], "parent": t5["parent"], "extent": np.array(t5["extent"], F), "radius": t5["radius"], "base": t5["base"],
                          "rest": np.array(t5["poses"][0], F), "keys": {}, "handles": [1, 3, 3, 4, 2], "set_times": [NAN] * 4,
                          "targets": [[[3, 2, -1], [-2, 3, 2], [1, 4, -3], [2, -3, 1], [0, 2, 2]], [[1, 1, 1]] * 5,
                                      [[-3, 1, 2], [2, 2, -3], [-1, 3, 3], [-2, -2, -2], [3, 0, 1]], [[2, 4, 1], [-3, 2, 1], [2, 3, -2], [1, -4, 2], [1, 1, 3]]],
                          "enabled": [[1, 1, 1, 1, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 0], [1, 0, 1, 1, 0]]},
        "deep262": _deep_rig(),
        "wide200": _wide_rig(),
    }


def load(name):
    return np.load(os.path.join(H.GOLDEN, f"ik_{name}.npz"))


# ---- generated rigs: no recording, the host definition (srt_pt_rig_step_ik_host, srt_pt_rig_posed_host) is what they are held to ----
# (joints, handles): 64 / 65 one wave and the first joint of the next; 255 / 256 the last sizes in LDS, 256 filling it exactly, with
# 1024 handles the handle tables too; 257 the first on scratch and d_pose; 513 the first at which a lane owns three joints; 4096 the
# size of the flag table.
GENERATED_SIZES = ((64, 8), (65, 8), (255, 255), (256, 256), (256, 1024), (257, 257), (513, 300), (1000, 1024), (4096, 1024), (4096, 64))
GENERATED = tuple(f"gen{nj}_{nh}" for nj, nh in GENERATED_SIZES)
KEYED_SIZES = (63, 64, 65, 257, 4096)       # ik_set_time_kernel's blocks are 64 lanes, the joint kernels' 256
MAX_DEPTH = 48
_SEEDS = {}                                 # name -> another seed, where the default misses a condition of test_pt_ik_host.py
_generated = {}


def _hierarchy(rng, n, cap):
    """parent[n], parents first: three roots (joint 0 and two further on), every other joint hung under one of the three before it
    half of the time and anywhere before it otherwise, never deeper than `cap`."""
    roots = {0, n // 3, (2 * n) // 3}
    parent, depth = [], []
    for j in range(n):
        if j in roots:
            p = -1
        else:
            p = j - int(rng.integers(1, min(j, 3) + 1)) if rng.random() < 0.5 else int(rng.integers(0, j))
            if depth[p] >= cap:
                p = int(rng.choice([q for q in range(j) if depth[q] < cap]))
        parent.append(p)
        depth.append(0 if p < 0 else depth[p] + 1)
    return np.array(parent, np.int32), np.array(depth)


def _rig(rng, n, cap=MAX_DEPTH):
    parent, depth = _hierarchy(rng, n, cap)
    d = rng.normal(size=(n, 3))
    extent = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 0.5, (n, 1))).astype(F)
    return {"parent": parent, "depth": depth, "extent": extent, "radius": np.full(n, 0.25, F), "base": np.array([0.3, -0.2, 0.1], F),
            "rest_pose": rng.uniform(-30, 30, (n, 3)).astype(F)}


def _no_keys(n):
    return {"knot_offsets": np.zeros(n + 1, np.uint32), "knot_times": np.zeros(0, F), "knot_quats": np.zeros((0, 4), F)}


def _handles(rng, parent, depth, nh):
    """nh handle joints under root 0, drawn with repetition: the first on the root itself (a chain of one), then the deepest joint
    under it and the last one under it, then an eighth of the list (two at least) on one joint, the rest anywhere under it."""
    n = len(parent)
    top = np.zeros(n, np.int64)
    for j in range(n):
        top[j] = j if parent[j] < 0 else top[parent[j]]
    under = np.nonzero(top == 0)[0]
    hj = rng.choice(under, nh)
    hj[:3] = [0, under[np.argmax(depth[under])], under[-1]]
    hj[3:3 + max(2, nh // 8)] = under[len(under) // 2]
    return hj.astype(np.uint32)


def generated(name):
    """The generated rig `name` of GENERATED as a dict with an IK fixture's inputs (no recorded outputs): K = 3 calls - every handle
    enabled, a random half, all but handles 64 .. 127 (one wave's worth of the copy into LDS).  Data only, seeded by the name."""
    if name not in _generated:
        nj, nh = GENERATED_SIZES[GENERATED.index(name)]
        rng = np.random.default_rng(_SEEDS.get(name, 1000 * nj + nh))
        g = _rig(rng, nj)
        g.update(_no_keys(nj))
        g["handle_joints"] = _handles(rng, g["parent"], g["depth"], nh)
        g["targets"] = rng.uniform(-2, 2, (3, nh, 3)).astype(F)
        enabled = np.ones((3, nh), np.uint8)
        enabled[1] = rng.permutation(nh) < nh // 2
        enabled[2, 64:128] = 0
        g["enabled"], g["set_times"] = enabled, np.full(3, NAN, F)
        _generated[name] = g
    return _generated[name]


def generated_keyed(nj):
    """A rig of nj joints, half of them keyed with knot counts cycling through AC.KNOTS' 1, 2, 3 and 6 (0: the other half), and a
    pose to start from that is not the rest pose."""
    name = f"keyed{nj}"
    if name not in _generated:
        rng = np.random.default_rng(_SEEDS.get(name, 77 + nj))
        g = _rig(rng, nj)
        keyed = np.sort(rng.permutation(nj)[:nj // 2])
        counts = np.zeros(nj, np.int64)
        counts[keyed] = np.array([k for k in AC.KNOTS if k])[np.arange(len(keyed)) % 4]
        times, quats = [], []
        for j in range(nj):
            times.extend(AC.KNOTS[int(counts[j])])
            quats.extend(AC.quat_of_euler(rng.uniform(-40, 40, 3)) for _ in range(counts[j]))
        g["knot_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        g["knot_times"], g["knot_quats"] = np.array(times, F), np.array(quats, F).reshape(-1, 4)
        g["had"] = rng.uniform(-60, 60, (nj, 3)).astype(F)
        _generated[name] = g
    return _generated[name]


def posed_host(lib, g, t, rest=None):
    """srt_pt_rig_posed_host at time t: (euler_out[n, 3], posed_out[n, 16]); `rest` in place of the rig's rest pose."""
    parent, base, rest0, koff, ktimes, kquats = rig_arrays(g)
    n = len(parent)
    euler, posed = np.zeros((n, 3), F), np.zeros((n, 16), F)
    kt, kq = (ktimes, kquats) if len(ktimes) else (np.zeros(1, F), np.zeros((1, 4), F))
    rest = rest0 if rest is None else np.ascontiguousarray(rest, F)
    assert lib.srt_pt_rig_posed_host(n, H.P(parent), H.P(np.ascontiguousarray(g["extent"], F)), H.P(base), H.P(rest), H.P(koff), H.P(kt), H.P(kq),
                                     ctypes.c_float(float(t)), H.P(euler), H.P(posed)) == 0
    return euler, posed


def waves(chain):
    """The 64-lane groups of the kernel's workgroup that own a chain's joints: joint j belongs to lane j % BLOCK."""
    return {(int(j) % BLOCK) // 64 for j in chain}


def check_wide(g):
    """What wide200's record must hold, in the recorded (for_joints) order: the LDS form with handles' chains across waves, 64
    handles with repeats under one root, one of them on that root, a third of the joints keyed, set_time before calls 0 and 2."""
    par, hj = np.asarray(g["parent"]), [int(j) for j in g["handle_joints"]]
    nj, ch = len(par), chains(par, hj)
    keyed = np.diff(np.asarray(g["knot_offsets"], np.int64)) > 0
    assert nj == 200 <= LDS_JOINTS and len(hj) == 64 and max(len(c) for c in ch) <= 17          # (depth 16: 17 joints)
    assert (par < 0).sum() == 3 and len({c[-1] for c in ch}) == 1 and ch[0][-1] in hj and len(set(hj)) < len(hj)
    assert max(np.bincount(hj)) >= 8                                                            # many handles on one joint
    assert max(len(waves(c)) for c in ch) >= 2 and set().union(*(waves(c) for c in ch)) == {0, 1, 2, 3}
    assert keyed.sum() == nj // 3 and any(keyed[j] for c in ch for j in c) and not all(keyed[j] for c in ch for j in c)
    assert [bool(np.isfinite(t)) for t in g["set_times"]] == [True, False, True]
    assert g["enabled"][0].all() and 0 < g["enabled"][1].sum() < len(hj)


def rig_arrays(g):
    """srt_pt_skin_set_rig's arguments from an IK fixture."""
    return (np.ascontiguousarray(g["parent"], np.int32), np.ascontiguousarray(g["base"], F), np.ascontiguousarray(g["rest_pose"], F),
            np.ascontiguousarray(g["knot_offsets"], np.uint32), np.ascontiguousarray(g["knot_times"], F), np.ascontiguousarray(g["knot_quats"], F).reshape(-1, 4))


def chains(parent, handle_joints):
    """Per handle, the joints of its chain: its joint and every ancestor."""
    out = []
    for j in handle_joints:
        c, j = [], int(j)
        while j >= 0:
            c.append(j)
            j = int(parent[j])
        out.append(c)
    return out


def step_host(lib, parent, extent, pose, handle_joints, targets, enabled, calls=1):
    """srt_pt_rig_step_ik_host on a copy of `pose`: (status, the pose after `calls` calls)."""
    parent, extent = np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(extent, F)
    out = np.array(pose, F, copy=True, order="C")
    hj = np.ascontiguousarray(handle_joints, np.uint32)
    tg = np.ascontiguousarray(targets, F)
    en = None if enabled is None else np.ascontiguousarray(enabled, np.uint8)
    st = lib.srt_pt_rig_step_ik_host(len(parent), H.P(parent), H.P(extent), H.P(out), H.P(hj) if len(hj) else None, H.P(tg) if len(hj) else None,
                                     None if en is None else H.P(en), len(hj), calls)
    return st, out


def set_time_host(lib, g, pose, t):
    """Skeleton::set_time(t) on `pose` with the fixture's keys: keyed joints take srt_pt_rig_posed_host's Euler angles, the others keep theirs."""
    euler = posed_host(lib, g, t)[0]
    keyed = np.diff(np.asarray(g["knot_offsets"], np.int64)) > 0
    out = np.array(pose, F, copy=True)
    out[keyed] = euler[keyed]
    return out


def replay_host(lib, g):
    """The fixture's calls through the host definition: the pose after every call, (K, njoints, 3)."""
    pose = np.array(g["rest_pose"], F)
    out = []
    for c in range(len(g["targets"])):
        if not np.isnan(g["set_times"][c]):
            pose = set_time_host(lib, g, pose, g["set_times"][c])
        st, pose = step_host(lib, g["parent"], g["extent"], pose, g["handle_joints"], g["targets"][c], g["enabled"][c])
        assert st == 0
        out.append(pose)
    return np.stack(out)


_poses = {}


def generated_poses(lib, name):
    """replay_host of generated(name), computed once and left unchanged: what the kernel is held to."""
    if name not in _poses:
        _poses[name] = replay_host(lib, generated(name))
        _poses[name].setflags(write=False)
    return _poses[name]


def skin_joints(g):
    """srt_pt_skin_joint records for a fixture without a committed skin fixture: bind = translate(base + the extents in front), built in
    float64 and rounded - any float32 matrices are valid inputs, and IK does not read them."""
    import _skin_expected as E

    n = len(g["parent"])
    joints = np.zeros(n, E.JOINT_DTYPE)
    at = np.zeros((n, 3))
    for j in range(n):
        p = int(g["parent"][j])
        at[j] = np.asarray(g["base"], np.float64) if p < 0 else at[p] + np.asarray(g["extent"][p], np.float64)
        m = np.eye(4)
        m[:3, 3] = at[j]
        joints[j] = (np.ascontiguousarray(m.T.reshape(16), F), np.asarray(g["extent"][j], F), F(g["radius"][j]))
    return joints


# ---- the host emulation of pt_ik.h (tests/host_emu/ik_host.cpp, g++ -ffp-contract=off) and the sanitized program ----
_emu = None


def ik_emu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(H.build_host_lib("ik_host", ["ik_host.cpp"], extra=("-lm",)))
    return _emu


def sanitized_program():
    """tests/host_emu/ik_sanitized_main.cpp built with -fsanitize=address,undefined: a program of its own, run as its own process."""
    return H.build_host_lib("ik_sanitized", ["ik_sanitized_main.cpp"], program=True,
                            extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-lm"))


def emu_one_call(g, c=0, pose=None):
    """The intermediate values of the first iteration and the pose after one whole call, from the host emulation, for call c on the
    pose the fixture records before it (or on `pose`): dict(origin[n, 3], axes[n, 3, 3], current[n, 3], active[n], pose[n, 3])."""
    n, nh = len(g["parent"]), len(g["handle_joints"])
    parent, extent = np.ascontiguousarray(g["parent"], np.int32), np.ascontiguousarray(g["extent"], F)
    pose = np.array(g["pose_before"][c] if pose is None else pose, F, copy=True, order="C")
    hj, tg, en = np.ascontiguousarray(g["handle_joints"], np.uint32), np.ascontiguousarray(g["targets"][c], F), np.ascontiguousarray(g["enabled"][c], np.uint8)
    frame, current, active = np.zeros((n, 12), F), np.zeros((n, 3), F), np.zeros(n, np.uint32)
    ik_emu().ik_emu_call(H.P(parent), H.P(extent), n, H.P(hj), H.P(tg), H.P(en), nh, H.P(pose), H.P(frame), H.P(current), H.P(active))
    return {"origin": frame[:, :3], "axes": frame[:, 3:].reshape(n, 3, 3), "current": current, "active": active, "pose": pose}
