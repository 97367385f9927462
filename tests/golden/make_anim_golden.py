"""Records tests/golden/anim_objects.npz and anim_rig_<name>.npz: what the reference's own Anim_Pose::at / Pose::transform and
Skeleton::set_time / joint_to_posed / posed_mesh compute for the keys of tests/_anim_cases.py at _anim_cases.TIMES.
Runs only where the reference is (integration/_build/libdropin_pt_full.so, harness/anim_ref.cpp):  python tests/golden/make_anim_golden.py
The files hold data only: the knot tables that went in, and per time the pose (position, Euler angles, scale), Pose::transform(),
the joints' Euler angles, joint_to_posed and the skinned vertices.  The rigs are the two of tests/_skin_cases.rigs() and are stored
in the joint order of the committed skin_<name>.npz (Skeleton::for_joints order), so that a skin made from that fixture takes them
as they are.  Every case the tests rely on is asserted here, on the recorded values."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _anim_cases as AC  # noqa: E402
import _harness as H  # noqa: E402
import _skin_cases as SC  # noqa: E402

F = np.float32


def dot32(a, b):
    s = F(a[0]) * F(b[0])
    for i in range(1, 4):
        s = F(s + F(F(a[i]) * F(b[i])))
    return s


def record_objects(lib):
    offsets, times, values = AC.object_tracks()
    n, nt = AC.NOBJECTS, len(AC.TIMES)
    pose, trans = np.zeros((nt, n, 9), F), np.zeros((nt, n, 16), F)
    for k in range(n):
        o = np.ascontiguousarray(offsets[3 * k:3 * k + 4])
        p9, t16 = np.zeros((nt, 9), F), np.zeros((nt, 16), F)
        lib.dropin_anim_pose_reference(H.P(o), H.P(times), H.P(values), H.P(AC.TIMES), nt, H.P(p9), H.P(t16))
        pose[:, k], trans[:, k] = p9, t16
    # ---- what the fixture must contain ----
    counts = np.diff(offsets).reshape(n, 3)
    assert n == 70 and len(offsets) == 3 * n + 1
    for track in range(3):
        assert set(counts[:, track]) >= {0, 1, 2, 3, 6}, (track, set(counts[:, track]))
    filled = (counts > 0).sum(axis=1)
    assert filled.min() >= 1 and (filled == 1).any() and (filled == 2).any() and (filled == 3).any()
    empty_scale = np.nonzero(counts[:, 2] == 0)[0]
    assert len(empty_scale) and np.all(pose[:, empty_scale, 6:9] == 0)                 # an empty track gives T(): a zero scale
    k6, T = np.array(AC.KNOTS[6], F), AC.TIMES
    assert len(set(np.diff(k6))) > 1                                                  # unevenly spaced
    assert (T < k6[0]).any() and (T > k6[-1]).any() and k6[0] in T and k6[2] in T and k6[-1] in T
    assert ((T > k6[0]) & (T < k6[1])).any() and ((T > k6[-2]) & (T < k6[-1])).any() and ((T > k6[2]) & (T < k6[3])).any()
    k2 = np.array(AC.KNOTS[2], F)
    assert ((T > k2[0]) & (T < k2[1])).sum() >= 2
    rot = lambda k: values[offsets[3 * k + 1]:offsets[3 * k + 2]]                      # noqa: E731
    one_minus_eps = F(1.0) - F(0.00001)
    assert dot32(*rot(AC.FLIP)) < 0
    assert dot32(rot(AC.IDENTICAL)[0], rot(AC.IDENTICAL)[1]) >= one_minus_eps and np.array_equal(rot(AC.IDENTICAL)[0], rot(AC.IDENTICAL)[1])
    assert one_minus_eps <= abs(dot32(*rot(AC.NEAR_LERP))) < 1 and not np.array_equal(*rot(AC.NEAR_LERP))
    assert F(0.9999) < abs(dot32(*rot(AC.NEAR_SLERP))) < one_minus_eps
    for k, sign in ((AC.PITCH_UP, 1), (AC.PITCH_DOWN, -1)):                             # the cy <= EPS_F branch: eul[2] = 0, pitch +-90
        e = pose[:, k, 3:6]
        assert np.all(e[:, 2] == 0) and np.all(np.abs(e[:, 1] - sign * 90) < 0.05), (k, e)
    e = pose[:, AC.SECOND_SOLUTION, 3:6]
    assert np.all(np.abs(e[:, 1]) > 90), e                                             # eul1's pitch is within +-90: this is eul2
    assert abs(np.linalg.norm(rot(AC.NON_UNIT)[0]) - 1) > 0.1 and np.isfinite(trans[:, AC.NON_UNIT]).all()
    assert not rot(AC.ZERO).any() and np.isnan(pose[:, AC.ZERO, 3:5]).all() and np.isnan(trans[:, AC.ZERO]).any(axis=1).all()   # (NaN, NaN, 0): cy > EPS_F is false for a NaN
    assert np.isnan(pose[-1, AC.ZERO_SECOND, 3:5]).all() and np.isfinite(pose[0, AC.ZERO_SECOND]).all()
    assert len(AC.scene_objects({"track_offsets": offsets, "trans": trans})) >= 12
    path = os.path.join(HERE, "anim_objects.npz")
    np.savez_compressed(path, track_offsets=offsets, knot_times=times, knot_values=values, times=AC.TIMES, pose=pose, trans=trans)
    print("objects", n, "knots", len(times), "times", nt, "NaN matrices", int(np.isnan(trans).any(axis=2).sum()), os.path.getsize(path), "bytes")


def record_rig(lib, name):
    rig = SC.rigs()[name]
    skin = np.load(os.path.join(HERE, f"skin_{name}.npz"))
    pos, nrm, idx = (np.ascontiguousarray(a, t) for a, t in zip(rig["mesh"](), (F, F, np.uint32)))
    assert np.array_equal(pos, skin["pos"]) and np.array_equal(idx, skin["idx"])
    nv, nj, nt = len(pos), len(rig["parent"]), len(AC.TIMES)
    parent, extent, radius, base = np.array(rig["parent"], np.int32), np.array(rig["extent"], F), np.array(rig["radius"], F), np.array(rig["base"], F)
    rest, keys = AC.rig_keys(name, nj)
    assert 0 < len(keys) < nj                                                          # some joints keyed, some left at their rest pose
    offs, times, quats = [0], [], []
    for j in range(nj):
        ts, qs = keys.get(j, ([], []))
        times.extend(ts)
        quats.extend(qs)
        offs.append(len(times))
    offs, times, quats = np.array(offs, np.uint32), np.array(times, F), np.array(quats, F).reshape(-1, 4)
    order, euler, posed, mesh = np.zeros(nj, np.uint32), np.zeros((nt, nj, 3), F), np.zeros((nt, nj, 16), F), np.zeros((nt, nv, 3), F)
    st = lib.dropin_anim_rig_reference(H.P(pos), H.P(nrm), nv, H.P(idx), len(idx), H.P(parent), H.P(extent), H.P(radius), H.P(rest), nj, H.P(base), H.P(offs),
                                       H.P(times), H.P(quats), H.P(AC.TIMES), nt, H.P(order), H.P(euler), H.P(posed), H.P(mesh))
    assert st == 0, name
    # the skinned vertices depend on the order Skeleton::for_joints visits the joints in (a vertex's float sum follows it): they are
    # only good for a skin in the committed fixture's order when this process visited the joints in that order
    assert np.array_equal(order, skin["order"]), (name, "for_joints order", order, "differs from the committed skin fixture's", skin["order"], "- run again")
    inv = np.zeros(nj, np.int64)
    inv[order] = np.arange(nj)
    parent_fo = np.array([-1 if parent[j] < 0 else inv[parent[j]] for j in order], np.int32)
    assert all(p < k for k, p in enumerate(parent_fo))                                 # parents come first
    knot_offsets, ktimes, kquats = [0], [], []
    for j in order:
        ktimes.extend(times[offs[j]:offs[j + 1]])
        kquats.extend(quats[offs[j]:offs[j + 1]])
        knot_offsets.append(len(ktimes))
    keyed = np.diff(knot_offsets) > 0
    assert np.array_equal(euler[:, ~keyed], np.broadcast_to(rest[order][~keyed], euler[:, ~keyed].shape))   # set_time left them alone
    assert np.array_equal(extent[order], skin["extent"])
    path = os.path.join(HERE, f"anim_rig_{name}.npz")
    np.savez_compressed(path, order=order, parent=parent_fo, extent=extent[order], base=base, rest_pose=rest[order], knot_offsets=np.array(knot_offsets, np.uint32),
                        knot_times=np.array(ktimes, F), knot_quats=np.array(kquats, F).reshape(-1, 4), times=AC.TIMES, euler=euler, posed=posed, mesh_pos=mesh)
    print(name, "joints", nj, "order", order, "keyed", keyed.astype(int), "knots", len(ktimes), os.path.getsize(path), "bytes")


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "integration", "_build", "libdropin_pt_full.so"))
    record_objects(lib)
    for name in AC.RIGS:
        record_rig(lib, name)


if __name__ == "__main__":
    main()
