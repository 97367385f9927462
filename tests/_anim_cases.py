"""Keys, times and rigs of the timeline tests (test_pt_anim_host.py, test_pt_anim_gpu.py, tests/golden/make_anim_golden.py).

object_tracks() and rig_keys() are what make_anim_golden.py runs through the reference (its own Anim_Pose, Skeleton::set_time and
Joint::joint_to_posed) and records as tests/golden/anim_objects.npz and anim_rig_<name>.npz; the tests read the keys back from the
fixtures, so that what is evaluated is what was recorded.  Everything here is data: knot times, knot values, time lists."""
import ctypes
import os

import numpy as np

import _harness as H

F = np.float32

# The knot times of the tracks by knot count (K6: unevenly spaced) and the times every object and rig is evaluated at.  Against K6:
# before the first knot, on it, inside the first interval (k0 is mirrored), on an interior knot, inside interior intervals, inside
# the last interval (k3 is mirrored), on the last knot, after it.  K2's interval holds 0.9, 1.25 and 1.7 with both neighbours mirrored.
KNOTS = {0: [], 1: [1.0], 2: [0.5, 2.0], 3: [0.0, 1.25, 4.0], 6: [0.0, 0.5, 1.25, 2.0, 3.5, 4.0]}
TIMES = np.array([-1.0, 0.0, 0.2, 0.5, 0.9, 1.25, 1.7, 2.0, 2.75, 3.75, 4.0, 5.5], F)
NOBJECTS = 70          # one wave of 64 lanes and a partial second one

# objects 0 .. 9: the rotation cases (see _special_rotations); 10 .. 15: one or two of the three tracks filled; the rest seeded
FLIP, IDENTICAL, NEAR_LERP, NEAR_SLERP, PITCH_UP, PITCH_DOWN, SECOND_SOLUTION, NON_UNIT, ZERO, ZERO_SECOND = range(10)


def quat_of_euler(deg):
    """A unit quaternion xyzw of the rotation rotate(z, Z) * rotate(y, Y) * rotate(x, X), built in float64 and rounded: an input like any other."""
    x, y, z = np.radians(np.asarray(deg, np.float64)) / 2.0
    qx, qy, qz = np.array([np.sin(x), 0, 0, np.cos(x)]), np.array([0, np.sin(y), 0, np.cos(y)]), np.array([0, 0, np.sin(z), np.cos(z)])

    def mul(a, b):
        av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
        return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])

    return mul(mul(qz, qy), qx).astype(F)


def _about(axis, half_angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([np.sin(half_angle) * axis, [np.cos(half_angle)]]).astype(F)


def _special_rotations():
    """object -> (knot times, quaternions) of its rotation track."""
    ident = np.array([0, 0, 0, 1], F)
    return {
        FLIP: (KNOTS[2], [quat_of_euler([10, 20, 30]), -quat_of_euler([40, -10, 60])]),                    # dot < 0: slerp flips q0
        IDENTICAL: (KNOTS[3], [quat_of_euler([15, 25, 35])] * 3),                                          # dot = 1: the lerp branch
        NEAR_LERP: (KNOTS[2], [ident, _about([1, 2, 3], 0.0040)]),                                         # dot = 1 - 8e-6 >= 1 - EPS_F: lerp
        NEAR_SLERP: (KNOTS[2], [ident, _about([1, 2, 3], 0.0050)]),                                        # dot = 1 - 1.25e-5 < 1 - EPS_F: slerp
        PITCH_UP: (KNOTS[2], [quat_of_euler([30, 90, 0]), quat_of_euler([30, 90, 0])]),                    # cy <= EPS_F: the gimbal branch
        PITCH_DOWN: (KNOTS[1], [quat_of_euler([-20, -90, 0])]),
        SECOND_SOLUTION: (KNOTS[2], [quat_of_euler([0, 170, 0]), quat_of_euler([0, 175, 5])]),             # d1 > d2: eul2 is returned
        NON_UNIT: (KNOTS[2], [F(2.5) * quat_of_euler([10, 20, 30]), F(0.5) * quat_of_euler([50, -20, 10])]),
        ZERO: (KNOTS[1], [np.zeros(4, F)]),                                                                # unit() divides by 0: NaN
        ZERO_SECOND: (KNOTS[2], [quat_of_euler([1, 2, 3]), np.zeros(4, F)]),
    }


def object_tracks():
    """(track_offsets[3 * NOBJECTS + 1], knot_times[n], knot_values[n, 4]) of the recorded objects."""
    rng = np.random.default_rng(2024)
    special = _special_rotations()
    partial = {10: (3, 0, 0), 11: (0, 6, 0), 12: (0, 0, 2), 13: (6, 1, 0), 14: (2, 0, 6), 15: (0, 3, 1)}
    counts = [0, 1, 2, 3, 6]
    offsets, times, values = [0], [], []

    def vec_track(n, lo, hi):
        for t in KNOTS[n]:
            times.append(t)
            values.append(np.concatenate([rng.uniform(lo, hi), [0.0]]))
        offsets.append(len(times))

    def quat_track(ts, qs):
        for t, q in zip(ts, qs):
            times.append(t)
            values.append(np.asarray(q, np.float64))
        offsets.append(len(times))

    for k in range(NOBJECTS):
        if k in special:
            n_pos, n_scale = 1 + k % 2, 2
            ts, qs = special[k]
        else:
            n_pos, n_rot, n_scale = partial.get(k) or (counts[k % 5], counts[(k // 5) % 5], counts[(k // 2 + 3) % 5])
            if n_pos == n_rot == n_scale == 0:
                n_rot = 6
            ts = KNOTS[n_rot]
            qs = []
            for _ in ts:
                q = rng.normal(size=4)
                qs.append(q / np.linalg.norm(q))
        vec_track(n_pos, [-0.55, 0.1, -0.55], [0.55, 0.9, 0.55])
        quat_track(ts, qs)
        vec_track(n_scale, [0.02] * 3, [0.06] * 3)
    return np.array(offsets, np.uint32), np.array(times, F), np.array(values, F).reshape(-1, 4)


def rig_keys(name, njoints):
    """(rest_pose[njoints, 3], {joint: (knot times, quaternions)}) in the caller's joint order of _skin_cases.rigs()[name]: some joints
    keyed, the others left at their rest pose."""
    import _skin_cases as SC

    rest = np.array(SC.rigs()[name]["poses"][0], F)
    assert rest.shape == (njoints, 3)
    rng = np.random.default_rng(7 + njoints)

    def keys(n, spread):
        return KNOTS[n], [quat_of_euler(rng.uniform(-spread, spread, 3)) for _ in KNOTS[n]]

    if name == "blob_chain3":
        return rest, {0: keys(6, 25.0), 2: keys(2, 30.0)}
    return rest, {1: keys(3, 40.0), 3: keys(6, 30.0), 4: keys(1, 45.0)}


RIGS = ("blob_chain3", "blob128_tree5")


def load_objects():
    return np.load(os.path.join(H.GOLDEN, "anim_objects.npz"))


def load_rig(name):
    return np.load(os.path.join(H.GOLDEN, f"anim_rig_{name}.npz"))


def scene_objects(g):
    """The recorded objects a scene can take as they are: all three tracks keyed and every recorded matrix finite."""
    off = g["track_offsets"].reshape(-1)
    keyed = np.array([all(off[3 * k + i + 1] > off[3 * k + i] for i in range(3)) for k in range(len(g["trans"][0]))])
    return np.nonzero(keyed & np.isfinite(g["trans"]).all(axis=(0, 2)))[0]


def sub_tracks(g, objects):
    """(track_offsets, knot_times, knot_values) of the listed recorded objects alone, re-packed."""
    off = g["track_offsets"].reshape(-1)
    offsets, times, values = [0], [], []
    for k in objects:
        for i in range(3):
            b, e = int(off[3 * k + i]), int(off[3 * k + i + 1])
            times.extend(g["knot_times"][b:e])
            values.extend(g["knot_values"][b:e])
            offsets.append(len(times))
    return np.array(offsets, np.uint32), np.array(times, F), np.array(values, F).reshape(-1, 4)


def bits_equal(a, b):
    """Bit equality of float32 arrays, with every NaN equal to every NaN."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def mismatches(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return int(np.sum(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))))


# ---- the host emulation of pt_anim.h (tests/host_emu/anim_host.cpp, g++ -ffp-contract=off) ----
_emu = None


def anim_emu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(H.build_host_lib("anim_host", ["anim_host.cpp"], extra=("-lm",)))
        _emu.anim_emu_hypot_sweep.restype = ctypes.c_uint64
        _emu.anim_emu_hypot_sweep.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    return _emu


def sanitized_program():
    """tests/host_emu/anim_sanitized_main.cpp built with -fsanitize=address,undefined: a program of its own, run as its own process."""
    return H.build_host_lib("anim_sanitized", ["anim_sanitized_main.cpp"], program=True,
                            extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-lm"))


def emu_objects(offsets, times, values, t):
    """(pose9[n, 9], trans[n, 16]) of every object at time t."""
    n = (len(offsets) - 1) // 3
    pose, trans = np.zeros((n, 9), F), np.zeros((n, 16), F)
    anim_emu().anim_emu_objects(H.P(offsets), H.P(times), H.P(values), n, ctypes.c_float(float(t)), H.P(pose), H.P(trans))
    return pose, trans


def emu_rig(parent, extent, base, rest, knot_offsets, times, quats, t):
    """(euler[n, 3], posed[n, 16]) after Skeleton::set_time(t)."""
    n = len(parent)
    euler, posed = np.zeros((n, 3), F), np.zeros((n, 16), F)
    anim_emu().anim_emu_rig(H.P(parent), H.P(extent), H.P(base), H.P(rest), H.P(knot_offsets), H.P(times), H.P(quats), n, ctypes.c_float(float(t)),
                            H.P(euler), H.P(posed))
    return euler, posed


def rig_arrays(g):
    """The arguments of srt_pt_skin_set_rig / srt_pt_rig_posed_host from a rig fixture, contiguous and typed."""
    return (np.ascontiguousarray(g["parent"], np.int32), np.ascontiguousarray(g["extent"], F), np.ascontiguousarray(g["base"], F),
            np.ascontiguousarray(g["rest_pose"], F), np.ascontiguousarray(g["knot_offsets"], np.uint32), np.ascontiguousarray(g["knot_times"], F),
            np.ascontiguousarray(g["knot_quats"], F))
