"""Keys, times and scenes of the shading-timeline tests (test_pt_shading_host.py, test_pt_shading_gpu.py,
tests/golden/make_shading_golden.py).

describe(group) is what make_shading_golden.py runs through the reference (its own Anim_Material::at, Spectrum::to_linear,
Material::emissive, Scene_Light::set_time, Scene_Light::radiance and Pose::transform) and records as tests/golden/anim_shading.npz; the
tests read the keys back from the fixture, so that what is evaluated is what was recorded.  Two groups: "record" - 20 materials of all
five types, 300 delta lights and the environment light, compared through values() and dump_shading() only, never rendered - and
"render" - the keys of three materials (a Lambertian wall, the glass, the area light's emission) and three delta lights of the Cornell
boxes the GPU tests render.  Everything here is data: knot times, knot values, time lists, and which recorded number goes where."""
import copy
import ctypes
import os

import numpy as np

import _anim_cases as AC
import _harness as H

F = np.float32
KNOTS, TIMES = AC.KNOTS, AC.TIMES
LAMBERTIAN, MIRROR, GLASS, DIFFUSE_LIGHT, REFRACT = range(5)                 # SRT_MAT_*
DIRECTIONAL, POINT, SPOT = range(3)                                          # SRT_LIGHT_*
REF_LIGHT_TYPE = {DIRECTIONAL: 0, POINT: 3, SPOT: 4}                         # Light_Type of scene/light.h
GROUPS = ("record", "render")
NLIGHTS = 300                                                                # 4 full waves and 44 lanes behind the materials' 20
OVERSHOOT, EMISSIVE_UNKEYED_INTENSITY, INTENSITY_ENDS_AT_ZERO = 0, 1, 2      # materials of "record"
RENDER_MATERIALS, RENDER_LIGHTS = (0, 6, 7), (0, 1, 2)                        # of scenes.cornell_box("cbox") / _cases.pt_scene("cbox_deltalights")
T_BETWEEN, T_ZERO_EMISSION = 4, 10                                           # indices into TIMES: 0.9, and 4.0 - the last knot of K3 and K6


def _tracks():
    offsets, times, values = [0], [], []

    def add(ts, vs):
        for t, v in zip(ts, vs):
            v = np.atleast_1d(np.asarray(v, np.float64))
            times.append(t)
            values.append(np.concatenate([v, np.zeros(4 - len(v))]))
        offsets.append(len(times))

    return offsets, times, values, add


def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def describe(group):
    """{"mat_types", "light_types", "light_init" (options6 + pose9 per light), "env", "track_offsets", "knot_times", "knot_values"}: the tracks
    in the order of srt_pt_shading_timeline_create."""
    offsets, times, values, add = _tracks()
    if group == "render":
        mat_types = [LAMBERTIAN, GLASS, DIFFUSE_LIGHT]
        k6, k3, k2 = KNOTS[6], KNOTS[3], KNOTS[2]
        add(k6, [[0.75, 0.27, 0.27], [0.2, 0.8, 0.3], [0.9, 0.9, 0.2], [0.3, 0.3, 0.85], [0.6, 0.2, 0.7], [0.5, 0.5, 0.5]])       # the left wall's albedo
        for _ in range(5):
            add([], [])
        add([], [])                                                                                                                   # glass: no albedo key
        add(k2, [[1.0, 1.0, 1.0], [0.6, 0.7, 0.9]])
        add(k3, [[1.0, 1.0, 1.0], [0.7, 0.9, 0.6], [0.95, 0.85, 0.8]])
        add([], [])
        add([], [])
        add(k3, [1.5, 1.25, 1.7])
        for _ in range(3):                                                                                                            # the area light: emissive and intensity
            add([], [])
        add(k2, [[1.0, 1.0, 1.0], [1.0, 0.8, 0.6]])
        add(k3, [10.0, 6.0, 0.0])                                                                                                     # .. whose last knot is exactly 0
        add([], [])
        light_types = [POINT, SPOT, DIRECTIONAL]
        init = np.zeros((3, 15))
        init[:, :6], init[:, 12:] = [1, 1, 1, 1, 30, 35], 1
        add(k3, [[1.0, 0.8, 0.6], [0.5, 0.9, 1.0], [1.0, 1.0, 1.0]]); add(k2, [0.6, 1.4]); add([], [])                                # point: options only
        for _ in range(3):
            add([], [])
        add(k2, [[0.8, 0.9, 1.0], [1.0, 0.7, 0.7]]); add(k3, [2.5, 1.5, 3.0]); add(k2, [[35.0, 70.0], [20.0, 45.0]])                  # spot: both
        add(k3, [[-0.25, 0.9, -0.1], [0.1, 0.85, 0.1], [0.3, 0.9, -0.2]])
        add(k2, [AC.quat_of_euler([20, 0, -12]), AC.quat_of_euler([-15, 30, 10])]); add([1.0], [[1.0, 1.0, 1.0]])
        for _ in range(3):                                                                                                            # directional: pose only
            add([], [])
        add([1.0], [[0.0, 0.0, 0.0]]); add(k3, [AC.quat_of_euler([28, 0, 17]), AC.quat_of_euler([-20, 10, 40]), AC.quat_of_euler([45, -30, 0])])
        add([1.0], [[1.0, 1.0, 1.0]])
        return {"mat_types": np.array(mat_types, np.uint32), "light_types": np.array(light_types, np.uint32), "light_init": init.astype(F), "env": False,
                "track_offsets": np.array(offsets, np.uint32), "knot_times": np.array(times, F), "knot_values": np.array(values, F).reshape(-1, 4)}
    assert group == "record"
    rng = np.random.default_rng(462)
    counts = [0, 1, 2, 3, 6]

    def spectrum_track(n):
        add(KNOTS[n], rng.uniform(0.05, 0.95, (n, 3)))

    def scalar_track(n, lo, hi):
        add(KNOTS[n], rng.uniform(lo, hi, n))

    mat_types = []
    for k in range(20):
        if k == OVERSHOOT:
            # channel 0 rises to 1, stays and falls: Catmull-Rom carries it above 1 between the two; channel 1 stays at or below the
            # to_linear threshold, a negative knot included; channel 2 is ordinary
            mat_types.append(LAMBERTIAN)
            add(KNOTS[6], np.stack([[0.0, 1.0, 1.0, 0.0, 0.5, 0.5], [0.03, 0.04045, -0.2, 0.02, 0.01, 0.04], rng.uniform(0.1, 0.9, 6)], axis=1))
            spectrum_track(1)
            for _ in range(4):
                add([], [])
        elif k == EMISSIVE_UNKEYED_INTENSITY:
            mat_types.append(DIFFUSE_LIGHT)
            for _ in range(3):
                add([], [])
            spectrum_track(3)
            add([], []); add([], [])
        elif k == INTENSITY_ENDS_AT_ZERO:
            mat_types.append(DIFFUSE_LIGHT)
            for _ in range(3):
                add([], [])
            spectrum_track(2)
            add(KNOTS[3], [4.0, 9.0, 0.0])
            add([], [])
        else:
            mat_types.append([LAMBERTIAN, MIRROR, GLASS, DIFFUSE_LIGHT, REFRACT][k % 5])
            n = [counts[(k + i * (1 + k // 5)) % 5] for i in range(6)]
            if not any(n):
                n[k % 6] = 3
            for i in range(4):
                spectrum_track(n[i])
            scalar_track(n[4], 0.5, 8.0)
            scalar_track(n[5], 1.1, 1.8)
    light_types, init = [], np.zeros((NLIGHTS, 15))
    for k in range(NLIGHTS):
        light_types.append((k // 3) % 3 if k < 9 else int(rng.integers(0, 3)))
        mode = k % 3 if k < 9 else int(rng.integers(0, 3))                            # 0: options only, 1: pose only, 2: both
        init[k] = np.concatenate([rng.uniform(0.1, 1.0, 3), rng.uniform(0.2, 5.0, 1), [rng.uniform(10, 40), rng.uniform(45, 80)], rng.uniform(-0.5, 0.9, 3),
                                  rng.uniform(-90, 90, 3), rng.uniform(0.5, 1.5, 3)])
        n = [counts[int(c)] for c in rng.integers(0, 5, 6)] if k >= 9 else [3, 2, 6, 6, 3, 2]
        if k >= 9 and not any(n[:3]):
            n[int(rng.integers(0, 3))] = 2
        if k >= 9 and not any(n[3:]):
            n[3 + int(rng.integers(0, 3))] = 6
        if mode == 1:
            n[:3] = [0, 0, 0]
        if mode == 0:
            n[3:] = [0, 0, 0]
        spectrum_track(n[0]); scalar_track(n[1], 0.2, 5.0)
        add(KNOTS[n[2]], np.stack([rng.uniform(10, 40, n[2]), rng.uniform(45, 80, n[2])], axis=1))
        add(KNOTS[n[3]], rng.uniform(-0.5, 0.9, (n[3], 3))); add(KNOTS[n[4]], _unit_quats(rng, n[4])); add(KNOTS[n[5]], rng.uniform(0.5, 1.5, (n[5], 3)))
    spectrum_track(6); scalar_track(3, 0.1, 2.0)                                      # the environment light
    return {"mat_types": np.array(mat_types, np.uint32), "light_types": np.array(light_types, np.uint32), "light_init": init.astype(F), "env": True,
            "track_offsets": np.array(offsets, np.uint32), "knot_times": np.array(times, F), "knot_values": np.array(values, F).reshape(-1, 4)}


_golden = None


def load():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(H.GOLDEN, "anim_shading.npz")))
    return _golden


def tracks(g, group):
    return (np.ascontiguousarray(g[group + "_track_offsets"], np.uint32), np.ascontiguousarray(g[group + "_knot_times"], F),
            np.ascontiguousarray(g[group + "_knot_values"], F).reshape(-1, 4))


def keyed(g, group):
    """(options keyed, pose keyed) per light of the group."""
    off, nm = g[group + "_track_offsets"].astype(np.int64), len(g[group + "_mat_types"])
    lo = off[6 * nm:6 * nm + 6 * len(g[group + "_light_types"]) + 1]
    return lo[3::6] > lo[0:-1:6], lo[6::6] > lo[3::6]


def material_values(g, group, ti):
    """The recorded options of time TIMES[ti] as srt_pt_update_materials takes them (MATERIAL_DTYPE): by committed type, the mapping of
    Pathtracer::build_scene (rays/pathtracer.cpp:93-117); the fields a type does not read are zero."""
    import srt_amd

    rows, types = g[group + "_mat_out"][ti], g[group + "_mat_types"]
    out = np.zeros(len(types), srt_amd.MATERIAL_DTYPE)
    for k, (ty, r) in enumerate(zip(types, rows)):
        out[k]["type"] = ty
        if ty == LAMBERTIAN:
            out[k]["a"] = r[14:17]                        # albedo.to_linear()
        elif ty == MIRROR:
            out[k]["a"] = r[3:6]
        elif ty == GLASS:
            out[k]["a"], out[k]["b"], out[k]["ior"] = r[6:9], r[3:6], r[13]
        elif ty == DIFFUSE_LIGHT:
            out[k]["a"] = r[17:20]                        # Material::emissive()
        else:
            out[k]["a"], out[k]["ior"] = r[6:9], r[13]
    return out


def stored(materials):
    """The records the kernels read: BSDF_Lambertian divides the albedo by PI_F (rays/bsdf.h:26); IEEE float32 division, as in C."""
    out = materials.copy()
    lam = out["type"] == LAMBERTIAN
    out["a"][lam] = out["a"][lam] / F(3.14159265358979323846)
    return out


def light_values(g, group, ti, scene_lights):
    """(nlights, 21) = radiance3, angle_bounds2, trans16 of time TIMES[ti]: the recorded values where the triple has a key, the scene's otherwise."""
    rows = g[group + "_light_out"][ti]
    opt, pose = keyed(g, group)
    out = np.zeros((len(rows), 21), F)
    for j, (r, l) in enumerate(zip(rows, scene_lights)):
        out[j, :3] = r[6:9] if opt[j] else l["radiance"]
        out[j, 3:5] = r[4:6] if opt[j] else l.get("angle_bounds", (0.0, 0.0))
        out[j, 5:] = r[9:25] if pose[j] else l["T"]
    return out


def record_scene(g):
    """A Cornell box with the 20 recorded materials appended (no object uses them) and the 300 recorded lights, each committed with the
    values the reference's light had at TIMES[0] - what an unkeyed triple keeps.  Compared through dumps only, never rendered."""
    import _cases

    s = copy.deepcopy(_cases.pt_scene("cbox"))
    s["env"] = {"type": 1, "radiance": np.array([0.3, 0.4, 0.5], F)}
    first = len(s["materials"])
    for ty in g["record_mat_types"]:
        s["materials"].append({"type": int(ty), "a": np.full(3, 0.5, F), "b": np.full(3, 0.25, F), "ior": 1.5})
    s["lights"] = [{"type": int(ty), "radiance": r[6:9].copy(), "angle_bounds": r[4:6].copy(), "T": r[9:25].copy()}
                   for ty, r in zip(g["record_light_types"], g["record_light_out"][0])]
    return s, np.arange(first, first + len(g["record_mat_types"]), dtype=np.uint32), np.arange(NLIGHTS, dtype=np.uint32)


def with_values(scene, material_idx, materials, light_idx, lights21, env=None):
    """The scene description a fresh commit takes: `scene` with the listed materials and lights replaced by the given values."""
    s = copy.deepcopy(scene)
    for k, m in zip(material_idx, materials):
        assert int(m["type"]) == int(s["materials"][k]["type"])
        s["materials"][k] = {"type": int(m["type"]), "a": m["a"].copy(), "b": m["b"].copy(), "ior": float(m["ior"])}
    for j, l in zip(light_idx, lights21):
        s["lights"][j] = {"type": s["lights"][j]["type"], "radiance": l[:3].copy(), "angle_bounds": l[3:5].copy(), "T": l[5:].copy()}
    if env is not None:
        s["env"] = {"type": s["env"]["type"], "radiance": np.asarray(env, F)}
    return s


def sub_tracks(g, group, track_ids):
    """(track_offsets, knot_times, knot_values) of the listed tracks of a group alone, re-packed."""
    off, kt, kv = tracks(g, group)
    offsets, times, values = [0], [], []
    for q in track_ids:
        times.extend(kt[off[q]:off[q + 1]])
        values.extend(kv[off[q]:off[q + 1]])
        offsets.append(len(times))
    return np.array(offsets, np.uint32), np.array(times, F), np.array(values, F).reshape(-1, 4)


def dumps_equal(a, b):
    return np.array_equal(a["materials"]["type"], b["materials"]["type"]) and all(AC.bits_equal(a["materials"][f], b["materials"][f]) for f in ("a", "b", "ior")) and \
        np.array_equal(a["light_heads"], b["light_heads"]) and AC.bits_equal(a["lights"], b["lights"]) and a["env_type"] == b["env_type"] and \
        AC.bits_equal(a["env_radiance"], b["env_radiance"])


# ---- the host emulation of pt_anim.h's shading items (tests/host_emu/shading_host.cpp, g++ -ffp-contract=off) ----
_emu = None
SRC = os.path.join(H.ROOT, "tests", "host_emu", "shading_host.cpp")


def shading_emu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(H.build_host_lib("shading_host", [SRC], extra=("-lm",)))
    return _emu


def sanitized_program():
    """The same file with its main(), built with -fsanitize=address,undefined: a program of its own, run as its own process."""
    return H.build_host_lib("shading_sanitized", [SRC], program=True,
                            extra=("-g", "-DSHADING_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-lm"))


def emu_values(g, group, t):
    """(materials (n, 7) = a3 b3 ior as srt_pt_update_materials takes them, stored a (n, 3), options (n, 14), lights (n, 21) with
    untouched entries NaN-free zeros, light flags (n, 2), env (3))."""
    off, kt, kv = tracks(g, group)
    types = np.ascontiguousarray(g[group + "_mat_types"], np.uint32)
    nm, nl = len(types), len(g[group + "_light_types"])
    mats, stored_a, options = np.zeros((nm, 7), F), np.zeros((nm, 3), F), np.zeros((nm, 14), F)
    lights, flags, env = np.zeros((nl, 21), F), np.zeros((nl, 2), np.uint32), np.zeros(3, F)
    emu = shading_emu()
    emu.shading_emu_materials(H.P(off), H.P(kt), H.P(kv), H.P(types), nm, ctypes.c_float(float(t)), H.P(options), H.P(mats), H.P(stored_a))
    lo = np.ascontiguousarray(off[6 * nm:])
    emu.shading_emu_lights(H.P(lo), H.P(kt), H.P(kv), nl, ctypes.c_float(float(t)), H.P(flags), H.P(lights))
    if len(lo) == 6 * nl + 3:
        emu.shading_emu_env(H.P(np.ascontiguousarray(lo[6 * nl:])), H.P(kt), H.P(kv), ctypes.c_float(float(t)), H.P(env))
    return mats, stored_a, options, lights, flags, env
