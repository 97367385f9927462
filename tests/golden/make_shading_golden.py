"""Records tests/golden/anim_shading.npz: what the reference's own Material::Anim_Material::at / Spectrum::to_linear / Material::emissive
and Scene_Light::set_time / Scene_Light::radiance / Pose::transform compute for the keys of tests/_shading_cases.py at _shading_cases.TIMES.
Runs only where the reference is (integration/_build/libdropin_pt_full.so, harness/anim_shading_ref.cpp):
    python tests/golden/make_shading_golden.py
The file holds data only: per group ("record", "render") the knot tables that went in, the materials' committed types, the lights'
types and starting values, and per time and material the six options, albedo.to_linear() and Material::emissive() (20 floats), per time
and light the options, Scene_Light::radiance() and pose.transform() (25 floats), per time the environment light's radiance.  Every case
the tests rely on is asserted here, on the recorded values."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _harness as H  # noqa: E402
import _shading_cases as SH  # noqa: E402

F = np.float32


def record(lib, group):
    d = SH.describe(group)
    off, times, values = d["track_offsets"], d["knot_times"], d["knot_values"]
    nm, nl, nt = len(d["mat_types"]), len(d["light_types"]), len(SH.TIMES)
    assert len(off) == 6 * nm + 6 * nl + (2 if d["env"] else 0) + 1 and off[-1] == len(times) == len(values)
    mat_out, light_out, env_out = np.zeros((nt, nm, 20), F), np.zeros((nt, nl, 25), F), np.zeros((nt, 3), F)
    for k in range(nm):
        o, rows = np.ascontiguousarray(off[6 * k:6 * k + 7]), np.zeros((nt, 20), F)
        lib.dropin_anim_material_reference(H.P(o), H.P(times), H.P(values), H.P(SH.TIMES), nt, H.P(rows))
        mat_out[:, k] = rows
    for j in range(nl):
        o, rows = np.ascontiguousarray(off[6 * nm + 6 * j:6 * nm + 6 * j + 7]), np.zeros((nt, 25), F)
        init = np.ascontiguousarray(d["light_init"][j])
        lib.dropin_anim_light_reference(SH.REF_LIGHT_TYPE[int(d["light_types"][j])], H.P(init[:6].copy()), H.P(init[6:].copy()), H.P(o), H.P(times), H.P(values),
                                        H.P(SH.TIMES), nt, H.P(rows))
        light_out[:, j] = rows
    if d["env"]:      # the environment light is a Scene_Light of type sphere with option keys only
        e = off[6 * nm + 6 * nl:]
        o, rows = np.array([e[0], e[1], e[2], e[2], e[2], e[2], e[2]], np.uint32), np.zeros((nt, 25), F)
        lib.dropin_anim_light_reference(1, H.P(np.array([1, 1, 1, 1, 30, 35], F)), H.P(np.array([0, 0, 0, 0, 0, 0, 1, 1, 1], F)), H.P(o), H.P(times), H.P(values),
                                        H.P(SH.TIMES), nt, H.P(rows))
        env_out = rows[:, 6:9].copy()
    out = {group + "_mat_types": d["mat_types"], group + "_light_types": d["light_types"], group + "_light_init": d["light_init"], group + "_track_offsets": off,
           group + "_knot_times": times, group + "_knot_values": values, group + "_mat_out": mat_out, group + "_light_out": light_out, group + "_env_out": env_out}
    return d, out


def check_record(d, g):
    """What the fixture must contain."""
    T, off = SH.TIMES, d["track_offsets"].astype(np.int64)
    nm, nl = len(d["mat_types"]), len(d["light_types"])
    mat_out, light_out = g["record_mat_out"], g["record_light_out"]
    assert set(d["mat_types"]) == {0, 1, 2, 3, 4} and nm == 20 and nl == SH.NLIGHTS == 300
    counts = np.diff(off)
    mc, lc = counts[:6 * nm].reshape(nm, 6), counts[6 * nm:6 * nm + 6 * nl].reshape(nl, 6)
    for i in range(6):
        assert set(mc[:, i]) >= {0, 1, 2, 3, 6}, (i, set(mc[:, i]))
        assert set(lc[:, i]) >= {0, 1, 2, 3, 6}, (i, set(lc[:, i]))
    assert (mc.sum(axis=1) > 0).all() and (lc.sum(axis=1) > 0).all()
    k6 = np.array(SH.KNOTS[6], F)
    assert len(set(np.diff(k6))) > 1                                                   # unevenly spaced
    assert (T < k6[0]).any() and (T > k6[-1]).any() and k6[0] in T and k6[2] in T and k6[-1] in T and ((T > k6[1]) & (T < k6[2])).any()
    # an empty track gives T(): zero options
    for i, sl in enumerate((slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, 13), slice(13, 14))):
        empty = mc[:, i] == 0
        assert empty.any() and np.all(mat_out[:, empty, sl] == 0), i
    over = mat_out[:, SH.OVERSHOOT]
    assert over[:, 0].max() > 1 and np.array(d["knot_values"])[off[0]:off[1], 0].max() == 1, over[:, 0]       # Catmull-Rom overshoot above every knot
    assert over[:, 14].max() > 1                                                                                # .. and its to_linear
    low = over[:, 1] <= F(0.04045)                                                                              # both to_linear branches, the threshold itself and a negative channel
    assert low.sum() >= 6 and (over[:, 1] == F(0.04045)).any() and (over[:, 1] < 0).any() and (over[:, 2] > F(0.04045)).all()
    assert np.array_equal(over[low, 15], (over[low, 1] / F(12.92)).astype(F)) and (over[:, 16] < over[:, 2]).all()
    un = mat_out[:, SH.EMISSIVE_UNKEYED_INTENSITY]
    assert (un[:, 9:12] != 0).all() and np.all(un[:, 12] == 0) and np.all(un[:, 17:20] == 0)                    # emissive keys, no intensity key: black
    z = mat_out[:, SH.INTENSITY_ENDS_AT_ZERO]
    late = T >= F(SH.KNOTS[3][-1])
    assert late.sum() >= 2 and np.all(z[late, 12] == 0) and np.all(z[late, 17:20] == 0) and (z[~late, 17:20] > 0).all()
    assert late[SH.T_ZERO_EMISSION] and not late[SH.T_BETWEEN]
    opt, pose = lc[:, :3].sum(axis=1) > 0, lc[:, 3:].sum(axis=1) > 0
    for ty in range(3):
        of_type = d["light_types"] == ty
        assert (of_type & opt & ~pose).any() and (of_type & ~opt & pose).any() and (of_type & opt & pose).any(), ty
    init = d["light_init"]
    want_r = (init[:, :3] * init[:, 3:4]).astype(F)
    assert np.array_equal(light_out[:, ~opt, 6:9], np.broadcast_to(want_r[~opt], light_out[:, ~opt, 6:9].shape))   # set_time left the options alone
    assert np.array_equal(light_out[:, ~pose, 9:], np.broadcast_to(light_out[0, ~pose, 9:], light_out[:, ~pose, 9:].shape))
    assert np.isfinite(g["record_env_out"]).all() and len(set(map(tuple, g["record_env_out"]))) > 3


def check_render(d, g):
    T = SH.TIMES
    m, l = g["render_mat_out"], g["render_light_out"]
    assert list(d["mat_types"]) == [SH.LAMBERTIAN, SH.GLASS, SH.DIFFUSE_LIGHT] and list(d["light_types"]) == [SH.POINT, SH.SPOT, SH.DIRECTIONAL]
    assert np.all(m[SH.T_ZERO_EMISSION, 2, 17:20] == 0) and (m[SH.T_BETWEEN, 2, 17:20] > 0).all()               # the area light goes black at 4.0
    assert (m[:, 0, 14:17] > 0).all() and (m[:, 0, 14:17] < 1).all() and (m[:, 1, 13] > 1.1).all()
    opt, pose = SH.keyed(g, "render")
    assert list(opt) == [True, True, False] and list(pose) == [False, True, True]
    assert np.isfinite(l[:, 1:, 9:]).all() and (l[:, 1, 4] < l[:, 1, 5]).all()
    assert T[SH.T_BETWEEN] == F(0.9) and T[SH.T_ZERO_EMISSION] == F(4.0)


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "integration", "_build", "libdropin_pt_full.so"))
    out = {"times": SH.TIMES}
    for group, check in (("record", check_record), ("render", check_render)):
        d, rec = record(lib, group)
        out.update(rec)
        check(d, out)
    path = os.path.join(HERE, "anim_shading.npz")
    np.savez_compressed(path, **out)
    print("materials", len(out["record_mat_types"]), "lights", len(out["record_light_types"]), "knots", len(out["record_knot_times"]), "times", len(SH.TIMES),
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
