"""CPU: new shading values for a committed scene on the host side - srt_pt_update_materials / srt_pt_update_lights /
srt_pt_update_env_light and the shading timelines' host form (srt_pt_shading_timeline_values / _update) through the ABI on a
host-only context, against what the reference recorded (tests/golden/anim_shading.npz) and against fresh commits, bit for bit; the
item functions of pt_anim.h through their host emulation (tests/host_emu/shading_host.cpp); every refusal, each with the scene left as
it was; and the emulation as a sanitized stand-alone program.  Every comparison is on float32 viewed as uint32, NaN matching NaN; there
are no tolerances."""
import ctypes
import subprocess

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _instance_cases as IC
import _shading_cases as SH

F = np.float32
INVALID, UNSUPPORTED, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def g():
    return SH.load()


@pytest.fixture(scope="module")
def record(g):
    return SH.record_scene(g)


def last_error(srt):
    return srt.load_library().srt_last_error().decode("utf-8", "replace")


def host_pt(srt, scene):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 4, True)
    pt.build_scene(scene)
    return pt


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    names = ("srt_pt_update_materials", "srt_pt_update_lights", "srt_pt_update_env_light", "srt_pt_shading_timeline_create", "srt_pt_shading_timeline_destroy",
             "srt_pt_shading_timeline_values", "srt_pt_shading_timeline_update", "srt_pt_shading_timeline_apply")
    text = open(H.ROOT + "/include/srt_pt.h").read()
    for name in names:
        assert getattr(lib, name) is not None and name + "(" in text, name
    assert lib.srt_pt_dump_shading is not None and "srt_pt_dump_shading(" in open(H.ROOT + "/include/srt_pt_debug.h").read()
    for ref in ("scene/object.cpp:71", "scene/material.cpp:44-52", "scene/light.cpp:30-38", "lib/spectrum.h:54-60", "rays/pathtracer.cpp:26-64,93-117"):
        assert ref in text, ref
    for cls, methods in ((srt.Pathtracer, ("update_materials", "update_lights", "update_env_light", "dump_shading", "create_shading_timeline")),
                         (srt.ShadingTimeline, ("values", "update", "apply", "close")), (srt.ShadingTimelineGroup, ("values", "update", "apply", "close")),
                         (srt.PathtracerGroup, ("update_materials", "update_lights", "update_env_light", "dump_shading", "create_shading_timeline"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)


def test_fixture_holds_the_cases(g):
    """What make_shading_golden.py asserted when it recorded, checked again on the committed file."""
    assert np.array_equal(g["times"], SH.TIMES)
    for group in SH.GROUPS:
        d = SH.describe(group)
        assert np.array_equal(d["track_offsets"], g[group + "_track_offsets"]) and np.array_equal(d["mat_types"], g[group + "_mat_types"])
        assert AC.bits_equal(d["knot_times"], g[group + "_knot_times"]) and AC.bits_equal(d["knot_values"], g[group + "_knot_values"])
        assert np.array_equal(d["light_types"], g[group + "_light_types"])
    off = g["record_track_offsets"].astype(np.int64)
    nm, nl = len(g["record_mat_types"]), len(g["record_light_types"])
    assert set(g["record_mat_types"]) == {0, 1, 2, 3, 4} and nl == 300 and (nm + nl) > 4 * 64 + 1
    counts = np.diff(off)
    mc, lc = counts[:6 * nm].reshape(nm, 6), counts[6 * nm:6 * nm + 6 * nl].reshape(nl, 6)
    assert all(set(mc[:, i]) >= {0, 1, 2, 3, 6} and set(lc[:, i]) >= {0, 1, 2, 3, 6} for i in range(6))
    m = g["record_mat_out"]
    over = m[:, SH.OVERSHOOT]
    assert over[:, 0].max() > 1 and (over[:, 1] <= F(0.04045)).sum() >= 6 and (over[:, 1] == F(0.04045)).any() and (over[:, 1] < 0).any() and (over[:, 2] > F(0.04045)).all()
    assert np.all(m[:, SH.EMISSIVE_UNKEYED_INTENSITY, 17:20] == 0) and (m[:, SH.EMISSIVE_UNKEYED_INTENSITY, 9:12] != 0).all()
    late = SH.TIMES >= F(SH.KNOTS[3][-1])
    assert late.sum() >= 2 and np.all(m[late, SH.INTENSITY_ENDS_AT_ZERO, 17:20] == 0) and (m[~late, SH.INTENSITY_ENDS_AT_ZERO, 17:20] > 0).all()
    opt, pose = SH.keyed(g, "record")
    for ty in range(3):
        of = g["record_light_types"] == ty
        assert (of & opt & ~pose).any() and (of & ~opt & pose).any() and (of & opt & pose).any()
    assert np.all(g["render_mat_out"][SH.T_ZERO_EMISSION, 2, 17:20] == 0) and (g["render_mat_out"][SH.T_BETWEEN, 2, 17:20] > 0).all()


def test_values_equal_the_reference(srt, g, record):
    """All 20 materials, 300 lights and the environment at every recorded time, through srt_pt_shading_timeline_values on a host-only context;
    materials also as stored records: the Lambertian / PI_F."""
    scene, mats, lights = record
    pt = host_pt(srt, scene)
    tl = pt.create_shading_timeline(mats, lights, True, SH.tracks(g, "record"))
    bad = {}
    for i, t in enumerate(g["times"]):
        v = tl.values(t)
        want_m, want_l = SH.material_values(g, "record", i), SH.light_values(g, "record", i, scene["lights"])
        assert np.array_equal(v["materials"]["type"], want_m["type"])
        bad[float(t)] = (sum(AC.mismatches(v["materials"][f], want_m[f]) for f in ("a", "b", "ior")), AC.mismatches(v["lights"], want_l),
                         AC.mismatches(v["env"], g["record_env_out"][i]))
        tl.update(t)
        d = pt.dump_shading()
        bad[float(t)] += (AC.mismatches(d["materials"]["a"][mats], SH.stored(want_m)["a"]), AC.mismatches(d["lights"][:, :21], want_l),
                          AC.mismatches(d["env_radiance"], g["record_env_out"][i]))
    tl.close()
    pt.close()
    assert not any(any(b) for b in bad.values()), bad


@pytest.mark.parametrize("ti", [0, SH.T_BETWEEN, SH.T_ZERO_EMISSION])
def test_updates_equal_a_fresh_commit(srt, g, record, ti):
    """update_materials / update_lights / update_env_light with explicit values, and ShadingTimeline.update(t): dump_shading of the host's
    record equals the dump of a fresh commit made with those values, itrans and has_trans included; no tree moves."""
    scene, mats, lights = record
    want_m, want_l, env = SH.material_values(g, "record", ti), SH.light_values(g, "record", ti, scene["lights"]), g["record_env_out"][ti]
    fresh = host_pt(srt, SH.with_values(scene, mats, want_m, lights, want_l, env))
    want, nobj = fresh.dump_shading(), len(scene["objects"])
    trees = IC.all_dumps(fresh, nobj)
    fresh.close()
    pt = host_pt(srt, scene)
    before = pt.dump_shading()
    assert not SH.dumps_equal(before, want)
    pt.update_materials(mats, want_m)
    pt.update_lights(lights, want_l[:, :3], want_l[:, 3:5], want_l[:, 5:])
    pt.update_env_light(env)
    assert SH.dumps_equal(pt.dump_shading(), want) and IC.dumps_equal(IC.all_dumps(pt, nobj), trees)
    assert pt.scene_counts()["uploaded_bytes"] == 0                                   # a host-only context uploads nothing
    pt.close()
    pt = host_pt(srt, scene)
    tl = pt.create_shading_timeline(mats, lights, True, SH.tracks(g, "record"))
    tl.update(g["times"][ti])
    assert SH.dumps_equal(pt.dump_shading(), want) and IC.dumps_equal(IC.all_dumps(pt, nobj), trees)
    tl.close()
    pt.close()


def test_emulation_equals_the_reference(g):
    """The item functions of pt_anim.h compiled with g++ -ffp-contract=off: the six options, the values, the stored Lambertian albedo,
    the lights' keyed triples and the environment."""
    bad = {}
    for group in SH.GROUPS:
        opt, pose = SH.keyed(g, group)
        for i, t in enumerate(g["times"]):
            mats, stored_a, options, lights, flags, env = SH.emu_values(g, group, t)
            want_m, rows = SH.material_values(g, group, i), g[group + "_light_out"][i]
            assert np.array_equal(flags[:, 0] != 0, opt) and np.array_equal(flags[:, 1] != 0, pose)
            bad[group, float(t)] = (AC.mismatches(options, g[group + "_mat_out"][i][:, :14]), AC.mismatches(mats[:, :3], want_m["a"]), AC.mismatches(mats[:, 3:6], want_m["b"]),
                                    AC.mismatches(mats[:, 6], want_m["ior"]), AC.mismatches(stored_a, SH.stored(want_m)["a"]),
                                    AC.mismatches(lights[opt, :3], rows[opt, 6:9]), AC.mismatches(lights[opt, 3:5], rows[opt, 4:6]), AC.mismatches(lights[pose, 5:], rows[pose, 9:]),
                                    AC.mismatches(env, g[group + "_env_out"][i]) if group == "record" else 0)
    assert not any(any(b) for b in bad.values()), {k: v for k, v in bad.items() if any(v)}


def _state(pt, nobj):
    return pt.dump_shading(), IC.all_dumps(pt, nobj), pt.scene_counts()


def _same_state(a, b):
    return SH.dumps_equal(a[0], b[0]) and IC.dumps_equal(a[1], b[1]) and a[2] == b[2]


def test_update_refusals_leave_the_scene_alone(srt, g, record):
    scene, mats, lights = record
    lib, nobj = srt.load_library(), len(scene["objects"])
    pt = host_pt(srt, scene)
    before = _state(pt, nobj)
    nmat, two = len(scene["materials"]), np.array([mats[0], mats[1]], np.uint32)
    recs = SH.material_values(g, "record", 3)[:2].copy()
    rad, ab, T = np.ones((2, 3), F), np.array([[10, 20], [30, 40]], F), np.tile(np.eye(4, dtype=F).reshape(16), (2, 1))
    null = ctypes.c_void_p()

    def um(idx=two, m=recs, n=2, ctx=None):
        return lib.srt_pt_update_materials(pt._ctx if ctx is None else ctx, None if idx is None else H.P(idx), None if m is None else H.P(m), n)

    def ul(idx=np.array([0, 1], np.uint32), rad=rad, ab=ab, T=T, n=2, ctx=None):
        return lib.srt_pt_update_lights(pt._ctx if ctx is None else ctx, None if idx is None else H.P(idx), None if rad is None else H.P(rad), None if ab is None else H.P(ab),
                                        None if T is None else H.P(T), n)

    assert um(ctx=null) == INVALID and um(idx=None) == INVALID and um(m=None) == INVALID
    assert um(idx=np.array([mats[0], nmat], np.uint32)) == INVALID and "out of range" in last_error(srt)
    assert um(idx=np.array([mats[0], mats[0]], np.uint32)) == INVALID and "twice" in last_error(srt)
    wrong = recs.copy()
    wrong[1]["type"] = (int(wrong[1]["type"]) + 1) % 5
    assert um(m=wrong) == INVALID
    msg = last_error(srt)
    names = ("Lambertian", "Mirror", "Glass", "Diffuse Light", "Refract")
    assert names[int(recs[1]["type"])] in msg and names[int(wrong[1]["type"])] in msg, msg
    wrong[1]["type"] = 9
    assert um(m=wrong) == INVALID
    assert ul(ctx=null) == INVALID and ul(idx=None) == INVALID and ul(rad=None) == INVALID and ul(T=None) == INVALID
    assert ul(idx=np.array([0, SH.NLIGHTS], np.uint32)) == INVALID and ul(idx=np.array([3, 3], np.uint32)) == INVALID
    spot = int(np.nonzero(g["record_light_types"] == SH.SPOT)[0][0])
    assert ul(idx=np.array([0, spot], np.uint32), ab=None) == INVALID and "spot" in last_error(srt)
    assert lib.srt_pt_update_env_light(null, H.P(rad)) == INVALID and lib.srt_pt_update_env_light(pt._ctx, None) == INVALID
    assert _same_state(_state(pt, nobj), before)
    assert um() == 0 and ul() == 0 and um(n=0, idx=None, m=None) == 0                                     # (and the valid forms are taken)
    pt.close()
    # no environment light, or an environment map: no radiance to replace
    import _cases

    plain = host_pt(srt, _cases.pt_scene("cbox"))
    assert lib.srt_pt_update_env_light(plain._ctx, H.P(rad)) == INVALID and "without an environment light" in last_error(srt)
    plain.close()
    mapped = host_pt(srt, _cases.pt_scene("cbox_envmap"))
    assert lib.srt_pt_update_env_light(mapped._ctx, H.P(rad)) == INVALID and "map" in last_error(srt)
    mapped.close()
    # no committed scene
    empty = srt.Pathtracer(device=-1)
    assert um(ctx=empty._ctx) == STATE and ul(ctx=empty._ctx) == STATE and lib.srt_pt_update_env_light(empty._ctx, H.P(rad)) == STATE
    counts = np.zeros(2, np.uint32)
    assert lib.srt_pt_dump_shading(empty._ctx, 0, H.P(counts), None, 0, None, None, 0, None, None) == STATE
    empty.close()


def test_timeline_refusals_leave_the_scene_alone(srt, g, record):
    """Every refusal of srt_pt_shading_timeline_create, the stale timeline, the device form on a host-only context."""
    scene, mats, lights = record
    lib, nobj = srt.load_library(), len(scene["objects"])
    pt = host_pt(srt, scene)
    before = _state(pt, nobj)
    m1, l1 = np.array([mats[0]], np.uint32), np.array([5], np.uint32)
    # one material (albedo 2 knots, intensity 1), one light (spectrum 1; position 2), the environment (intensity 1)
    off = np.array([0, 2, 2, 2, 2, 3, 3, 4, 4, 4, 6, 6, 6, 6, 7], np.uint32)
    times, values = np.array([0.0, 1.0, 0.0, 0.5, 0.0, 2.0, 1.0], F), np.ones((7, 4), F)
    h, null = ctypes.c_void_p(), ctypes.c_void_p()

    def create(ms=m1, nm=1, ls=l1, nl=1, env=1, off=off, times=times, values=values, ctx=None, out=h):
        return lib.srt_pt_shading_timeline_create(pt._ctx if ctx is None else ctx, None if ms is None else H.P(ms), nm, None if ls is None else H.P(ls), nl, env,
                                                  None if off is None else H.P(off), None if times is None else H.P(times), None if values is None else H.P(values),
                                                  None if out is None else ctypes.byref(out))

    assert create(ctx=null) == INVALID and create(ms=None) == INVALID and create(ls=None) == INVALID and create(off=None) == INVALID
    assert create(times=None) == INVALID and create(values=None) == INVALID and create(out=None) == INVALID
    assert create(ms=np.array([len(scene["materials"])], np.uint32)) == INVALID and create(ls=np.array([SH.NLIGHTS], np.uint32)) == INVALID
    assert create(ms=np.array([mats[0], mats[0]], np.uint32), nm=2, ls=None, nl=0, env=0, off=np.array([0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2], np.uint32)) == INVALID
    assert "twice" in last_error(srt)
    assert create(ms=None, nm=0, ls=None, nl=0, env=0, off=np.zeros(1, np.uint32)) == INVALID and "nothing" in last_error(srt)
    for bad_times in ([0.0, 0.0, 0.0, 0.5, 0.0, 2.0, 1.0], [1.0, 0.0, 0.0, 0.5, 0.0, 2.0, 1.0], [0.0, np.nan, 0.0, 0.5, 0.0, 2.0, 1.0], [0.0, np.inf, 0.0, 0.5, 0.0, 2.0, 1.0]):
        assert create(times=np.array(bad_times, F)) == INVALID, bad_times
    first = off.copy(); first[0] = 1
    down = off.copy(); down[1], down[2] = 3, 2
    assert create(off=first) == INVALID and create(off=down) == INVALID
    for none, what in (([0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2], "material"), ([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2], "light"),
                       ([0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2], "environment")):                                    # an item without any key
        assert create(off=np.array(none, np.uint32)) == INVALID and "any()" in last_error(srt) and what in last_error(srt), what
    assert not h.value
    plain_scene = dict(scene)
    del plain_scene["env"]
    plain = host_pt(srt, plain_scene)
    assert create(ctx=plain._ctx) == INVALID and "environment" in last_error(srt)                          # env keys without an environment light
    plain.close()
    assert _same_state(_state(pt, nobj), before)
    # a valid one: the device form is refused after validation, the host forms work; NaN knot VALUES are not checked
    values[1] = np.nan
    assert create() == 0 and h.value
    tl = srt.ShadingTimeline(pt, h, m1, l1, True)
    assert lib.srt_pt_shading_timeline_apply(tl._h, None, 0.5) == UNSUPPORTED and "host-only" in last_error(srt)
    assert lib.srt_pt_shading_timeline_apply(None, None, 0.5) == INVALID and lib.srt_pt_shading_timeline_update(None, 0.5) == INVALID
    out_m, out_l, out_e = np.zeros(1, srt.MATERIAL_DTYPE), np.zeros(21, F), np.zeros(3, F)
    assert lib.srt_pt_shading_timeline_values(None, 0.5, H.P(out_m), H.P(out_l), H.P(out_e)) == INVALID
    assert lib.srt_pt_shading_timeline_values(tl._h, 0.5, None, H.P(out_l), H.P(out_e)) == INVALID
    assert lib.srt_pt_shading_timeline_values(tl._h, 0.5, H.P(out_m), None, H.P(out_e)) == INVALID
    assert lib.srt_pt_shading_timeline_values(tl._h, 0.5, H.P(out_m), H.P(out_l), None) == INVALID
    assert _same_state(_state(pt, nobj), before)
    v = tl.values(0.5)
    assert np.isnan(v["materials"]["a"]).all() and np.all(v["lights"][0, :5] == 0)     # a spectrum key without an intensity key: T() = 0.0f, a black light
    # stale: the scene was committed again
    pt.build_scene(scene)
    assert lib.srt_pt_shading_timeline_values(tl._h, 0.5, H.P(out_m), H.P(out_l), H.P(out_e)) == STATE and "stale" in last_error(srt)
    assert lib.srt_pt_shading_timeline_update(tl._h, 0.5) == STATE and lib.srt_pt_shading_timeline_apply(tl._h, None, 0.5) == STATE
    assert _same_state(_state(pt, nobj)[:2] + (0,), before[:2] + (0,))
    tl.close()
    assert lib.srt_pt_shading_timeline_destroy(None) == 0
    fresh = srt.Pathtracer(device=-1)
    assert create(ctx=fresh._ctx) == STATE
    fresh.close()
    pt.close()


def test_closing_the_context_closes_its_timelines(srt, g, record):
    scene, mats, lights = record
    pt = host_pt(srt, scene)
    a = pt.create_shading_timeline(mats, lights, True, SH.tracks(g, "record"))
    b = pt.create_shading_timeline([mats[0]], [], False, [((0.0, 1.0), np.zeros((2, 3))), None, None, None, ((0.5,), [2.0]), None])   # the bindings' per-track form
    a.close()
    assert not a._h and b._h
    pt.close()
    assert not b._h
    b.close(); a.close()


def _flat_file(path, g, group):
    off, kt, kv = SH.tracks(g, group)
    types = np.ascontiguousarray(g[group + "_mat_types"], np.uint32)
    nm, nl, env = len(types), len(g[group + "_light_types"]), int(group == "record")
    opt, pose = SH.keyed(g, group)
    with open(path, "wb") as f:
        np.array([nm, nl, env, len(g["times"]), len(kt)], np.uint32).tofile(f)
        for a in (types, off, kt, kv, np.ascontiguousarray(g["times"], F)):
            a.tofile(f)
        for i in range(len(g["times"])):
            m, rows = SH.material_values(g, group, i), g[group + "_light_out"][i]
            np.concatenate([m["a"], m["b"], m["ior"][:, None]], axis=1).astype(F).tofile(f)
            np.ascontiguousarray(SH.stored(m)["a"], F).tofile(f)
            np.stack([opt, pose], axis=1).astype(np.uint32).tofile(f)
            np.concatenate([rows[:, 6:9], rows[:, 4:6], rows[:, 9:]], axis=1).astype(F).tofile(f)
            np.ascontiguousarray(g[group + "_env_out"][i], F).tofile(f)


@pytest.mark.parametrize("group", SH.GROUPS)
def test_sanitized_program(g, group, tmp_path):
    """-fsanitize=address,undefined over the evaluation of every recorded item, odd query times, non-finite albedo channels and the
    table check on malformed offsets and times.  A program of its own, run as its own process."""
    exe = SH.sanitized_program()
    path = str(tmp_path / "shading.bin")
    _flat_file(path, g, group)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "shading_sanitized: ok" in run.stdout and "ACCEPTED" not in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
