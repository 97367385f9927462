"""CPU: srt_pt_emitter - Scene_Particles::step for a pool of fixed capacity - as far as a host reaches: the ABI and the contract in the
header, the schedule (csrc/pt_emitter.h through the library on a host-only context and through the g++ emulation) against the
substep and spawn counts the reference recorded (tests/golden/emitter_*.npz, made by tests/golden/make_emitter_golden.py), the spawn
arithmetic against the recorded velocities bit for bit, the seeded uniforms, and every refusal.  Comparisons of floats are on their
bits; there are no tolerances."""
import ctypes
import os

import numpy as np
import pytest

import _emitter_cases as EC
import _harness as H
import _instance_cases as IC
import _light_cases as LC
import _repose_refit_cases as C

F = np.float32
INVALID, UNSUPPORTED, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def host_pt(srt, scene, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(-1)
    pt.set_params(32, 24, 1, 4, use_bvh)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    return pt


@pytest.fixture(scope="module")
def contexts(srt):
    """Host-only contexts of the small case: (render, collide, the pool's objects)."""
    S, pool = EC.pool("cbox_particles")
    render, collide = host_pt(srt, S), host_pt(srt, EC.collide_scene())
    yield render, collide, pool
    render.close(); collide.close()


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    names = ("srt_pt_emitter_create", "srt_pt_emitter_destroy", "srt_pt_emitter_set_options", "srt_pt_emitter_set_pose", "srt_pt_emitter_seed",
             "srt_pt_emitter_set_uniforms_device", "srt_pt_emitter_step_device", "srt_pt_emitter_step", "srt_pt_emitter_present_device",
             "srt_pt_emitter_frame_device", "srt_pt_emitter_clear_device", "srt_pt_emitter_clear", "srt_pt_emitter_read", "srt_pt_emitter_write",
             "srt_pt_emitter_counts", "srt_pt_emitter_arrays_device")
    text = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for name in names:
        assert getattr(lib, name) is not None and name + "(" in text, name
    for phrase in ("4096 substeps", "1048576 spawns", "k-th dead slot in ascending slot index", "dropped and counted", "a double minus a float",
                   "sorted by `birth`", "collide == render", "emitter key is objects[0]", "gui/simulate.cpp:69-99"):
        assert phrase in text, phrase
    assert "Spawning and removing particles stay with the caller" not in text and "torch op of its own" not in text
    assert "srt_pt_emitter_advance_host(" in open(os.path.join(H.ROOT, "include", "srt_pt_debug.h")).read()
    header = open(os.path.join(H.ROOT, "soft-rendering-toolsets_amd", "csrc", "pt_emitter.h")).read()
    assert f"kEmitterMaxSubsteps = {EC.MAX_SUBSTEPS}" in header and "kEmitterMaxSpawns = 1u << 20" in header and EC.MAX_SPAWNS == 1 << 20
    methods = ("set_options", "set_pose", "seed", "set_uniforms_device", "step_device", "step", "present_device", "frame_device", "clear", "read", "write",
               "counts", "close")
    for cls in (srt.Emitter, srt.EmitterGroup):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(srt.Emitter.clear_device) and callable(srt.Emitter.arrays_device) and callable(srt.Emitter.advance_host)
    assert callable(srt.Pathtracer.create_emitter) and callable(srt.PathtracerGroup.create_emitter)


@pytest.mark.parametrize("name", EC.CASES)
def test_fixture_holds_the_cases(name):
    """What make_emitter_golden.py asserted when it recorded, checked again on the committed file; and the file is the case's."""
    g, case = EC.load(name), EC.cases()[name]
    dts, options, poses = case["frames"]
    assert EC.bits_equal(g["dts"], dts) and EC.bits_equal(g["options"], options) and EC.bits_equal(g["pose"], poses)
    assert int(g["capacity"]) == case["capacity"] and str(g["pool"]) == case["pool"] and F(g["radius"]) == EC.RADIUS
    n = len(dts)
    assert g["particles"].shape == (n, case["record"], 7) and np.isfinite(g["particles"]).all() and g["count"].max() <= min(case["capacity"], case["record"])
    assert 2 * int(g["spawns"].sum()) == g["uniforms"].size and np.all((g["uniforms"] >= 0) & (g["uniforms"] < 1))
    deaths = reuse = bounces = 0
    for f in range(n):
        c = int(g["count"][f])
        assert np.all(np.diff(g["particles"][f, :c, 6]) >= 0) and np.all(np.diff(g["birth"][f, :c].astype(np.int64)) > 0)
        if f == 0 or not g["options"][f][6]:
            continue
        a, b = g["birth"][f - 1, :g["count"][f - 1]], g["birth"][f, :c]
        gone = np.setdiff1d(a, b)
        deaths += len(gone)
        reuse += bool(len(gone) and g["spawns"][f])
        _, ia, ib = np.intersect1d(a, b, return_indices=True)
        va, vb = g["particles"][f - 1, ia, 3:6], g["particles"][f, ib, 3:6]
        bounces += int(np.sum((np.abs(va[:, 0] - vb[:, 0]) > 1e-6) | (np.abs(va[:, 2] - vb[:, 2]) > 1e-6)))
    assert deaths >= 1 and reuse >= 1 and bounces >= 1
    if name == "small":
        en, odt = g["options"][:, 6] != 0, g["options"][:, 5]
        assert np.any((g["substeps"] == 0) & en & (odt >= 1e-5)) and np.any(g["substeps"] >= 3) and np.any(odt < 1e-5)
        assert np.any(~en) and np.any(en[1:] & ~en[:-1]) and case["capacity"] % 64 != 0
        assert np.any((g["pose"][:, 3:] != 0).all(axis=1) & (g["options"][:, 1] > 0))
    else:
        assert g["count"].max() > 256 and g["substeps"].sum() >= 40 and g["count"].max() <= 1200


@pytest.mark.parametrize("name", EC.CASES)
def test_schedule_equals_the_reference(contexts, name):
    """Substeps and spawns per frame, last_update and particle_cooldown after every frame: the library's schedule on a host-only context
    and the emulation's against the recorded ones.  The birth ordinals advance with the spawns."""
    render, collide, pool = contexts
    g = EC.load(name)
    em = render.create_emitter(collide, pool, float(g["radius"]))
    born = 0
    for f in range(len(g["dts"])):
        EC.set_frame(em, g, f)
        spawns, cleared, (last, cooldown) = em.advance_host(float(g["dts"][f]))
        assert cleared == (not g["options"][f][6])
        assert len(spawns) == g["substeps"][f] and int(spawns.sum()) == g["spawns"][f], f"frame {f}"
        assert F(last) == F(g["schedule"][f][0]) and cooldown == g["schedule"][f][1], f"frame {f}"
        born += int(spawns.sum())
        assert em.counts() == {"alive": 0, "born": born, "dropped": 0}
    em.close()
    sub, sp, st = EC.emu_schedule(g["options"], g["dts"])
    assert np.array_equal(sub, g["substeps"]) and np.array_equal(sp, g["spawns"]) and not st.any()


@pytest.mark.parametrize("name", EC.CASES)
def test_spawn_arithmetic_equals_the_reference(name):
    """Every particle in the frame it was born in and not yet stepped since - the spawns of the frame's last substep, whose age is still
    the lifetime - has the velocity the emulation of pt_emitter.h gives for its two recorded uniforms, bit for bit, and sits at the pose."""
    g = EC.load(name)
    checked = 0
    for f in range(len(g["dts"])):
        c = int(g["count"][f])
        fresh = np.flatnonzero(g["particles"][f, :c, 6] == g["options"][f][3])
        if not len(fresh) or not g["substeps"][f]:
            continue
        b = g["birth"][f, fresh]
        want = g["particles"][f, fresh]
        got = EC.emu_velocities(g["options"][f], g["pose"][f], g["uniforms"][b])
        assert EC.bits_equal(got, want[:, 3:6]), f"frame {f}"
        assert EC.bits_equal(want[:, :3], np.tile(g["pose"][f][:3], (len(fresh), 1)))
        checked += len(fresh)
    assert checked >= (20 if name == "small" else 100)


def test_sincos_restatement_is_exact_on_the_spawn_range():
    """srt_sincosf2 over [0, 2 pi) - t = 2 PI_F u for every 16th of the 2^24 uniforms and the last 64 - against this host's cosf / sinf, the
    functions the reference's std::cos / std::sin called: equal bit for bit, so pt_emitter.h needs no restatement of its own."""
    u = np.concatenate([np.arange(0, 1 << 24, 16, dtype=np.uint32), np.arange((1 << 24) - 64, 1 << 24, dtype=np.uint32)]).astype(F) * F(1.0 / 16777216.0)
    t = (F(2) * F(np.pi)) * u
    assert t.dtype == F and 6.28 < t.max() < 6.2831856
    got, want = EC.emu_sincos(t), EC.emu_sincos(t, libm=True)
    assert EC.bits_equal(got[0], want[0]) and EC.bits_equal(got[1], want[1])
    half = (np.arange(0, 36000, dtype=F) * F(0.01) * (F(np.pi) / F(180.0))) / F(2.0)      # Radians(angle) / 2 for angles of 0 .. 360 degrees
    assert EC.bits_equal(EC.emu_sincos(half)[0], EC.emu_sincos(half, libm=True)[0])


def test_seeded_uniforms_are_srt_rng_v1():
    """emitter_uniforms restates pt_device.h's Rng: the same two draws for a few keys, in [0, 1), different per ordinal, key and seed."""
    for seed, key, first in ((0, 0, 0), (7, 8, 0), (0x123456789ABCDEF, 0xFFFFFFFF, 0xFFFFFFF0), (7, 9, 1000)):
        a, b = EC.emu_uniforms(seed, key, first, 12), EC.emu_uniforms(seed, key, first, 12, through_rng=True)
        assert EC.bits_equal(a, b) and np.all((a >= 0) & (a < 1)) and len(np.unique(a)) == 24
    assert not EC.bits_equal(EC.emu_uniforms(7, 8, 0, 4), EC.emu_uniforms(7, 9, 0, 4)) and not EC.bits_equal(EC.emu_uniforms(7, 8, 0, 4), EC.emu_uniforms(8, 8, 0, 4))
    assert EC.bits_equal(EC.emu_uniforms(7, 8, 3, 1), EC.emu_uniforms(7, 8, 0, 4)[3:])
    # the PCG32 XSH-RR output function on the first state, restated in Python integers
    seed, key, b = 7, 8, 3
    M = (1 << 64) - 1
    k = (key << 32) | b
    z = (seed + 0x9E3779B97F4A7C15 * (k + 1)) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    inc = ((k << 1) | 1) & M
    state = (z * 6364136223846793005 + inc) & M
    xs, rot = ((((state >> 18) ^ state) >> 27) & 0xFFFFFFFF), state >> 59
    v = ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF
    assert EC.emu_uniforms(seed, key, b, 1)[0, 0] == F(v >> 8) * F(1.0 / 16777216.0)


def test_host_only_context_validates_and_refuses_device_work(srt, contexts):
    render, collide, pool = contexts
    em = render.create_emitter(collide, pool, 1.0)
    em.set_options(enabled=True)
    em.set_pose([0, 1, 0], [0, 0, 0])
    em.seed(5)
    for call in (lambda: em.step_device(0.1), lambda: em.step(0.1), lambda: em.present_device(), lambda: em.frame_device(0.1), lambda: em.clear(),
                 lambda: em.clear_device(), lambda: em.read(), lambda: em.write(alive=np.zeros(60, np.uint8)), lambda: em.arrays_device()):
        with pytest.raises(srt.SrtError, match="host-only") as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert em.counts() == {"alive": 0, "born": 0, "dropped": 0}       # the refused steps did not advance the schedule
    spawns, cleared, _ = em.advance_host(0.25)                        # defaults: opt.dt 0.01, pps 5
    assert len(spawns) == 24 and int(spawns.sum()) == 2 and not cleared
    # a commit on the render context leaves the handle stale
    S, _ = EC.pool("cbox_particles")
    render.build_scene(S)
    with pytest.raises(srt.SrtError, match="stale") as e:
        em.advance_host(0.1)
    assert e.value.status == STATE
    em.close()


def scene_state(pt, nobj):
    return IC.all_dumps(pt, nobj), pt.active(), pt.scene_counts()


def test_refusals_leave_the_scene_unchanged(srt, contexts):
    """What srt_pt_set_active refuses, with its codes: a duplicate, an index out of range, an emissive object; a list scene and a scene of
    one object; and NULL arguments, an empty pool, a short uniform buffer, the substep and spawn bounds.  Nothing changes."""
    render, collide, pool = contexts
    S, _ = EC.pool("cbox_particles")
    nobj = len(S["objects"])
    before = scene_state(render, nobj)
    for match, bad in (("listed twice", [9, 9]), ("out of range", [nobj, 9]), ("area light", [9, 7])):
        with pytest.raises(srt.SrtError, match=match) as e:
            render.create_emitter(collide, bad, 1.0)
        assert e.value.status == INVALID and "srt_pt_emitter_create:" in str(e.value)
    lib = srt.load_library()
    h, idx = ctypes.c_void_p(), np.array([9, 10], np.uint32)
    for args in ((None, collide._ctx, H.P(idx), 2), (render._ctx, None, H.P(idx), 2), (render._ctx, collide._ctx, None, 2), (render._ctx, collide._ctx, H.P(idx), 0)):
        assert lib.srt_pt_emitter_create(args[0], args[1], args[2], args[3], ctypes.c_float(1.0), ctypes.byref(h)) == INVALID and not h
    assert lib.srt_pt_emitter_create(render._ctx, collide._ctx, H.P(idx), 2, ctypes.c_float(1.0), None) == INVALID
    empty = srt.Pathtracer(-1)
    with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
        render.create_emitter(empty, pool, 1.0)
    assert e.value.status == STATE
    empty.close()
    lst = host_pt(srt, IC.sweeps_scene(), use_bvh=False)
    with pytest.raises(srt.SrtError, match="without BVHs") as e:
        lst.create_emitter(collide, [3], 1.0)
    assert e.value.status == UNSUPPORTED
    lst.close()
    one = host_pt(srt, C.one_object_scene())
    with pytest.raises(srt.SrtError, match="root of the BVH<Object> is a leaf") as e:
        one.create_emitter(collide, [0], 1.0)
    assert e.value.status == UNSUPPORTED
    one.close()
    lit = host_pt(srt, LC.three_light_scene(), dynamic=True)
    with pytest.raises(srt.SrtError, match="area light") as e:
        lit.create_emitter(lit, [3, LC.CBOX_LIGHT], 1.0)
    assert e.value.status == INVALID
    lit.close()
    # refusals of a step: the schedule stays
    em = render.create_emitter(collide, pool, 1.0)
    em.set_options(pps=500.0, dt=0.01, enabled=True)
    em.set_uniforms_device(0x1000, 2 * 9)                             # (a host-only context keeps the pointer and never reads it)
    with pytest.raises(srt.SrtError, match="uniform buffer is too short") as e:
        em.advance_host(0.025)                                        # 2 substeps, 10 spawns
    assert e.value.status == INVALID
    em.set_uniforms_device(0x1000, 2 * 10)
    spawns, _, _ = em.advance_host(0.025)
    assert list(spawns) == [5, 5]
    em.set_uniforms_device(0, 0)
    with pytest.raises(srt.SrtError, match="substeps") as e:
        em.advance_host(0.01 * (EC.MAX_SUBSTEPS + 2))
    assert e.value.status == UNSUPPORTED
    em.set_options(pps=1e9, dt=0.01, enabled=True)
    with pytest.raises(srt.SrtError, match="spawns in one substep") as e:
        em.advance_host(0.011)
    assert e.value.status == UNSUPPORTED
    em.set_options(pps=500.0, dt=0.01, enabled=True)
    spawns, _, _ = em.advance_host(0.02)                              # 0.005 left over + 0.02: the schedule is where the last good step left it
    assert list(spawns) == [5, 5] and em.counts()["born"] == 20
    with pytest.raises(srt.SrtError, match="NULL argument"):
        em._check(lib, lib.srt_pt_emitter_set_pose(em._h, None, None))
    assert lib.srt_pt_emitter_counts(None, None) == INVALID and lib.srt_pt_emitter_step(None, ctypes.c_float(0.1)) == INVALID
    em.close()
    after = scene_state(render, nobj)
    assert IC.dumps_equal(after[0], before[0]) and np.array_equal(after[1], before[1]) and after[2] == before[2]


@pytest.mark.ref
@pytest.mark.skipif(not os.path.exists(os.path.join(H.ROOT, "integration", "_build", "libdropin_pt_full.so")) or not os.path.isdir("/root/reference"),
                    reason="integration/_build not built (needs /root/reference)")
@pytest.mark.parametrize("name", EC.CASES)
def test_fixture_is_what_the_reference_computes(name):
    """The harness run again: the committed file's recordings, bit for bit."""
    import sys

    sys.path.insert(0, H.GOLDEN)
    import make_emitter_golden as M

    lib = ctypes.CDLL(os.path.join(H.ROOT, "integration", "_build", "libdropin_pt_full.so"))
    g, case = EC.load(name), EC.cases()[name]
    r = M.run_reference(lib, case)
    assert EC.bits_equal(r["particles"], g["particles"]) and EC.bits_equal(r["uniforms"], g["uniforms"])
    assert np.array_equal(r["count"], g["count"]) and np.array_equal(r["substeps"], g["substeps"]) and np.array_equal(r["spawns"], g["spawns"])
    assert np.array_equal(r["schedule"], g["schedule"]) and np.array_equal(M.number_births(case, r), g["birth"])
