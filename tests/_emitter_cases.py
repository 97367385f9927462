"""Cases of the emitter tests (test_pt_emitter_host.py, test_pt_emitter_gpu.py, tests/golden/make_emitter_golden.py).

cases() is what make_emitter_golden.py runs through the reference's own Scene_Particles::step (integration/harness/emitter_ref.cpp)
and records as tests/golden/emitter_<name>.npz; the tests read everything back from the fixtures, so that what is replayed is what
was recorded.  Everything here is data.

Both cases collide with collide_scene(): pt_scene("cbox_particles") without its 60 particles - the Cornell box's five walls, two
spheres and light plus six small spheres, what Simulate::build_scene would hold.  Lifetimes stay constant inside a case and longer
than any frame, so that ages never decrease along the reference's vector and no particle is born and dies inside one frame: the
survivors of a frame are then the tail of the previous vector and the births its last entries, which is how the recorder numbers
the birth ordinals."""
import ctypes
import os

import numpy as np

import _harness as H
import _instance_cases as IC
import _repose_refit_cases as C

F = np.float32
CASES = ("small", "wide")
RADIUS = F(1.0)                 # Scene_Particles::radius of both cases (a unit mesh)
MAX_SUBSTEPS = 4096             # kEmitterMaxSubsteps
MAX_SPAWNS = 1 << 20            # kEmitterMaxSpawns


def _frames(rows):
    """rows of (frame dt, options7, pose6) -> (dts, options (n, 7), poses (n, 6))"""
    return np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], F), np.array([r[2] for r in rows], F)


def cases():
    # small: capacity 60 (the last wave is partial).  5 spawns per substep, 8 substeps of life: at most 45 alive.
    on = (12.0, 50.0, 0.03, 0.08, 500.0, 0.01, 1)
    pose_a, pose_b = (0.5, 0.6, 0.1, 20.0, 30.0, -75.0), (-0.4, 0.9, -0.2, -40.0, 110.0, 200.0)
    small = _frames([
        (0.035, on, pose_a),                                            # 3 substeps
        (0.004, on, pose_a),                                            # 0 substeps
        (0.05, on, pose_a),                                             # 5
        (0.045, on, pose_a),                                            # the first deaths, their slots reused in the same substep
        (0.03, on[:6] + (0,), pose_a),                                  # disabled: clear()
        (0.03, on, pose_b),                                             # enabled again, another pose
        (0.03, on[:5] + (1e-6, 1), pose_b),                             # opt.dt < EPS_F: nothing happens
        (0.06, (9.0, 80.0, 0.03, 0.08, 500.0, 0.01, 1), pose_b),
        (0.05, (9.0, 80.0, 0.03, 0.08, 500.0, 0.01, 1), pose_a),
    ])
    # wide: capacity 1200.  20 spawns per substep, 30 substeps of life, 40 substeps: births, deaths and reuse cross waves and workgroups.
    won = (6.0, 120.0, 0.02, 0.3, 2000.0, 0.01, 1)
    wide = _frames([(0.05, won, (0.0, 0.8, 0.0, 10.0, 0.0, 25.0))] * 8)
    return {"small": {"frames": small, "pool": "cbox_particles", "capacity": 60, "record": 60},
            "wide": {"frames": wide, "pool": "pool1200", "capacity": 1200, "record": 700}}


def collide_scene():
    base = IC.pt_scene("cbox_particles")
    out = dict(base)
    out["objects"] = [o for k, o in enumerate(base["objects"]) if not IC.PARTICLE_FIRST <= k < IC.PARTICLE_FIRST + IC.PARTICLE_COUNT]
    out["name"] = "cbox_particles without its particles"
    return out


def pool(name):
    """(render scene, the pool's objects): the 74-object particle scene with its 60 particle instances, or the pool of 1200 cubes."""
    if name == "cbox_particles":
        return IC.particles_shared()[0], C.particle_indices()
    assert name == "pool1200"
    S = C.pool_scene(1200)
    return S, np.arange(len(S["objects"]), dtype=np.uint32)


def load(name):
    return np.load(os.path.join(H.GOLDEN, f"emitter_{name}.npz"))


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def vector_of(pos, vel, age, alive, birth):
    """The reference's vector from a pool: the alive slots sorted by birth, (n, 7) = pos, velocity, age; and their ordinals."""
    slots = np.flatnonzero(alive)
    slots = slots[np.argsort(birth[slots], kind="stable")]
    return np.concatenate([pos[slots], vel[slots], age[slots, None]], axis=1).astype(F), birth[slots]


def set_frame(em, g, f):
    o = g["options"][f]
    em.set_options(*(float(v) for v in o[:6]), enabled=bool(o[6]))
    em.set_pose(g["pose"][f][:3], g["pose"][f][3:])


# ---- the host emulation of pt_emitter.h (tests/host_emu/emitter_host.cpp, g++ -ffp-contract=off) ----
_emu = None


def emitter_emu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(H.build_host_lib("emitter_host", ["emitter_host.cpp"], extra=("-lm",)))
    return _emu


def emu_velocities(options, pose, uniforms):
    """The spawn velocities of uniforms (n, 2) under one frame's options7 and pose6, from the emulation: (n, 3)."""
    u = np.ascontiguousarray(uniforms, F).reshape(-1, 2)
    o, p = np.ascontiguousarray(options, F), np.ascontiguousarray(pose, F)
    out = np.zeros((len(u), 3), F)
    emitter_emu().emitter_emu_velocities(H.P(o), H.P(p), H.P(u), len(u), H.P(out))
    return out


def emu_uniforms(seed, key, first, n, through_rng=False):
    """The uniforms of ordinals first .. first + n - 1 for (seed, key): (n, 2).  through_rng: drawn from pt_device.h's Rng instead of
    pt_emitter.h's restatement of it."""
    out = np.zeros((n, 2), F)
    emitter_emu().emitter_emu_uniforms(ctypes.c_uint64(seed), ctypes.c_uint32(key), ctypes.c_uint32(first), ctypes.c_uint32(n), int(through_rng), H.P(out))
    return out


def emu_sincos(x, libm=False):
    """(cos, sin) of float32 x by srt_sincosf2, or by the host's cosf / sinf."""
    x = np.ascontiguousarray(x, F)
    c, s = np.zeros_like(x), np.zeros_like(x)
    emitter_emu().emitter_emu_sincos(H.P(x), len(x), int(libm), H.P(c), H.P(s))
    return c, s


def emu_schedule(options, dts):
    """pt_emitter.h's emitter_plan_step over frames: (substeps per frame, spawns per frame, status per frame)."""
    o, d = np.ascontiguousarray(options, F), np.ascontiguousarray(dts, F)
    n = len(d)
    sub, sp, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    emitter_emu().emitter_emu_schedule(H.P(o), H.P(d), n, H.P(sub), H.P(sp), H.P(st))
    return sub, sp, st
