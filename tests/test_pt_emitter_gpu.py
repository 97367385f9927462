"""GPU: srt_pt_emitter - the whole Scene_Particles::step on the device.  The reference's recorded runs (tests/golden/emitter_*.npz)
replayed with their uniforms: after every frame the alive slots sorted by birth are the reference's vector bit for bit.  The slot
rule on hand-written pools against np.flatnonzero(alive == 0)[:k]; the masked step against srt_pt_particles_step on the compacted
arrays; the one-stream frame loop against the host forms; the seeded generator against the emulation; the group forwarder.
Everything is compared bit for bit; every test runs once."""
import numpy as np
import pytest

import _emitter_cases as EC
import _instance_cases as IC
import _repose_device_cases as RDC
from _active_cases import DEPTH, HT, SEED, W

pytestmark = pytest.mark.gpu

F = np.float32
STEP = 0.015                    # one substep of Options::dt = 0.01 from a fresh schedule


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make_pt(srt, scene):
    pt = srt.Pathtracer(0)
    pt.set_params(W, HT, 1, DEPTH, True)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


@pytest.fixture(scope="module")
def collide(srt):
    pt = make_pt(srt, EC.collide_scene())
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def renders(srt):
    """One render context per pool, made on first use: "cbox_particles" (its 60 particles and, for a capacity of 61, one sphere more) and
    "pool1200"."""
    made = {}

    def get(name):
        if name not in made:
            S, pool = EC.pool(name)
            made[name] = (make_pt(srt, S), pool, S)
        return made[name]

    yield get
    for pt, _, _ in made.values():
        pt.close()


def on_device(torch, a):
    d = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", EC.CASES)
def test_replay_equals_the_reference(torch, collide, renders, name):
    """Both recorded runs through step_device with the recorded uniforms: after every frame the alive slots sorted by birth equal the
    reference's vector - pos, velocity, age - bit for bit, with the recorder's ordinals; counts() agrees and nothing was dropped."""
    g = EC.load(name)
    pt, pool, _ = renders(str(g["pool"]))
    assert len(pool) == int(g["capacity"])
    em = pt.create_emitter(collide, pool, float(g["radius"]))
    d_u = on_device(torch, g["uniforms"].reshape(-1))
    em.set_uniforms_device(d_u.data_ptr(), d_u.numel())
    st = torch.cuda.Stream(device="cuda:0")
    born = 0
    for f in range(len(g["dts"])):
        EC.set_frame(em, g, f)
        em.step_device(float(g["dts"][f]), st.cuda_stream)
        p = em.read()
        vec, birth = EC.vector_of(p["pos"], p["vel"], p["age"], p["alive"], p["birth"])
        c = int(g["count"][f])
        born += int(g["spawns"][f])
        assert len(vec) == c, f"frame {f}: {len(vec)} alive, the reference has {c}"
        assert np.array_equal(birth, g["birth"][f, :c]), f"frame {f}"
        assert EC.bits_equal(vec, g["particles"][f, :c]), f"frame {f}: {int(np.sum(vec.view(np.uint32) != g['particles'][f, :c].view(np.uint32)))} words differ"
        assert em.counts() == {"alive": c, "born": born, "dropped": 0}
    if name == "wide":
        assert np.flatnonzero(p["alive"]).max() > 256
    em.close()


def hand_pool(n, alive, seed):
    """A pool of n slots: positions inside the box, velocities of about 1, ages far from death, ordinals 1000 + slot; the dead slots hold
    NaNs with the slot number as payload, so that a write to any of them shows."""
    rng = np.random.default_rng(seed)
    pos = ((rng.random((n, 3)) - 0.5) * [0.6, 0.6, 0.6] + [0.0, 0.6, 0.0]).astype(F)
    vel = ((rng.random((n, 3)) - 0.5) * 2.0).astype(F)
    age = np.full(n, 100.0, F)
    birth = (1000 + np.arange(n)).astype(np.uint32)
    alive = np.ascontiguousarray(alive, np.uint8)
    dead = np.flatnonzero(alive == 0)
    nan = (np.uint32(0x7fc00000) + dead.astype(np.uint32)).view(F)
    pos[dead], vel[dead], age[dead] = nan[:, None], nan[:, None], nan
    return {"pos": pos, "vel": vel, "age": age, "alive": alive, "birth": birth}


def spawns_of(pps, dts=(STEP,)):
    """The spawns per call of a fresh emitter with Options::dt = 0.01, from the emulation of the schedule (held to the reference's
    recorded counts by test_pt_emitter_host.py)."""
    o = np.tile(np.array([1.0, 0.0, 1.0, 1.0, pps, 0.01, 1], F), (len(dts), 1))
    return [int(v) for v in EC.emu_schedule(o, np.array(dts, F))[1]]


def holes(n, at):
    alive = np.ones(n, np.uint8)
    alive[list(at)] = 0
    return alive


HOLES_1200 = (0, 63, 64, 255, 256, 1023, 1024, 1199)
SLOT_CASES = [
    # (pool, capacity, alive pattern, pps): the one substep spawns spawns_of(pps) = 3, 10 or 1000 for pps = 300, 1000 or 100000
    ("pool1200", 1200, lambda: holes(1200, HOLES_1200), 300.0),                 # 3 spawns, 8 holes
    ("pool1200", 1200, lambda: holes(1200, HOLES_1200), 1000.0),                # 10 spawns, 8 holes: 2 dropped
    ("pool1200", 1200, lambda: np.zeros(1200, np.uint8), 1000.0),               # none alive
    ("pool1200", 1200, lambda: np.zeros(1200, np.uint8), 100000.0),             # 1000 spawns across 16 waves and 4 workgroups
    ("pool1200", 1200, lambda: np.ones(1200, np.uint8), 300.0),                 # all alive: everything dropped
    ("pool1200", 1200, lambda: (np.arange(1200) % 2).astype(np.uint8), 100000.0),   # 600 dead, 1000 spawns
    ("pool1200", 1200, lambda: holes(1200, HOLES_1200), 0.0),                   # no spawn at all
    ("cbox_particles", 61, lambda: holes(61, (0, 30, 60)), 300.0),              # as many spawns as holes
    ("cbox_particles", 61, lambda: holes(61, (0, 60)), 300.0),                  # one more
    ("cbox_particles", 61, lambda: holes(61, (0, 59, 60)), 100.0),              # fewer
    ("cbox_particles", 61, lambda: np.zeros(61, np.uint8), 100000.0),
    ("cbox_particles", 61, lambda: np.ones(61, np.uint8), 300.0),
]


@pytest.mark.parametrize("which", range(len(SLOT_CASES)))
def test_slot_rule(collide, renders, which):
    """The k spawns of a substep go to np.flatnonzero(alive == 0)[:k] with ordinals in slot order; what finds no slot is counted; a dead
    slot that takes no spawn keeps every bit; the alive slots are srt_pt_particles_step's of the compacted arrays."""
    name, n, pattern, pps = SLOT_CASES[which]
    pt, pool, S = renders(name)
    if n == 61:
        pool = np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + 61, dtype=np.uint32)      # the 60 particles and the first small sphere
        assert S["objects"][int(pool[-1])]["kind"] == "sphere"
    before = hand_pool(n, pattern(), seed=which)
    opts = dict(velocity=4.0, angle=70.0, scale=0.03, lifetime=2.5, pps=pps, dt=0.01, enabled=True)
    pose = (np.array([0.1, 0.7, -0.2], F), np.array([15.0, -30.0, 60.0], F))
    em = pt.create_emitter(collide, pool, 1.0)
    em.set_options(**opts)
    em.set_pose(*pose)
    em.seed(which)
    em.write(**before)
    em.step_device(STEP)
    after, counts = em.read(), em.counts()
    em.close()
    k = counts["born"]
    assert k == spawns_of(pps)[0] and (k > 0) == (pps > 0)
    dead = np.flatnonzero(before["alive"] == 0)
    took, idle, live = dead[:k], dead[k:], np.flatnonzero(before["alive"])
    assert counts["dropped"] == max(0, k - len(dead)) and counts["alive"] == len(live) + len(took)
    # the spawned slots
    assert np.all(after["alive"][took] == 1) and np.array_equal(after["birth"][took], np.arange(len(took), dtype=np.uint32))
    assert EC.bits_equal(after["age"][took], np.full(len(took), 2.5, F)) and EC.bits_equal(after["pos"][took], np.tile(pose[0], (len(took), 1)))
    o7 = np.array([4.0, 70.0, 0.03, 2.5, pps, 0.01, 1], F)
    want_vel = EC.emu_velocities(o7, np.concatenate(pose), EC.emu_uniforms(which, int(pool[0]), 0, len(took)))
    assert EC.bits_equal(after["vel"][took], want_vel)
    # the dead slots that took no spawn: every bit
    assert np.all(after["alive"][idle] == 0) and np.array_equal(after["birth"][idle], before["birth"][idle])
    for key in ("pos", "vel", "age"):
        assert np.array_equal(after[key][idle].view(np.uint32), before[key][idle].view(np.uint32)), key
    # the alive slots: one Particle::update
    if len(live):
        pos, vel, age, alive = collide.particles_step(before["pos"][live], before["vel"][live], before["age"][live], 0.01, F(1.0) * F(0.03))
        assert EC.bits_equal(after["pos"][live], pos) and EC.bits_equal(after["vel"][live], vel) and EC.bits_equal(after["age"][live], age)
        assert np.array_equal(after["alive"][live], alive) and np.array_equal(after["birth"][live], before["birth"][live])


def test_masked_step(collide, renders):
    """Dead slots filled with NaN stay bit-identical through three substeps without a spawn; the alive slots - some of which die on
    the way and are then left alone - equal particles_step on the compacted arrays, substep by substep."""
    pt, pool, _ = renders("pool1200")
    n = len(pool)
    alive = (np.random.default_rng(3).random(n) < 0.6).astype(np.uint8)
    alive[[0, 63, 64, 1199]] = (1, 0, 1, 1)
    before = hand_pool(n, alive, seed=31)
    live = np.flatnonzero(alive)
    before["age"][live[::3]] = F(0.015)                       # dead after the second substep
    before["vel"][live[::5]] *= F(40.0)                       # fast ones: they reach a wall inside a substep
    em = pt.create_emitter(collide, pool, 1.0)
    em.set_options(scale=0.03, pps=0.0, dt=0.01, enabled=True)
    em.write(**before)
    em.step_device(0.035)                                     # three substeps
    after, counts = em.read(), em.counts()
    em.close()
    pos, vel, age, on = before["pos"].copy(), before["vel"].copy(), before["age"].copy(), alive.copy()
    bounced = 0
    for _ in range(3):
        idx = np.flatnonzero(on)
        p, v, a, al = collide.particles_step(pos[idx], vel[idx], age[idx], 0.01, F(1.0) * F(0.03))
        bounced += int(np.sum(np.abs(v[:, 0] - vel[idx, 0]) > 1e-6))
        pos[idx], vel[idx], age[idx], on[idx] = p, v, a, al
    assert bounced > 10 and 0 < on.sum() < alive.sum()
    for key, want in (("pos", pos), ("vel", vel), ("age", age)):
        assert np.array_equal(after[key].view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)), key
    assert np.array_equal(after["alive"], on) and np.array_equal(after["birth"], before["birth"])
    assert counts == {"alive": int(on.sum()), "born": 0, "dropped": 0}


FRAME_OPTS = dict(velocity=3.0, angle=40.0, scale=float(RDC.PARTICLE_SCALE), lifetime=0.05, pps=300.0, dt=0.01, enabled=True)
FRAME_POSE = ([0.1, 0.5, 0.0], [25.0, 0.0, -35.0])


def test_frame_loop(srt, torch, collide):
    """Three frame_device + render_epoch_device on one stream with no host wait - nothing settled on the way - against a second context
    driven by Emitter.step and the host forms set_active / repose_refit / render_epoch: the image, the active table, the dumps, the pool."""
    S, pidx = EC.pool("cbox_particles")
    nobj, n = len(S["objects"]), len(pidx)
    pt = make_pt(srt, S)
    em = pt.create_emitter(collide, pidx, 1.0)
    em.set_options(**FRAME_OPTS)
    em.set_pose(*FRAME_POSE)
    em.seed(11)
    local_tiles, _, floats_per_tile = pt.tile_info()
    tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    for frame in range(3):
        em.frame_device(0.03, s)
        pt.render_epoch_device(s, SEED, frame, 1, tiles.data_ptr())
    pt.untile_device(s, tiles.data_ptr(), image.data_ptr())
    assert pt.top_refit_pending()[0] == 6                     # set_active_device and repose_refit_device per frame, none settled on the way
    st.synchronize()
    got = {"image": image.cpu().numpy().reshape(HT, W, 3), "pool": em.read(), "counts": em.counts(), "active": pt.active(), "dumps": IC.all_dumps(pt, nobj)}
    em.close(); pt.close()
    ref = make_pt(srt, S)
    rem = ref.create_emitter(collide, pidx, 1.0)
    rem.set_options(**FRAME_OPTS)
    rem.set_pose(*FRAME_POSE)
    rem.seed(11)
    populations = []
    for frame in range(3):
        rem.step(0.03)
        p = rem.read()
        ref.set_active(pidx, p["alive"])
        ref.repose_refit(pidx, RDC.translate_scale_product(p["pos"], RDC.PARTICLE_SCALE))
        ref_image = ref.render_epoch(SEED, frame, 1)
        populations.append(int(p["alive"].sum()))
    want = {"pool": p, "counts": rem.counts(), "active": ref.active(), "dumps": IC.all_dumps(ref, nobj)}
    rem.close(); ref.close()
    per_frame = spawns_of(FRAME_OPTS["pps"], (0.03, 0.03, 0.03))
    born = sum(per_frame)                                     # 3 spawns per substep, 5 substeps of life
    assert populations[0] == per_frame[0] > 0 and 0 < populations[2] < born and want["counts"] == {"alive": populations[2], "born": born, "dropped": 0}
    assert got["counts"] == want["counts"] and np.array_equal(got["pool"]["alive"], want["pool"]["alive"]) and np.array_equal(got["pool"]["birth"], want["pool"]["birth"])
    for key in ("pos", "vel", "age"):
        assert EC.bits_equal(got["pool"][key], want["pool"][key]), key
    assert np.array_equal(got["active"], want["active"]) and np.array_equal(got["active"][pidx], want["pool"]["alive"])
    assert IC.dumps_equal(got["dumps"], want["dumps"])
    assert EC.bits_equal(got["image"], ref_image)


def test_seeded_generator(collide, renders):
    """Without a uniform buffer: 1000 spawns in one substep; every velocity is the emulation's for the two SRT-RNG v1 draws keyed (seed,
    objects[0], ordinal).  Another seed gives other velocities; clear() empties the pool and keeps ordinals and schedule."""
    pt, pool, _ = renders("pool1200")
    o7 = np.array([5.0, 100.0, 0.02, 3.0, 100000.0, 0.01, 1], F)
    pose = np.array([0.0, 0.8, 0.1, -20.0, 45.0, 10.0], F)
    out = []
    for seed in (77, 78):
        em = pt.create_emitter(collide, pool, 1.0)
        em.set_options(*(float(v) for v in o7[:6]), enabled=True)
        em.set_pose(pose[:3], pose[3:])
        em.seed(seed)
        em.step(STEP)
        p = em.read()
        slots = np.flatnonzero(p["alive"])
        n1, n2 = spawns_of(100000.0, (STEP, 0.01))
        assert n1 > 960 and n1 + n2 > 1200 > n2               # past fifteen waves; the second step fits only into a cleared pool
        assert np.array_equal(slots, np.arange(n1)) and np.array_equal(p["birth"][slots], np.arange(n1, dtype=np.uint32))
        u = EC.emu_uniforms(seed, int(pool[0]), 0, n1)
        assert EC.bits_equal(p["vel"][slots], EC.emu_velocities(o7, pose, u))
        out.append(p["vel"][slots])
        if seed == 78:
            em.clear()
            assert em.counts() == {"alive": 0, "born": n1, "dropped": 0}
            em.step(0.01)                                     # 0.005 left over + 0.01: one more substep; the ordinals go on
            p = em.read()
            assert em.counts() == {"alive": n2, "born": n1 + n2, "dropped": 0}
            assert np.array_equal(p["birth"][np.flatnonzero(p["alive"])], np.arange(n1, n1 + n2, dtype=np.uint32))
        em.close()
    assert not EC.bits_equal(out[0], out[1])


def test_refused_steps_enqueue_nothing(srt, torch, collide, renders):
    """A step whose last ordinal lies beyond the uniform buffer, and one beyond the substep bound, on the device: refused with the
    host's codes, the pool, the ordinals and the schedule as they were - the next step is the one a fresh emitter would take."""
    pt, pool, _ = renders("pool1200")
    em = pt.create_emitter(collide, pool, 1.0)
    em.set_options(velocity=4.0, angle=70.0, scale=0.03, lifetime=2.5, pps=300.0, dt=0.01, enabled=True)
    d_u = on_device(torch, np.random.default_rng(5).random(2 * 4, dtype=F))
    em.set_uniforms_device(d_u.data_ptr(), d_u.numel())
    k2, k1 = spawns_of(300.0, (0.025,))[0], spawns_of(300.0)[0]
    assert k1 <= 4 < k2
    with pytest.raises(srt.SrtError, match="uniform buffer is too short") as e:
        em.step_device(0.025)
    assert e.value.status == -1
    with pytest.raises(srt.SrtError, match="substeps") as e:
        em.step_device(0.01 * (EC.MAX_SUBSTEPS + 2))
    assert e.value.status == -4
    assert em.counts() == {"alive": 0, "born": 0, "dropped": 0} and not em.read()["alive"].any()
    em.step_device(STEP)
    p = em.read()
    assert em.counts() == {"alive": k1, "born": k1, "dropped": 0} and np.array_equal(np.flatnonzero(p["alive"]), np.arange(k1))
    o7 = np.array([4.0, 70.0, 0.03, 2.5, 300.0, 0.01, 1], F)
    assert EC.bits_equal(p["vel"][:k1], EC.emu_velocities(o7, np.zeros(6, F), d_u.cpu().numpy().reshape(-1, 2)[:k1]))
    em.close()


def test_group(srt, collide):
    """PathtracerGroup.create_emitter on a one-device group: the single context's pool."""
    S, pidx = EC.pool("cbox_particles")
    groups = []
    for scene in (S, EC.collide_scene()):
        g = srt.PathtracerGroup([0])
        g.set_params(W, HT, 1, DEPTH, True)
        g.build_scene(scene)
        g.set_camera(scene["camera"])
        groups.append(g)
    grp, cgrp = groups
    gem = grp.create_emitter(cgrp, pidx, 1.0)
    gem.set_options(**FRAME_OPTS)
    gem.set_pose(*FRAME_POSE)
    gem.seed(11)
    for _ in range(3):
        gem.step(0.03)
    got, counts = gem.read(), gem.counts()
    gem.frame_device(0.03)
    image = grp.render_epoch(SEED, 0, 1)
    with pytest.raises(ValueError):
        gem.set_uniforms_device([], 0)
    gem.close(); grp.close(); cgrp.close()
    pt = make_pt(srt, S)
    em = pt.create_emitter(collide, pidx, 1.0)
    em.set_options(**FRAME_OPTS)
    em.set_pose(*FRAME_POSE)
    em.seed(11)
    for _ in range(3):
        em.step(0.03)
    want = em.read()
    assert counts == em.counts() and counts["born"] == sum(spawns_of(FRAME_OPTS["pps"], (0.03, 0.03, 0.03)))
    em.frame_device(0.03)
    pt.sync()
    want_image = pt.render_epoch(SEED, 0, 1)
    em.close(); pt.close()
    for key in ("pos", "vel", "age", "alive", "birth"):
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
    assert EC.bits_equal(image, want_image)
