"""Frame time of an emitting particle pool, two ways, on the GPU: a pool of `capacity` instanced cubes (tests/_repose_refit_cases.py:
pool_scene) rendered at 128x128, 1 spp, depth 4, the particles colliding with the Cornell box of tests/_emitter_cases.py.  A frame
is 1 / 60 s of Scene_Particles::step (Options::dt 0.01: one or two substeps), gen_instances and one epoch.  pps = capacity and a
lifetime of 0.5 s keep about half of the pool alive.

  (a) emitter       Emitter.frame_device -> render_epoch_device, one stream, no host wait inside the loop.
  (b) host spawns   what a caller had to build before the emitter: the schedule in Python, and per substep particles_step_device, a
                    read-back of `alive`, the spawn arithmetic in numpy for the lowest dead slots and an upload of their pos, vel, age
                    and alive; then particle_transforms_device -> set_active_device -> repose_refit_device -> render_epoch_device.

The host clock runs around the whole loop, which ends in a stream synchronise; loop time / frames is the frame time.  Each run warms
up until the population is steady before its timed window; the ways alternate, `runs` times each, and the medians over the runs are
reported with min and max.  Prints one JSON line per capacity; DESIGN.md records a run.

    python tools/emitter_frame_time.py [frames = 40] [runs = 5] [capacities = 1200,65536] [warm-up frames = 40]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import srt_amd  # noqa: E402
import _emitter_cases as EC  # noqa: E402
import _repose_refit_cases as C  # noqa: E402

F = np.float32
W = HT = 128
SPP, DEPTH, SEED = 1, 4, 9
FRAME_DT, STEP_DT, SCALE, LIFETIME, VELOCITY, ANGLE = 1.0 / 60.0, 0.01, 0.02, 0.5, 2.0, 120.0
POSE = ([0.0, 0.8, 0.0], [10.0, 0.0, 25.0])
WARM = 40                                                     # the default warm-up, 0.67 s: longer than a lifetime (30 frames)


def context(S):
    pt = srt_amd.Pathtracer(0)
    pt.set_params(W, HT, 1, DEPTH, True)
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    return pt


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


class HostSchedule:
    """Scene_Particles::step's last_update (float) and particle_cooldown (double) in Python: the spawns of every substep of a frame."""

    def __init__(self, pps):
        self.last, self.cooldown, self.period = F(0.0), 0.0, 1.0 / float(F(pps))

    def frame(self, dt):
        out = []
        self.last = F(self.last + F(dt))
        while self.last > F(STEP_DT):
            self.cooldown -= float(F(STEP_DT))
            k = 0
            while self.cooldown <= 0.0:
                k += 1
                self.cooldown += self.period
            out.append(k)
            self.last = F(self.last - F(STEP_DT))
        return out


def rotation(euler):
    x, y, z = np.radians(np.asarray(euler, np.float64))
    rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(F)


def main(frames, runs, capacities, warm=WARM):
    import torch

    collide = context(EC.collide_scene())
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    for n in capacities:
        S = C.pool_scene(n)
        pidx = np.arange(n, dtype=np.uint32)
        pps = float(n)
        R, cos_half = rotation(POSE[1]), F(np.cos(np.radians(ANGLE) / 2))

        def emitter_loop(pt, em, tiles, first, count):
            t0 = time.perf_counter()
            for f in range(first, first + count):
                em.frame_device(FRAME_DT, s)
                pt.render_epoch_device(s, SEED, f, SPP, tiles.data_ptr())
            st.synchronize()
            return time.perf_counter() - t0

        def host_loop(pt, state, sched, rng, tiles, first, count):
            d_pos, d_vel, d_age, d_alive, d_T = state
            t0 = time.perf_counter()
            with torch.cuda.stream(st):
                for f in range(first, first + count):
                    for k in sched.frame(FRAME_DT):
                        collide.particles_step_device(d_pos.data_ptr(), d_vel.data_ptr(), d_age.data_ptr(), n, STEP_DT, SCALE, d_alive.data_ptr(), s)
                        alive = d_alive.cpu().numpy()              # the read-back: waits for the stream
                        slots = np.flatnonzero(alive == 0)[:k]
                        if len(slots):
                            u = rng.random((len(slots), 2), dtype=F)
                            z = cos_half + (F(1) - cos_half) * u[:, 0]
                            t, r = F(2 * np.pi) * u[:, 1], np.sqrt(F(1) - z * z)
                            vel = (F(VELOCITY) * np.stack([r * np.cos(t), z, r * np.sin(t)], axis=1)) @ R.T
                            idx = torch.from_numpy(slots).to("cuda:0")
                            d_pos[idx] = torch.from_numpy(np.tile(np.asarray(POSE[0], F), (len(slots), 1))).to("cuda:0")
                            d_vel[idx] = torch.from_numpy(np.ascontiguousarray(vel, F)).to("cuda:0")
                            d_age[idx] = LIFETIME
                            d_alive[idx] = 1
                    pt.particle_transforms_device(d_pos.data_ptr(), n, SCALE, d_T.data_ptr(), s)
                    pt.set_active_device(pidx, d_alive.data_ptr(), s)
                    pt.repose_refit_device(pidx, d_T.data_ptr(), s)
                    pt.render_epoch_device(s, SEED, f, SPP, tiles.data_ptr())
            st.synchronize()
            return time.perf_counter() - t0

        emitter_ms, host_ms, alive_end = [], [], {}
        for r in range(runs):
            for way in ("emitter", "host"):
                pt = context(S)
                local_tiles, _, floats_per_tile = pt.tile_info()
                tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
                if way == "emitter":
                    em = pt.create_emitter(collide, pidx, 1.0)
                    em.set_options(velocity=VELOCITY, angle=ANGLE, scale=SCALE, lifetime=LIFETIME, pps=pps, dt=STEP_DT, enabled=True)
                    em.set_pose(*POSE)
                    em.seed(r)
                    emitter_loop(pt, em, tiles, 0, warm)
                    emitter_ms.append(emitter_loop(pt, em, tiles, warm, frames) / frames * 1e3)
                    alive_end[way] = em.counts()
                    em.close()
                else:
                    state = (torch.zeros((n, 3), device="cuda:0"), torch.zeros((n, 3), device="cuda:0"), torch.zeros(n, device="cuda:0"),
                             torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros((n, 16), device="cuda:0"))
                    torch.cuda.synchronize()
                    sched, rng = HostSchedule(pps), np.random.default_rng(r)
                    host_loop(pt, state, sched, rng, tiles, 0, warm)
                    host_ms.append(host_loop(pt, state, sched, rng, tiles, warm, frames) / frames * 1e3)
                    alive_end[way] = int(state[3].sum().item())
                pt.close()
                print(f"capacity {n} run {r} {way}: {(emitter_ms if way == 'emitter' else host_ms)[-1]:.2f} ms per frame", file=sys.stderr, flush=True)
        out = {"scene": f"pool of {n} cubes, colliding with cbox_particles without its particles", "size": [W, HT], "spp": SPP, "depth": DEPTH, "capacity": n,
               "pps": pps, "lifetime": LIFETIME, "frame_dt": FRAME_DT, "options_dt": STEP_DT, "frames": frames, "warm_up_frames": warm, "runs": runs,
               "emitter_frame_ms": summary(emitter_ms), "host_spawn_frame_ms": summary(host_ms), "emitter_counts_at_the_end": alive_end["emitter"],
               "host_spawn_alive_at_the_end": alive_end["host"],
               "frame_time_ratio_host_over_emitter": statistics.median(host_ms) / statistics.median(emitter_ms)}
        print(json.dumps(out), flush=True)
    collide.close()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if len(a) > 0 else 40, int(a[1]) if len(a) > 1 else 5, [int(c) for c in a[2].split(",")] if len(a) > 2 else [1200, 65536],
         int(a[3]) if len(a) > 3 else WARM)
