"""Frame time of a particle pool whose population changes, three ways, on the GPU: cbox_particles (74 objects, 60 instanced particles)
at 256x256, 4 spp, depth 8.  About 10 % of the particles change state per frame: three die and the three that died the frame before
return (the first particle, the mesh the others are instances of, always lives, so that way (b) can leave the dead out).

  (a) pool loop     particles_step_device -> particle_transforms_device -> set_active_device(d_alive) -> repose_refit_device ->
                    render_epoch_device, one stream, no host wait inside the loop; the deaths and births are torch writes to the
                    ages on the same stream.
  (a') pool loop with a rebuild every tenth frame: srt_pt_repose_device in the place of srt_pt_repose_refit_device there (it waits; the
                    flags persist across it), so that the tree does not degrade over the run.
  (b) commit        what the code before srt_pt_set_active needs for the same frames: particles_step with host arrays, then
                    srt_pt_scene_begin .. srt_pt_scene_commit of the surviving objects at their new places, then
                    render_epoch_device.

The host clock runs around the whole loop, which ends in a stream synchronise; loop time / frames is the frame time.  Each run warms
up (code objects, tables, the list) before its timed window; the ways alternate, `runs` times each, and the medians over the runs
are reported with min and max.  Prints one JSON line; DESIGN.md records a run.

    python tools/active_frame_time.py [frames = 40] [runs = 5]"""
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
import _instance_cases as IC  # noqa: E402
import _repose_device_cases as RDC  # noqa: E402

W = HT = 256
SPP, DEPTH, SEED = 4, 8, 9
DT, RADIUS = 0.01, 0.015
BLOCK = 3                                                    # particles that die per frame; as many return


def context(S):
    pt = srt_amd.Pathtracer(0)
    pt.set_params(W, HT, 1, DEPTH, True)
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    return pt


def blocks(n):
    """The particles that die in frame f (never particle 0, the source mesh): block f % nblocks of 1 .. n - 1."""
    ids = np.arange(1, n)
    return [ids[k:k + BLOCK] for k in range(0, len(ids) - BLOCK + 1, BLOCK)]


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(frames, runs):
    import torch

    S = IC.particles_shared()[0]
    pidx = np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + IC.PARTICLE_COUNT, dtype=np.uint32)
    n = len(pidx)
    pos0 = RDC.particle_positions(S)
    vel0 = ((np.random.default_rng(8).random((n, 3)) - 0.5) * 2.0).astype(np.float32)
    B = blocks(n)
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    d_blocks = [torch.from_numpy(b.astype(np.int64)).to("cuda:0") for b in B]

    def pool_loop(pt, state, tiles, first, count, rebuild_every=0):
        d_pos, d_vel, d_age, d_alive, d_T = state
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            for f in range(first, first + count):
                d_age[d_blocks[f % len(B)]] = 0.0            # these die in this step ..
                d_age[d_blocks[(f - 1) % len(B)]] = 100.0    # .. and the ones that died in the last step are born again
                pt.particles_step_device(d_pos.data_ptr(), d_vel.data_ptr(), d_age.data_ptr(), n, DT, RADIUS, d_alive.data_ptr(), s)
                pt.particle_transforms_device(d_pos.data_ptr(), n, RDC.PARTICLE_SCALE, d_T.data_ptr(), s)
                pt.set_active_device(pidx, d_alive.data_ptr(), s)
                if rebuild_every and f % rebuild_every == rebuild_every - 1:
                    pt.repose_device(pidx, d_T.data_ptr(), s)
                else:
                    pt.repose_refit_device(pidx, d_T.data_ptr(), s)
                pt.render_epoch_device(s, SEED, f, SPP, tiles.data_ptr())
        st.synchronize()
        return time.perf_counter() - t0

    def commit_loop(pt, state, tiles, first, count):
        t0 = time.perf_counter()
        for f in range(first, first + count):
            state["age"][B[f % len(B)]] = 0.0
            state["age"][B[(f - 1) % len(B)]] = 100.0
            state["pos"], state["vel"], state["age"], alive = pt.particles_step(state["pos"], state["vel"], state["age"], DT, RADIUS)
            T = RDC.translate_scale_product(state["pos"], RDC.PARTICLE_SCALE)
            posed = IC.with_poses(S, pidx, T)
            dead = {int(pidx[k]) for k in np.nonzero(alive == 0)[0]}
            posed["objects"] = [o for k, o in enumerate(posed["objects"]) if k not in dead]
            pt.build_scene(posed)
            pt.render_epoch_device(s, SEED, f, SPP, tiles.data_ptr())
        st.synchronize()
        return time.perf_counter() - t0

    warm = 5
    pool_ms, rebuilt_ms, commit_ms, pool_up, costs = [], [], [], [], {}
    for r in range(runs):
        for way in ("pool", "pool_rebuilt", "commit"):
            pt = context(S)
            local_tiles, _, floats_per_tile = pt.tile_info()
            tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
            if way != "commit":
                every = 10 if way == "pool_rebuilt" else 0
                state = (torch.from_numpy(pos0.copy()).to("cuda:0"), torch.from_numpy(vel0.copy()).to("cuda:0"), torch.full((n,), 100.0, device="cuda:0"),
                         torch.ones(n, dtype=torch.uint8, device="cuda:0"), torch.zeros((n, 16), device="cuda:0"))
                torch.cuda.synchronize()
                cost0 = pt.scene_tree_cost()
                pool_loop(pt, state, tiles, 0, warm, every)
                b0 = pt.scene_counts()["uploaded_bytes"]
                (rebuilt_ms if every else pool_ms).append(pool_loop(pt, state, tiles, warm, frames, every) / frames * 1e3)
                if not every:
                    pool_up.append((pt.scene_counts()["uploaded_bytes"] - b0) / frames)
                hidden = int(np.sum(pt.active() == 0))
                costs[way] = [cost0, pt.scene_tree_cost()]   # committed, after the last frame
            else:
                state = {"pos": pos0.copy(), "vel": vel0.copy(), "age": np.full(n, 100.0, np.float32)}
                torch.cuda.synchronize()
                commit_loop(pt, state, tiles, 0, warm)
                commit_ms.append(commit_loop(pt, state, tiles, warm, frames) / frames * 1e3)
            pt.close()
    out = {"scene": "cbox_particles", "size": [W, HT], "spp": SPP, "depth": DEPTH, "particles": n, "state_changes_per_frame": 2 * BLOCK,
           "hidden_at_the_end": hidden, "frames": frames, "warm_up_frames": warm, "runs": runs,
           "pool_loop_frame_ms": summary(pool_ms), "pool_loop_rebuilt_every_10th_frame_ms": summary(rebuilt_ms),
           "tree_cost_committed_and_after_the_last_frame": costs, "commit_frame_ms": summary(commit_ms), "pool_loop_bytes_up_per_frame": summary(pool_up),
           "frame_time_ratio_commit_over_pool": statistics.median(commit_ms) / statistics.median(pool_ms)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if len(a) > 0 else 40, a[1] if len(a) > 1 else 5)
