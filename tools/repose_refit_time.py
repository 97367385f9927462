"""Frame time of a particle loop with srt_pt_repose_refit_device against the same loop with srt_pt_repose_device, on the GPU, and
what the refitted tree costs to trace: N posed copies of blob_mesh(3) (the pool of tools/repose_device_time.py: one mesh, N - 1
instances, a jittered grid of pitch 1 under the Cornell light, no walls) drift apart with seeded constant velocities of up to
`SPEED` per axis and frame.  A frame is positions (a torch op) -> particle_transforms_device -> repose -> one 1-spp epoch at
64x64, all on one stream; the loop is synchronised once, after its last frame, and the host clock around the whole loop divided
by the frames is the frame time; a second clock around each repose call alone gives the host time inside the call.  Both loops
start from the same commit and see the same positions.  Then, at 1, 10 and 100 frames of drift: the SAH cost of the refitted
tree and of the tree repose_device builds for the same poses, next to the rays per second of one 16-spp epoch on each.
Prints JSON lines; DESIGN.md records a run.

    python tools/repose_refit_time.py [N = 4096] [frames = 100] [runs = 3]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from repose_device_time import scene, transforms  # noqa: E402  (also puts the package on the path)
import srt_amd  # noqa: E402

SPEED = 0.02


def context(S):
    pt = srt_amd.Pathtracer(0)
    pt.set_params(64, 64, 1, 8, True)
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    return pt


def main(n, frames, runs):
    import torch

    T0 = transforms(n, 1)
    T0[:, 0] = T0[:, 5] = T0[:, 10] = 1.0                  # the transforms particle_transforms_device forms: translate * scale(1)
    S = scene(n, T0)
    idx = np.arange(1, n + 1, dtype=np.uint32)
    rng = np.random.default_rng(4)
    pos0 = torch.from_numpy(np.ascontiguousarray(T0[:, 12:15])).to("cuda:0")
    vel = torch.from_numpy(((rng.random((n, 3)) - 0.5) * 2.0 * SPEED).astype(np.float32)).to("cuda:0")
    d_T = torch.zeros((n, 16), device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream

    def loop(pt, call, first, count, tiles):
        """frames [first, first + count) of the loop; returns (seconds for all of them, host seconds inside the repose calls)"""
        inside = 0.0
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            for f in range(first, first + count):
                pos = pos0 + vel * float(f + 1)
                pt.particle_transforms_device(pos.data_ptr(), n, 1.0, d_T.data_ptr(), s)
                c0 = time.perf_counter()
                call(idx, d_T.data_ptr(), s)
                inside += time.perf_counter() - c0
                pt.render_epoch_device(s, 9, f, 1, tiles.data_ptr())
        st.synchronize()
        return time.perf_counter() - t0, inside

    def rays_per_second(pt):
        pt.render_epoch(9, 0, 16)
        pt.ray_count(reset=True)
        t0 = time.perf_counter()
        pt.render_epoch(9, 0, 16)
        dt = time.perf_counter() - t0
        return pt.ray_count(reset=True)[0] / dt

    out = {"instances": n, "frames": frames, "runs": runs, "speed_per_axis_and_frame": SPEED}
    checkpoints = {}
    for name in ("repose_device", "repose_refit_device"):
        frame_ms, inside_ms = [], []
        for r in range(runs):
            pt = context(S)
            call = getattr(pt, name)
            local_tiles, _, floats_per_tile = pt.tile_info()
            tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
            torch.cuda.synchronize()
            loop(pt, call, 0, 2, tiles)                    # warm-up: code objects, tables, workspace (two frames of the same drift)
            total, inside = loop(pt, call, 0, frames, tiles)
            frame_ms.append(total / frames * 1e3)
            inside_ms.append(inside / frames * 1e3)
            pt.close()
        out[name] = {"frame_ms": {"median": statistics.median(frame_ms), "min": min(frame_ms), "max": max(frame_ms)},
                     "host_ms_inside_the_call": {"median": statistics.median(inside_ms), "min": min(inside_ms), "max": max(inside_ms)}}
    print(json.dumps(out), flush=True)
    # the cost of tracing a refitted tree: the same drift, refitted every frame, against a rebuild of the same poses
    pt, rebuilt = context(S), context(S)
    local_tiles, _, floats_per_tile = pt.tile_info()
    tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
    torch.cuda.synchronize()
    checkpoints["committed"] = {"tree_cost": pt.scene_tree_cost(), "rays_per_second": rays_per_second(pt)}
    done = 0
    for upto in (1, 10, 100):
        loop(pt, pt.repose_refit_device, done, upto - done, tiles)
        done = upto
        with torch.cuda.stream(st):
            pos = pos0 + vel * float(upto)
            rebuilt.particle_transforms_device(pos.data_ptr(), n, 1.0, d_T.data_ptr(), s)
            rebuilt.repose_device(idx, d_T.data_ptr(), s)
        checkpoints[f"after {upto} frames"] = {"refitted_tree_cost": pt.scene_tree_cost(), "rebuilt_tree_cost": rebuilt.scene_tree_cost(),
                                               "refitted_rays_per_second": rays_per_second(pt), "rebuilt_rays_per_second": rays_per_second(rebuilt)}
    pt.close(); rebuilt.close()
    print(json.dumps({"instances": n, "tree": checkpoints}), flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(a[0] if len(a) > 0 else 4096, a[1] if len(a) > 1 else 100, a[2] if len(a) > 2 else 3)
