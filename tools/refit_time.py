"""srt_pt_refit_mesh_device against srt_pt_update_mesh_device on the GPU, and what a refitted tree costs to render: object 6 of
scenes.cornell_with_mesh(n) (n = 7: the 131 072-triangle blob of BASELINE's cfg5; n = 3: 512 triangles), one JSON line.

  * wall time of the two calls in one process on the same two device arrays (alternating, so that every call really moves the
    mesh), each ending in the call's own stream synchronise, a host clock around it: median, min and max of `runs`;
  * over a sequence of increasing amplitude a - vertices = blob(seed 7) + a * (blob(seed 11) - blob(seed 7)), same index buffer -
    one context refits the tree committed for a = 0 and one rebuilds: srt_pt_mesh_tree_cost, the dominant kernel's time for one
    16-spp launch at 1024 x 1024 (srt_pt_kernel_time), and the rays of that launch, for both.

Run each n in a fresh process:  python tools/refit_time.py 7 [runs = 5]
SRT_REFIT_LEVEL_LAUNCHES=1 in the environment makes the refit launch every interior level on its own (DESIGN.md "Refit")."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srt_amd  # noqa: E402
from soft_rendering_toolsets_amd import scenes  # noqa: E402

AMPLITUDES = (0.0, 0.05, 0.1, 0.25, 0.5, 1.0)


def arrays(n, seed):
    v, f = scenes.blob_mesh(n, seed)
    p, nr, _ = scenes._flat_mesh_fast(v, f)
    return np.ascontiguousarray(p), np.ascontiguousarray(nr)


def render(pt):
    pt.render_epoch(1, 0, 16)                  # warm-up: buffers, the ray-cast kernel's launch shape for this scene
    pt.ray_count(reset=True)
    pt.kernel_time(True)
    pt.render_epoch(1, 0, 16)
    ms, launches = pt.kernel_time(False)
    rays, _ = pt.ray_count()
    return {"kernel_ms": ms, "launches": launches, "rays": rays}


if __name__ == "__main__":
    import torch

    n = int(sys.argv[1])
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    S = scenes.cornell_with_mesh(n, "glass")
    (p0, n0), (p1, n1) = arrays(n, 7), arrays(n, 11)
    ref, upd = srt_amd.Pathtracer(0), srt_amd.Pathtracer(0)
    for pt in (ref, upd):
        pt.set_params(1024, 1024, 16, 8, True)
        pt.build_scene(S)
        pt.set_camera(S["camera"])
    blend = lambda a: np.ascontiguousarray((p0 + np.float32(a) * (p1 - p0)).astype(np.float32))
    sets = [(torch.from_numpy(blend(a)).cuda(), torch.from_numpy(n0).cuda()) for a in (0.05, 0.1)]
    torch.cuda.synchronize()
    nverts = len(p0)
    calls = {"refit": lambda k: ref.refit_mesh_device(6, sets[k][0].data_ptr(), sets[k][1].data_ptr(), nverts),
             "update": lambda k: upd.update_mesh_device(6, sets[k][0].data_ptr(), sets[k][1].data_ptr(), nverts)}
    for k in (1, 0):                           # warm-up: code objects, the refit tables, the builder's workspace
        for c in calls.values():
            c(k)
    before = ref.scene_counts()
    times = {"refit": [], "update": []}
    for r in range(runs):
        for name, c in calls.items():
            t0 = time.perf_counter()
            c((r + 1) % 2)
            times[name].append((time.perf_counter() - t0) * 1e3)
    after = ref.scene_counts()
    out = {"n_subdiv": n, "triangles": 8 * 4 ** n, "runs": runs, "level_launches": os.environ.get("SRT_REFIT_LEVEL_LAUNCHES", "0"),
           "refit_uploaded_bytes": (after["uploaded_bytes"] - before["uploaded_bytes"]) // runs, "kernel_form": ref.kernel_form()}
    for name, t in times.items():
        out[name + "_ms_median"], out[name + "_ms_min"], out[name + "_ms_max"] = statistics.median(t), min(t), max(t)
    out["update_over_refit"] = out["update_ms_median"] / out["refit_ms_median"]
    # the amplitude sequence: `ref` goes back to the tree of a = 0 first (a rebuild with the committed vertices)
    ref.update_mesh(6, p0, n0)
    upd.update_mesh(6, p0, n0)
    seq = []
    for a in AMPLITUDES:
        p = blend(a)
        ref.refit_mesh(6, p, n0)
        upd.update_mesh(6, p, n0)
        row = {"amplitude": a, "refitted_cost": ref.mesh_tree_cost(6), "rebuilt_cost": upd.mesh_tree_cost(6)}
        for name, pt in (("refitted", ref), ("rebuilt", upd)):
            for k, v in render(pt).items():
                row[name + "_" + k] = v
        seq.append(row)
    out["sequence"] = seq
    out["refit_ms"], out["update_ms"] = times["refit"], times["update"]
    print(json.dumps(out), flush=True)
    ref.close(); upd.close()
