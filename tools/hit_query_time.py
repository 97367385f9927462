"""Device time of srt_pt_hit_device through its routes, on the GPU: the per-lane walk (kernel mode 4), the ray-cast kernel forced
(mode 6) and what the automatic mode picks (mode 0), in alternation within one process on the same device ray arrays.

Points: scenes cbox, cbox_particles, cbox_blob131072_glass x rays {camera rays of a 1024 x 1024 image (coherent), random_rays
(incoherent)} x n in {2^10, 2^16, 2^22} x outputs {the nine-float record, the hit byte alone}.  Per point and route: three warm-up
calls, then CALLS timed calls, each between two device events on the stream; median, minimum and maximum.  The outputs of the
routes are compared bit for bit at every point.  One JSON line per point into profiles/hit_query_time.jsonl (or the path given).

A coherent set of n < 2^22 camera rays is n / 1024 whole rows around the middle of the image (the top rows look over the box).

    python tools/hit_query_time.py [out.jsonl] [calls] [sizes, comma-separated] [scenes, comma-separated]

(the last two for a finer sweep, e.g. to place the size below which the automatic mode stays per lane)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import srt_amd  # noqa: E402
from _cases import camera_rays, pt_scene, random_rays  # noqa: E402

SCENES = ("cbox", "cbox_particles", "cbox_blob131072_glass")
SIZES = (1 << 10, 1 << 16, 1 << 22)
ROUTES = (("per_lane", 4), ("cast", 6), ("auto", 0))
WARMUP = 3


def main():
    import torch

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hit_query_time.jsonl")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    sizes = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else SIZES
    scene_names = tuple(sys.argv[4].split(",")) if len(sys.argv) > 4 else SCENES
    dev = "cuda:0"
    nmax = max(SIZES)
    lines = []
    for name in scene_names:
        scene = pt_scene(name)
        pt = srt_amd.Pathtracer(0)
        pt.set_params(64, 64, 1, 8, True)
        pt.build_scene(scene)
        pt.set_camera(scene["camera"])
        ray_sets = {"camera": camera_rays(scene["camera"], 1024, 1024, jitters=((0.5, 0.5), (0.1, 0.2), (0.9, 0.3), (0.3, 0.9))),
                    "random": random_rays(5, nmax)}
        for kind, (org, d, b) in ray_sets.items():
            assert len(org) == nmax
            all_org, all_d, all_b = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (org, d, b))
            for n in sizes:
                first = max(0, 512 - n // 2048) * 1024 if kind == "camera" and n < nmax else 0
                t_org, t_d, t_b = (a[first:first + n] for a in (all_org, all_d, all_b))      # (contiguous slices: rows of the arrays)
                for outputs in ("out9", "hit"):
                    outs = {r: (torch.zeros((n, 9), device=dev) if outputs == "out9" else torch.zeros((n,), dtype=torch.uint8, device=dev)) for r, _ in ROUTES}
                    times = {r: [] for r, _ in ROUTES}
                    taken = {}
                    torch.cuda.synchronize()
                    for it in range(WARMUP + calls):
                        for r, mode in ROUTES:                     # the routes in alternation
                            pt.set_kernel(mode)
                            before = pt.hit_device_paths()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            pt.hit_device(t_org.data_ptr(), t_d.data_ptr(), t_b.data_ptr(), n, outs[r].data_ptr() if outputs == "out9" else 0, 0,
                                          outs[r].data_ptr() if outputs == "hit" else 0, stream=torch.cuda.current_stream().cuda_stream)
                            e1.record()
                            e1.synchronize()
                            after = pt.hit_device_paths()
                            taken[r] = ("cast", "per_lane", "flat")[[a - c for a, c in zip(after, before)].index(1)]
                            if it >= WARMUP:
                                times[r].append(e0.elapsed_time(e1))
                    ref = outs["per_lane"].cpu().numpy()
                    equal = all(np.array_equal(ref.view(np.uint32 if outputs == "out9" else np.uint8),
                                               outs[r].cpu().numpy().view(np.uint32 if outputs == "out9" else np.uint8)) for r, _ in ROUTES)
                    line = {"scene": name, "objects": len(scene["objects"]), "rays": kind, "n": n, "outputs": outputs, "calls": calls,
                            "hit_fraction": float((ref[:, 0] != 0).mean() if outputs == "out9" else ref.mean()), "routes_bit_equal": bool(equal)}
                    for r, _ in ROUTES:
                        t = np.array(times[r])
                        line[r] = {"took": taken[r], "median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                                   "mrays_per_s": float(n / np.median(t) / 1e3)}
                    lines.append(line)
                    print(json.dumps(line), flush=True)
        pt.close()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
    assert all(line["routes_bit_equal"] for line in lines), "the routes disagree"


if __name__ == "__main__":
    main()
