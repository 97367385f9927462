"""Device time of a 16-spp epoch at 1024 x 1024 with Env_Map's uniform sampler and with its image sampler (srt_pt_set_env_sampling), on
the GPU: scenes cbox_envmap (area light + map) and the open box without its area light (every light sample is the map's), each under
the 37 x 19 map of cbox_envmap and under a generated 2048 x 1024 sun map (an 8 MB CDF: L2 / MALL-resident).

Per point: two warm-up epochs, then EPOCHS timed ones (srt_pt_kernel_time: HIP events around the dominant kernel's launches), the two
modes in alternation on one context; median, minimum and maximum ms per epoch, the rays of one epoch (the draw ledgers differ, so
the paths and their ray counts do too) and ms per million rays.  One JSON line per point into profiles/env_sampling_time.jsonl (or
the path given).

    python tools/env_sampling_time.py [out.jsonl] [epochs]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import srt_amd  # noqa: E402
from _cases import pt_scene  # noqa: E402

W = H = 1024
SPP, DEPTH, SEED, WARMUP = 16, 8, 11, 2


def sun_map(w=2048, h=1024):
    """A sky gradient with a small, very bright sun: what an HDR map's luminance looks like to the sampler."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([0.2 + 0.5 * yy / h, 0.3 + 0.4 * xx / w, 0.9 - 0.5 * yy / h], -1).astype(np.float32)
    img += (5e3 * np.exp(-((xx - 0.3 * w) ** 2 + (yy - 0.7 * h) ** 2) / (2 * 6.0 ** 2)))[..., None].astype(np.float32)
    return np.ascontiguousarray(img, np.float32)


def scenes():
    small = np.ascontiguousarray(pt_scene("cbox_envmap")["env"]["image"], np.float32)
    for map_name, img in (("37x19", small), ("sun2048x1024", sun_map())):
        a = pt_scene("cbox_envmap")
        a["env"] = {"type": 3, "image": img}
        yield "cbox_envmap", map_name, a
        b = pt_scene("cbox_envonly")
        b["env"] = {"type": 3, "image": img}
        yield "cbox_envonly", map_name, b


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "env_sampling_time.jsonl")
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    with open(out_path, "w") as out:
        for scene_name, map_name, scene in scenes():
            pt = srt_amd.Pathtracer(0)
            pt.set_params(W, H, SPP, DEPTH, True)
            pt.build_scene(scene)
            pt.set_camera(scene["camera"])
            times = {"uniform": [], "image": []}
            rays = {}
            for k in range(WARMUP + epochs):
                for mode in ("uniform", "image"):
                    pt.set_env_sampling(mode)
                    pt.kernel_time(True)
                    pt.ray_count(reset=True)
                    pt.render_epoch(SEED, k * SPP, SPP)
                    ms, _ = pt.kernel_time(True)
                    if k >= WARMUP:
                        times[mode].append(ms)
                    rays[mode] = pt.ray_count()[0]
            for mode in ("uniform", "image"):
                t = sorted(times[mode])
                line = {"scene": scene_name, "map": map_name, "mode": mode, "width": W, "height": H, "spp": SPP, "depth": DEPTH,
                        "kernel_form": pt.kernel_form(), "epochs": epochs, "ms_median": t[len(t) // 2], "ms_min": t[0], "ms_max": t[-1],
                        "rays_per_epoch": int(rays[mode]), "ms_per_mray": t[len(t) // 2] / (rays[mode] / 1e6)}
                out.write(json.dumps(line) + "\n")
                print(json.dumps(line), flush=True)
            pt.close()


if __name__ == "__main__":
    main()
