"""Time of srt_pt_repose_device (transforms already in device memory) against srt_pt_repose (the same matrices on the host), on
the GPU: N posed copies of blob_mesh(3) - one mesh and N - 1 instances - on a seeded, jittered grid under the Cornell light, no
walls (walls make the BVH<Object> build non-terminating from a few hundred particles on: DESIGN.md).  All N are re-posed,
alternating between two seeded sets of transforms, under the default builder rule and under set_bvh_builder(False).  Each call
ends in a device synchronise of its own; a host clock around it; the two forms alternate so that both see the same machine.
Prints one JSON line per N and rule with the median and the spread (min .. max) of the runs, the bytes each form adds to the
upload figure per call and the bytes the device form reads back (from the layouts); DESIGN.md records a run.

    python tools/repose_device_time.py [runs = 5] [N ...]
    python tools/repose_device_time.py --commit-only [N ...]      (host-only contexts, no GPU: does each size commit?)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srt_amd  # noqa: E402
from soft_rendering_toolsets_amd import scenes  # noqa: E402

LIGHT = 0                                                  # object 0 is the area light; objects 1 .. N are the blobs


def transforms(n, seed):
    """(n, 16) column-major: cell k of a cubic grid of pitch 1, jittered by up to a quarter of the pitch, uniform scale 0.8 .. 1.2."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    k = np.arange(n)
    cell = np.stack([k % side, (k // side) % side, k // (side * side)], 1).astype(np.float64)
    pos = cell - (side - 1) / 2.0 + (rng.random((n, 3)) - 0.5) * 0.5
    T = np.zeros((n, 16), np.float32)
    T[:, 0] = T[:, 5] = T[:, 10] = (0.8 + 0.4 * rng.random(n)).astype(np.float32)
    T[:, 15] = 1.0
    T[:, 12:15] = pos.astype(np.float32)
    return T


def scene(n, T):
    box = scenes.cornell_box("cbox_lambertian")
    light = [o for o in box["objects"] if o.get("is_light")][0]
    v, f = scenes.blob_mesh(3, 7)
    p, nr, ix = scenes.flat_mesh(v, f)
    objs = [light, {"kind": "mesh", "pos": p, "nrm": nr, "idx": ix, "T": T[0], "material": 5, "is_light": False}]
    objs += [{"kind": "instance", "of": 1, "T": T[k], "material": 5} for k in range(1, n)]
    return {"name": f"blobs{n}", "materials": box["materials"], "objects": objs, "camera": box["camera"]}


def context(device, S, builder):
    pt = srt_amd.Pathtracer(device)
    pt.set_params(64, 64, 1, 8, True)
    if builder is not None:
        pt.set_bvh_builder(*builder)
    pt.build_scene(S)
    return pt


def timed(call, sync):
    t0 = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def measure(n, runs, builder, rule):
    import torch

    sets = [transforms(n, 1), transforms(n, 2)]
    S = scene(n, sets[0])
    idx = np.arange(1, n + 1, dtype=np.uint32)
    host, dev = context(0, S, builder), context(0, S, builder)
    d_sets = [torch.from_numpy(t).to("cuda:0") for t in sets]
    torch.cuda.synchronize()
    for k in (1, 0, 1, 0):                                  # warm-up: both sets through both forms (code objects, the tables, the workspace)
        host.repose(idx, sets[k])
        dev.repose_device(idx, d_sets[k].data_ptr())
    h0, d0 = host.scene_counts(), dev.scene_counts()
    th, td = [], []
    for r in range(runs):
        k = (r + 1) % 2
        th.append(timed(lambda: host.repose(idx, sets[k]), host.sync))
        td.append(timed(lambda: dev.repose_device(idx, d_sets[k].data_ptr()), dev.sync))
    h1, d1 = host.scene_counts(), dev.scene_counts()
    nodes = len(dev.dump_bvh(-1)[0])
    nobj = n + 1
    device_built = builder is None and nobj >= 16384 or (builder is not None and builder[0] and nobj >= builder[1])
    same = all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(host.dump_bvh(-1), dev.dump_bvh(-1)))
    out = {"instances": n, "objects": nobj, "rule": rule, "tree_built_on": "device" if device_built else "host", "runs": runs, "tlas_nodes": nodes,
           "repose_ms": spread(th), "repose_device_ms": spread(td), "repose_over_repose_device": statistics.median(th) / statistics.median(td),
           "repose_uploaded_bytes_per_call": (h1["uploaded_bytes"] - h0["uploaded_bytes"]) // runs,
           "repose_device_uploaded_bytes_per_call": (d1["uploaded_bytes"] - d0["uploaded_bytes"]) // runs,
           # 156 B per listed object; then the tree (40 B per node, 4 B per slot) of a device build, or the posed boxes (24 B per object) a host build starts from
           "repose_device_read_back_bytes_per_call": 156 * n + (40 * nodes + 4 * nobj if device_built else 24 * nobj),
           "same_trees": bool(same), "repose_ms_runs": th, "repose_device_ms_runs": td}
    host.close(); dev.close()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--commit-only":
        for n in ([int(a) for a in args[1:]] or [1024, 16384, 65536]):
            t0 = time.perf_counter()
            pt = context(-1, scene(n, transforms(n, 1)), None)
            pt.repose(np.arange(1, n + 1, dtype=np.uint32), transforms(n, 2))
            print(json.dumps({"instances": n, "commits": True, "objects": pt.scene_counts()["objects"], "tlas_nodes": len(pt.dump_bvh(-1)[0]),
                              "seconds": time.perf_counter() - t0}), flush=True)
            pt.close()
        sys.exit(0)
    runs = int(args[0]) if args else 5
    for n in ([int(a) for a in args[1:]] or [1024, 16384, 65536]):
        for builder, rule in ((None, "default"), ((False, 16384), "set_bvh_builder(False)")):
            print(json.dumps(measure(n, runs, builder, rule)), flush=True)
