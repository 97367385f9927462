"""Commit time of a scene of N posed copies of one mesh, with srt_pt_add_mesh per copy and with srt_pt_add_instance, on a host-only
context (no GPU needed): the Cornell box plus N poses of blob_mesh(3).  Prints one JSON line; DESIGN.md records a run.

    python tools/instance_commit_time.py [poses = 2000] [open]      (open: without the five walls)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srt_amd  # noqa: E402
from soft_rendering_toolsets_amd import scenes  # noqa: E402


def scene(n, walls=True):
    """The Cornell box with the glass blob shrunk to a particle, plus n - 1 more poses of it on a jittered lattice that fills
    the box.  walls = False leaves the five walls out: from a few hundred particles on, some node of the BVH<Object> holds a wall
    and two particles whose centres lie within one tenth of the node's extent on every axis, all nine candidate planes leave one
    side empty, and the reference's build - and with it this one - does not terminate."""
    s = scenes.cornell_with_mesh(3, "glass")
    blob = s["objects"][6]
    rng = np.random.default_rng(5)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    objs = []
    for k in range(n):
        i, j, l = k % side, (k // side) % side, k // (side * side)
        T = np.eye(4, dtype=np.float32)
        T[0, 0] = T[1, 1] = T[2, 2] = np.float32(0.25 / side)
        T[:3, 3] = ((np.array([i, j, l]) + 0.5 + (rng.random(3) - 0.5) * 0.4) / side * [0.9, 0.9, 0.9] - [0.45, -0.05, 0.45]).astype(np.float32)
        objs.append(dict(blob, T=np.ascontiguousarray(T.T.reshape(16))))
    s["objects"] = (s["objects"][:6] if walls else s["objects"][5:6]) + objs + s["objects"][7:]
    return s


def commit_seconds(pt, s, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        pt.build_scene(s)
        out.append(time.perf_counter() - t0)
    return out


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    runs = 5
    walls = not (len(sys.argv) > 2 and sys.argv[2] == "open")
    copies = scene(n, walls)
    shared = scenes.share_meshes(copies)
    pt = srt_amd.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    tc = commit_seconds(pt, copies, runs)
    cc = pt.scene_counts()
    ts = commit_seconds(pt, shared, runs)
    cs = pt.scene_counts()
    print(json.dumps({"poses": n, "walls": walls, "copies_s": tc, "instances_s": ts, "copies_median_s": statistics.median(tc), "instances_median_s": statistics.median(ts),
                      "copies_spread_s": max(tc) - min(tc), "copies_triangles": cc["triangles"], "instances_triangles": cs["triangles"],
                      "copies_blas_records": cc["blas_records"], "instances_blas_records": cs["blas_records"]}))
