"""Time of srt_pt_update_mesh against a fresh srt_pt_scene_begin .. srt_pt_scene_commit of the same scene, on the GPU: object 6 of
scenes.cornell_with_mesh(n) for n = 5 and 7 (8 192 and 131 072 triangles) alternates between two sets of vertex arrays, both
calls under the default builder rule.  Each call ends in a device synchronise of its own; a host clock around it.  Prints one
JSON line per n with the median and the spread (min .. max) of several runs; DESIGN.md records a run.

    python tools/mesh_update_time.py [runs = 9] [n ...]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srt_amd  # noqa: E402
from soft_rendering_toolsets_amd import scenes  # noqa: E402


def arrays(n, seed):
    v, f = scenes.blob_mesh(n, seed)
    p, nr, _ = scenes._flat_mesh_fast(v, f)
    return np.ascontiguousarray(p), np.ascontiguousarray(nr)


def timed(call, sync):
    t0 = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t0) * 1e3


def measure(n, runs):
    S = scenes.cornell_with_mesh(n, "glass")
    sets = [arrays(n, 7), arrays(n, 11)]
    desc = [scenes.with_vertices(S, 6, *a) for a in sets]
    upd, com = srt_amd.Pathtracer(0), srt_amd.Pathtracer(0)
    for pt in (upd, com):
        pt.set_params(64, 64, 1, 8, True)
        pt.build_scene(S)
    # warm-up: both shapes of both calls (first launches load code objects, the workspace grows once)
    for k in (1, 0):
        upd.update_mesh(6, *sets[k])
        com.build_scene(desc[k])
    before = upd.scene_counts()
    tu, tc, tr = [], [], []
    for r in range(runs):                                   # alternating, so that all see the same machine
        k = (r + 1) % 2
        tu.append(timed(lambda: upd.update_mesh(6, *sets[k]), upd.sync))
        tc.append(timed(lambda: com.build_scene(desc[k]), com.sync))
    after = upd.scene_counts()
    # what an update shares with srt_pt_repose - the BVH<Object> rebuild and the upload of the tables of object order - timed as a
    # repose of no object; and the same update with the mesh's tree built on the host
    for r in range(runs):
        tr.append(timed(lambda: upd.repose([], np.zeros((0, 16), np.float32)), upd.sync))
    upd.set_bvh_builder(False)
    th = []
    upd.update_mesh(6, *sets[0])
    for r in range(runs):
        th.append(timed(lambda: upd.update_mesh(6, *sets[(r + 1) % 2]), upd.sync))
    out = {"n_subdiv": n, "triangles": 8 * 4 ** n, "runs": runs,
           "update_ms_median": statistics.median(tu), "update_ms_min": min(tu), "update_ms_max": max(tu),
           "commit_ms_median": statistics.median(tc), "commit_ms_min": min(tc), "commit_ms_max": max(tc),
           "commit_over_update": statistics.median(tc) / statistics.median(tu),
           "empty_repose_ms_median": statistics.median(tr), "empty_repose_ms_min": min(tr), "empty_repose_ms_max": max(tr),
           "update_host_builder_ms_median": statistics.median(th), "update_host_builder_ms_min": min(th), "update_host_builder_ms_max": max(th),
           "update_uploaded_bytes": (after["uploaded_bytes"] - before["uploaded_bytes"]) // runs, "scene_device_bytes": after["device_bytes"],
           "update_ms": tu, "commit_ms": tc}
    upd.close(); com.close()
    return out


if __name__ == "__main__":
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    for n in ([int(a) for a in sys.argv[2:]] or [5, 7]):
        print(json.dumps(measure(n, runs)), flush=True)
