"""Per-frame time of Skin.pose on the GPU against the host route it replaces, for one rigged mesh: tests/golden/mesh_beast.npz (32 311
vertices, 64 618 triangles, scaled into the Cornell box in place of cbox+blob512's blob) with a generated chain of joints along x.

  device route   Skin.pose(posed): 64 B per joint up, the skinning kernels, srt_pt_update_mesh_device (one BVH<Triangle> build);
                 wall time with the call's own synchronise, and the device time of the skinning kernels alone (events around
                 Skin.vertices_device on a stream)
  host route     what the parent commit offers: the numpy restatement tests/_skin_expected.py skinning on the host (weights kept
                 from a find_joints done once, as on the device), then Pathtracer.update_mesh with the 24 B per vertex

Prints one JSON line; asserts nothing.  DESIGN.md quotes a run, profiles/skin_frame_time.json holds it.

    python tools/skin_frame_time.py [frames = 9] [joints = 8]"""
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
from soft_rendering_toolsets_amd import scenes  # noqa: E402

import _skin_cases as SC  # noqa: E402
import _skin_expected as E  # noqa: E402


def beast():
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_beast.npz"))
    pos = np.ascontiguousarray(g["positions"] * np.float32(0.12), np.float32)
    tri = np.ascontiguousarray(g["triangles"], np.int64)
    n = np.zeros_like(pos)
    c = np.cross(pos[tri[:, 1]] - pos[tri[:, 0]], pos[tri[:, 2]] - pos[tri[:, 0]])
    for k in range(3):
        np.add.at(n, tri[:, k], c)
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    return pos, np.ascontiguousarray(n, np.float32), np.ascontiguousarray(tri.reshape(-1), np.uint32)


def rig(pos, njoints):
    lo, hi = float(pos[:, 0].min()), float(pos[:, 0].max())
    step = (hi - lo) / njoints
    base, extents = [lo, 0.0, float(pos[:, 2].mean())], [[step, 0, 0]] * njoints
    joints = SC.chain(base, extents, [5.0 * step] * njoints)
    frames = [SC.chain_posed(base, extents, [[3 * np.sin(0.7 * f + j), 0, 5 * np.cos(0.4 * f + 0.5 * j)] for j in range(njoints)]) for f in range(4)]
    return joints, frames


def timed(call, sync):
    t0 = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t0) * 1e3


def main(frames, njoints):
    import torch

    pos, nrm, idx = beast()
    S = scenes.cornell_with_mesh(3, "glass")
    S["objects"][6] = dict(S["objects"][6], pos=pos, nrm=nrm, idx=idx)
    joints, poses = rig(pos, njoints)
    dev, host = srt_amd.Pathtracer(0), srt_amd.Pathtracer(0)
    for pt in (dev, host):
        pt.set_params(64, 64, 1, 8, True)
        pt.build_scene(S)
    t0 = time.perf_counter()
    skin = dev.create_skin(6, pos, nrm, joints)
    create_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    _, _, _, inside, Wm = E.find_joints(pos, joints)
    host_find_ms = (time.perf_counter() - t0) * 1e3
    d_pos, d_nrm = torch.empty(pos.shape, dtype=torch.float32, device="cuda"), torch.empty(pos.shape, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    for k in (0, 1):                                        # warm-up: code objects, the builder's workspace, the staging
        skin.pose(poses[k])
        host.update_mesh(6, E.skin(pos, joints, poses[k], inside, Wm), nrm)
        skin.vertices_device(poses[k], d_pos.data_ptr(), d_nrm.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    t_pose, t_kern, t_host_skin, t_host_update = [], [], [], []
    for f in range(frames):
        posed = poses[f % len(poses)]
        t_pose.append(timed(lambda: skin.pose(posed), dev.sync))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        skin.vertices_device(posed, d_pos.data_ptr(), d_nrm.data_ptr(), stream=stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        t_kern.append(a.elapsed_time(b))
        t0 = time.perf_counter()
        p = E.skin(pos, joints, posed, inside, Wm)
        t_host_skin.append((time.perf_counter() - t0) * 1e3)
        t_host_update.append(timed(lambda: host.update_mesh(6, p, nrm), host.sync))
    got = skin.vertices(poses[(frames - 1) % len(poses)])[0]
    med = statistics.median
    out = {"mesh": "mesh_beast", "vertices": len(pos), "triangles": len(idx) // 3, "joints": njoints, "influences": skin.counts()["influences"], "frames": frames,
           "device_equals_host_bits": bool(np.array_equal(got.view(np.uint32), p.view(np.uint32))),
           "skin_create_ms": create_ms, "host_find_joints_ms": host_find_ms,
           "pose_wall_ms_median": med(t_pose), "pose_wall_ms_min": min(t_pose), "pose_wall_ms_max": max(t_pose),
           "skin_kernels_device_ms_median": med(t_kern), "skin_kernels_device_ms_min": min(t_kern), "skin_kernels_device_ms_max": max(t_kern),
           "host_skin_ms_median": med(t_host_skin), "host_update_mesh_ms_median": med(t_host_update),
           "host_route_ms_median": med([x + y for x, y in zip(t_host_skin, t_host_update)]),
           "host_route_over_pose": med([x + y for x, y in zip(t_host_skin, t_host_update)]) / med(t_pose),
           "pose_wall_ms": t_pose, "host_skin_ms": t_host_skin, "host_update_mesh_ms": t_host_update}
    skin.close(); dev.close(); host.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 9, int(sys.argv[2]) if len(sys.argv) > 2 else 8)
