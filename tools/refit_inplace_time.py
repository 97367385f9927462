"""Per-frame time of a deforming mesh through the enqueue-only in-place refit against the blocking refit it stands beside, both in
this process, after a warm-up:

  refit_mesh_inplace_device  against  refit_mesh_device      object 6 of cornell_with_mesh(3) (512 triangles) and of
                                                            cornell_with_mesh(7) (131 072 triangles), two deformations alternating,
                                                            the vertices resident in device memory
  Skin.pose_inplace_at       against  Skin.pose_refit_at     tests/golden/mesh_beast.npz (32 311 vertices, 64 618 triangles) in the
                                                            Cornell box with a generated, keyed chain of joints along x

Per frame two figures: the host time inside the call, and the whole frame - the call, render_epoch_device on the same stream, one
synchronise at the end.  Medians with min .. max; one JSON line per case, appended to the file given (profiles/refit_inplace_time.jsonl
holds a run, DESIGN.md quotes it).  The last line has the SAH cost of the BVH<Object> kept against rebuilt after the largest
deformation.  Asserts nothing; "same_image" records whether both routes left the same last frame, bit for bit.

    python tools/refit_inplace_time.py [frames = 31] [out = profiles/refit_inplace_time.jsonl]"""
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

import _anim_cases as AC  # noqa: E402
import _skin_cases as SC  # noqa: E402
import _update_cases as UC  # noqa: E402
from skin_frame_time import beast  # noqa: E402

W = HT = 64
SPP = 1


def make_pt(S):
    pt = srt_amd.Pathtracer(0)
    pt.set_params(W, HT, 1, 8, True)
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    return pt


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def frames_of(torch, pt, call, frames, warm=3):
    """(host ms inside the call, ms of the whole frame) per frame: call(f, stream), render_epoch_device, one synchronise."""
    local_tiles, _, floats_per_tile = pt.tile_info()
    tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
    image = torch.zeros(HT * W * 3, device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    inside, whole = [], []
    for f in range(-warm, frames):
        t0 = time.perf_counter()
        call(f, st.cuda_stream)
        t1 = time.perf_counter()
        pt.render_epoch_device(st.cuda_stream, 9, 0, SPP, tiles.data_ptr())
        pt.untile_device(st.cuda_stream, tiles.data_ptr(), image.data_ptr())
        st.synchronize()
        t2 = time.perf_counter()
        if f >= 0:
            inside.append((t1 - t0) * 1e3)
            whole.append((t2 - t0) * 1e3)
    return inside, whole, image.cpu().numpy()


def mesh_case(torch, level, frames):
    S = scenes.cornell_with_mesh(level, "glass")
    D = [UC.blob_arrays(level, seed=s)[:2] for s in (11, 12)]
    keep = [(torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda()) for p, n in D]
    nverts = len(D[0][0])
    out = {"case": f"cornell_with_mesh({level}) object 6", "vertices": nverts, "triangles": len(S["objects"][6]["idx"]) // 3, "frames": frames}
    images = {}
    for name in ("refit_mesh_inplace_device", "refit_mesh_device"):
        pt = make_pt(S)
        fn = getattr(pt, name)
        inside, whole, images[name] = frames_of(torch, pt, lambda f, s: fn(6, keep[f % 2][0].data_ptr(), keep[f % 2][1].data_ptr(), nverts, s), frames)
        out[name] = {"call_host_ms": spread(inside), "frame_ms": spread(whole), "call_host_ms_all": inside, "frame_ms_all": whole}
        out[name]["scene_tree_cost"], out[name]["mesh_tree_cost"] = pt.scene_tree_cost(), pt.mesh_tree_cost(6)
        pt.close()
    out["same_image"] = bool(np.array_equal(images["refit_mesh_inplace_device"].view(np.uint32), images["refit_mesh_device"].view(np.uint32)))
    return out


def skin_case(torch, frames, njoints=8):
    pos, nrm, idx = beast()
    S = scenes.cornell_with_mesh(3, "glass")
    S["objects"][6] = dict(S["objects"][6], pos=pos, nrm=nrm, idx=idx)
    lo, hi = float(pos[:, 0].min()), float(pos[:, 0].max())
    step = (hi - lo) / njoints
    base, extents = [lo, 0.0, float(pos[:, 2].mean())], [[step, 0, 0]] * njoints
    joints = SC.chain(base, extents, [5.0 * step] * njoints)
    times = np.arange(4, dtype=np.float32)
    quats = np.array([AC.quat_of_euler([3 * np.sin(0.7 * f + j), 0, 5 * np.cos(0.4 * f + 0.5 * j)]) for j in range(njoints) for f in range(4)], np.float32)
    rig = (np.arange(-1, njoints - 1, dtype=np.int32), base, np.zeros((njoints, 3), np.float32), np.arange(0, 4 * njoints + 1, 4, dtype=np.uint32),
           np.tile(times, njoints), quats)
    out = {"case": "mesh_beast skin", "vertices": len(pos), "triangles": len(idx) // 3, "joints": njoints, "frames": frames}
    images = {}
    for name in ("pose_inplace_at", "pose_refit_at"):
        pt = make_pt(S)
        skin = pt.create_skin(6, pos, nrm, joints)
        skin.set_rig(*rig)
        fn = getattr(skin, name)
        inside, whole, images[name] = frames_of(torch, pt, lambda f, s: fn(0.25 + 0.375 * (f % 8), False, s), frames)
        out[name] = {"call_host_ms": spread(inside), "frame_ms": spread(whole), "call_host_ms_all": inside, "frame_ms_all": whole}
        out[name]["scene_tree_cost"] = pt.scene_tree_cost()
        skin.close(); pt.close()
    out["same_image"] = bool(np.array_equal(images["pose_inplace_at"].view(np.uint32), images["pose_refit_at"].view(np.uint32)))
    return out


def tree_costs():
    """The BVH<Object> kept against rebuilt after the largest deformation of the 512-triangle blob (UC.deformations()' D2 scales it)."""
    S = UC.blob_scene()
    costs = {}
    for name, (p, n) in UC.deformations().items():
        kept, rebuilt = make_pt(S), make_pt(S)
        kept.refit_mesh_inplace(UC.BLOB_OBJECT, p, n)
        rebuilt.refit_mesh(UC.BLOB_OBJECT, p, n)
        costs[name] = {"kept": kept.scene_tree_cost(), "rebuilt": rebuilt.scene_tree_cost()}
        kept.close(); rebuilt.close()
    return {"case": "scene_tree_cost of cbox+blob512, BVH<Object> kept / rebuilt", "costs": costs}


def main(frames, path):
    import torch

    lines = [mesh_case(torch, 3, frames), mesh_case(torch, 7, frames), skin_case(torch, frames), tree_costs()]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 31, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "refit_inplace_time.jsonl"))
