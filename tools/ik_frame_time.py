"""Per-frame time of a rig driven by IK handles: the whole frame on the device against the frame a caller had before the device form
existed, both in this process, after a warm-up:

  step_ik_device -> pose_current("inplace") -> render_epoch_device        one stream, no host wait, nothing uploaded
  against
  Skeleton::do_ik on the CPU (srt_pt_rig_step_ik_host) + joint_to_posed on the CPU (srt_pt_rig_posed_host)
  + Skin.pose_inplace(posed) -> render_epoch_device                      64 B per joint go up

on the three-joint rig through the blob of cbox+blob512 (tests/golden/ik_blob_chain3.npz) and on tests/golden/mesh_beast.npz (32 311
vertices) with a generated chain of 24 joints along x and three handles.  The targets alternate between two sets that are resident
in device memory; both routes start from the same pose and see the same targets, so they walk through the same poses.

Per frame two figures: the host time until the frame is enqueued, and the whole frame with one synchronise at the end.  A third
case times the kernel alone (HIP events around step_ik_device) on the recorded rigs: blob_chain3 and blob128_tree5 keep their joints in
LDS, deep262 (262 joints) in device scratch.  Medians with min .. max; one JSON line per case, appended to the file given
(profiles/ik_frame_time.jsonl holds a run, DESIGN.md quotes it).  Asserts nothing; "same_image" and "same_pose" record whether both
routes ended on the same bits.

    python tools/ik_frame_time.py [frames = 31] [out = profiles/ik_frame_time.jsonl]"""
import ctypes
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

import _harness as H  # noqa: E402
import _ik_cases as IK  # noqa: E402
import _skin_cases as SC  # noqa: E402
import _update_cases as UC  # noqa: E402
from skin_frame_time import beast  # noqa: E402

F = np.float32
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
    """(host ms until the frame's pose work is enqueued, ms of the whole frame) per frame: call(f, stream), render_epoch_device, one synchronise."""
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


def rig_case(torch, name, S, obj, pos, nrm, joints, rig, extent, handles, targets, frames):
    """rig: srt_pt_skin_set_rig's arguments (no keys are needed); targets: two sets, (2, nhandles, 3)."""
    lib = srt_amd.load_library()
    parent, base, rest = np.ascontiguousarray(rig[0], np.int32), np.ascontiguousarray(rig[1], F), np.ascontiguousarray(rig[2], F)
    nj, hj = len(parent), np.ascontiguousarray(handles, np.uint32)
    extent, targets = np.ascontiguousarray(extent, F), np.ascontiguousarray(targets, F)
    no_keys = (np.zeros(nj + 1, np.uint32), np.zeros(1, F), np.zeros((1, 4), F))
    out = {"case": name, "vertices": len(pos), "joints": nj, "handles": len(hj), "frames": frames}
    images, poses = {}, {}
    # the device route
    pt = make_pt(S)
    skin = pt.create_skin(obj, pos, nrm, joints)
    skin.set_rig(*rig)
    skin.set_ik_handles(hj)
    d_targets = [torch.from_numpy(t).to("cuda:0") for t in targets]

    def device_frame(f, s):
        skin.step_ik_device(d_targets[f % 2].data_ptr(), 0, s)
        skin.pose_current("inplace", False, s)

    inside, whole, images["device"] = frames_of(torch, pt, device_frame, frames)
    poses["device"] = skin.joint_pose()
    out["device"] = {"enqueue_host_ms": spread(inside), "frame_ms": spread(whole), "enqueue_host_ms_all": inside, "frame_ms_all": whole}
    skin.close(); pt.close()
    # the host route: do_ik and joint_to_posed on the CPU, the matrices uploaded
    pt = make_pt(S)
    skin = pt.create_skin(obj, pos, nrm, joints)
    pose, posed = rest.copy(), np.zeros((nj, 16), F)
    cpu = []

    def host_frame(f, s):
        t0 = time.perf_counter()
        t = targets[f % 2]
        lib.srt_pt_rig_step_ik_host(nj, H.P(parent), H.P(extent), H.P(pose), H.P(hj), H.P(t), None, len(hj), 1)
        lib.srt_pt_rig_posed_host(nj, H.P(parent), H.P(extent), H.P(base), H.P(pose), H.P(no_keys[0]), H.P(no_keys[1]), H.P(no_keys[2]), ctypes.c_float(0.0), None, H.P(posed))
        cpu.append((time.perf_counter() - t0) * 1e3)
        skin.pose_inplace(posed, False, s)

    inside, whole, images["host"] = frames_of(torch, pt, host_frame, frames)
    poses["host"] = pose.copy()
    out["host"] = {"enqueue_host_ms": spread(inside), "frame_ms": spread(whole), "cpu_ik_ms": spread(cpu[-frames:]), "enqueue_host_ms_all": inside, "frame_ms_all": whole}
    skin.close(); pt.close()
    out["same_image"] = bool(np.array_equal(images["device"].view(np.uint32), images["host"].view(np.uint32)))
    out["same_pose"] = bool(np.array_equal(poses["device"].view(np.uint32), poses["host"].view(np.uint32)))
    return out


def blob_case(torch, frames):
    S = UC.blob_scene()
    g, joints = SC.load_fixture("blob_chain3")
    ik = IK.load("blob_chain3")
    rig = IK.rig_arrays(ik)
    nj = len(ik["parent"])
    rig = (rig[0], rig[1], rig[2], np.zeros(nj + 1, np.uint32), np.zeros(1, F), np.zeros((1, 4), F))
    return rig_case(torch, "cbox+blob512, blob_chain3", S, UC.BLOB_OBJECT, g["pos"], g["nrm"], joints, rig, ik["extent"], ik["handle_joints"],
                    np.stack([ik["targets"][0], ik["targets"][1]]), frames)


def beast_case(torch, frames, njoints=24):
    pos, nrm, idx = beast()
    S = scenes.cornell_with_mesh(3, "glass")
    S["objects"][6] = dict(S["objects"][6], pos=pos, nrm=nrm, idx=idx)
    lo, hi = float(pos[:, 0].min()), float(pos[:, 0].max())
    step = (hi - lo) / njoints
    base, extents = [lo, 0.0, float(pos[:, 2].mean())], [[step, 0, 0]] * njoints
    joints = SC.chain(base, extents, [5.0 * step] * njoints)
    rig = (np.arange(-1, njoints - 1, dtype=np.int32), base, np.zeros((njoints, 3), F), np.zeros(njoints + 1, np.uint32), np.zeros(1, F), np.zeros((1, 4), F))
    handles = [njoints - 1, njoints // 2, njoints // 4]
    span = hi - lo
    targets = np.array([[[span, 0.2 * span, 0.1 * span], [0.5 * span, -0.1 * span, 0.0], [0.25 * span, 0.1 * span, 0.0]],
                        [[span, -0.2 * span, -0.1 * span], [0.5 * span, 0.1 * span, 0.05 * span], [0.25 * span, -0.1 * span, 0.0]]], F)
    return rig_case(torch, "mesh_beast, chain of 24", S, 6, pos, nrm, joints, rig, extents, handles, targets, frames)


def kernel_case(torch, frames):
    """Device time of one step_ik_device launch (50 iterations) per recorded rig, by HIP events on the null stream."""
    out = {"case": "step_ik_device alone, HIP events", "frames": frames, "rigs": {}}
    for name in IK.RIGS:
        ik = IK.load(name)
        if name in IK.MESHED:
            g, joints = SC.load_fixture(name)
            pos, nrm, idx = g["pos"], g["nrm"], g["idx"]
        else:
            pos, nrm, idx = SC.small_blob_mesh()
            joints = IK.skin_joints(ik)
        pt = srt_amd.Pathtracer(0)
        pt.set_params(8, 8, 1, 4, True)
        pt.build_scene(SC.single_mesh_scene(pos, nrm, idx))
        skin = pt.create_skin(0, pos, nrm, joints)
        skin.set_rig(*IK.rig_arrays(ik))
        skin.set_ik_handles(ik["handle_joints"])
        d_t = torch.from_numpy(np.ascontiguousarray(ik["targets"][0], F)).to("cuda:0")
        torch.cuda.synchronize()
        ms = []
        for f in range(-3, frames):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            skin.step_ik_device(d_t.data_ptr())
            b.record()
            b.synchronize()
            if f >= 0:
                ms.append(a.elapsed_time(b))
        out["rigs"][name] = {"joints": len(ik["parent"]), "handles": len(ik["handle_joints"]), "in_lds": len(ik["parent"]) <= IK.LDS_JOINTS, "kernel_ms": spread(ms),
                             "kernel_ms_all": ms}
        skin.close(); pt.close()
    return out


def main(frames, path):
    import torch

    lines = [blob_case(torch, frames), beast_case(torch, frames), kernel_case(torch, frames)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 31, sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ik_frame_time.jsonl"))
