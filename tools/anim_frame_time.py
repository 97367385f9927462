"""Frame time and upload of an animated frame with the keys evaluated on the device (srt_pt_timeline_*, srt_pt_skin_pose_refit_at)
against the same frame with the keys evaluated on the host, on the GPU.

Objects: N posed copies of blob_mesh(3) (the pool of tools/repose_device_time.py: one mesh, N - 1 instances, a jittered grid of pitch 1),
every instance with six position keys around its cell, six rotation keys and six scale keys at uneven times.  Two loops over the same
times, one stream, synchronised once after the last frame; the host clock around the whole loop divided by the frames is the frame
time, a second clock around the scene calls alone gives the host time inside them:
  host keys      transforms on the host from the same keys (srt_pt_timeline_transforms: the reference's arithmetic, one core) -> a
                 pinned tensor -> 64 B per object up -> repose_refit_device -> a 1-spp epoch at 64x64       [what a caller did before]
  device keys    Timeline.repose_refit(t) -> the same epoch
Rig: cbox+blob512 with the committed three-joint chain and its recorded keys (tests/golden): posed_at(t) on the host ->
pose_refit(posed), against pose_refit_at(t); both wait inside the refit (its verdict), so this pair compares the 64 B per joint and
the host arithmetic only (3000 frames per run: half a second).  Then the new kernels alone: events around 50000 back-to-back
launches (half a second per run) give the time per launch of a saturated stream - launch throughput, an upper bound of the
kernel's duration; the duration itself comes from a profiler run of its own over the `kernels` mode, which only launches them:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/anim_frame_time.py 4096 200 1 kernels
Bytes are the context's upload counter (plus the transforms' own copy in the host-keys loop).  Prints JSON lines; DESIGN.md records a run.

    python tools/anim_frame_time.py [N = 4096] [frames = 200] [runs = 3] [kernels]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from repose_device_time import scene, transforms  # noqa: E402  (also puts the package on the path)
import srt_amd  # noqa: E402

TESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
KNOTS = np.array([0.0, 0.5, 1.25, 2.0, 3.5, 4.0], np.float32)


def keys(T0, seed):
    """track_offsets, knot_times, knot_values for every row of T0: positions within 0.2 of the cell, unit quaternions, scales 0.8 .. 1.2."""
    rng = np.random.default_rng(seed)
    n, k = len(T0), len(KNOTS)
    values = np.zeros((n, 3, k, 4), np.float32)
    values[:, 0, :, :3] = T0[:, None, 12:15] + (rng.random((n, k, 3)) - 0.5) * 0.4
    q = rng.normal(size=(n, k, 4))
    values[:, 1] = q / np.linalg.norm(q, axis=2, keepdims=True)
    values[:, 2, :, :3] = 0.8 + 0.4 * rng.random((n, k, 3))
    return np.arange(3 * n + 1, dtype=np.uint32) * k, np.tile(KNOTS, 3 * n), values.reshape(-1, 4)


def context(S):
    pt = srt_amd.Pathtracer(0)
    pt.set_params(64, 64, 1, 8, True)
    pt.build_scene(S)
    pt.set_camera(S["camera"])
    return pt


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main(n, frames, runs, kernels_only=False):
    import torch

    T0 = transforms(n, 1)
    S = scene(n, T0)
    idx = np.arange(1, n + 1, dtype=np.uint32)
    tracks = keys(T0, 4)
    times = [float(t) for t in np.linspace(-0.25, 4.25, frames)]
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    pinned = [torch.zeros((n, 16)).pin_memory() for _ in range(frames)]     # one per frame: a copy in flight is not overwritten
    d_T = torch.zeros((n, 16), device="cuda:0")

    def loop(pt, tl, tiles, device_keys, ts):
        inside = 0.0
        t0 = time.perf_counter()
        with torch.cuda.stream(st):
            for f, t in enumerate(ts):
                c0 = time.perf_counter()
                if device_keys:
                    tl.repose_refit(t, s)
                else:
                    pinned[f].numpy()[:] = tl.transforms(t)
                    d_T.copy_(pinned[f], non_blocking=True)
                    pt.repose_refit_device(idx, d_T.data_ptr(), s)
                inside += time.perf_counter() - c0
                pt.render_epoch_device(s, 9, f, 1, tiles.data_ptr())
        st.synchronize()
        return time.perf_counter() - t0, inside

    out = {"instances": n, "frames": frames, "runs": runs, "knots_per_track": len(KNOTS)}
    for name, device_keys in (() if kernels_only else (("host_keys", False), ("device_keys", True), ("host_keys_again", False), ("device_keys_again", True))):
        frame_ms, inside_ms, up = [], [], []
        for r in range(runs):
            pt = context(S)
            tl = pt.create_timeline(idx, tracks)
            local_tiles, _, floats_per_tile = pt.tile_info()
            tiles = torch.zeros(local_tiles * floats_per_tile, device="cuda:0")
            torch.cuda.synchronize()
            loop(pt, tl, tiles, device_keys, times[:2])    # warm-up: code objects, the refit's tables, the list
            b0 = pt.scene_counts()["uploaded_bytes"]
            total, inside = loop(pt, tl, tiles, device_keys, times)
            up.append((pt.scene_counts()["uploaded_bytes"] - b0) / frames + (0 if device_keys else 64 * n))
            frame_ms.append(total / frames * 1e3)
            inside_ms.append(inside / frames * 1e3)
            tl.close(); pt.close()
        out[name] = {"frame_ms": summary(frame_ms), "host_ms_in_the_scene_calls": summary(inside_ms), "bytes_up_per_frame": summary(up)}
    if not kernels_only:
        out["frame_time_ratio_host_over_device"] = out["host_keys"]["frame_ms"]["median"] / out["device_keys"]["frame_ms"]["median"]
        print(json.dumps(out), flush=True)

    # the device time of the pose kernel alone
    pt = context(S)
    tl = pt.create_timeline(idx, tracks)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(20):
        tl.transforms_device(1.0, d_T.data_ptr())
    torch.cuda.synchronize()
    reps, per_launch = (2000 if kernels_only else 50000), []
    for r in range(runs):
        e0.record()
        for k in range(reps):
            tl.transforms_device(times[k % len(times)], d_T.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        per_launch.append(e0.elapsed_time(e1) / reps * 1e3)
    tl.close(); pt.close()
    print(json.dumps({"anim_pose_kernel": {"objects": n, "back_to_back_launches": reps, "us_per_launch": summary(per_launch)}}), flush=True)

    # the rig: cbox+blob512, the committed chain of three and its recorded keys
    sys.path.insert(0, TESTS)
    import _anim_cases as AC
    import _skin_cases as SC
    import _update_cases as UC

    B = UC.blob_scene()
    g, joints = SC.load_fixture("blob_chain3")
    rig = AC.load_rig("blob_chain3")
    rig_frames = 15 * frames
    rts = [float(t) for t in np.linspace(-0.25, 4.25, rig_frames)]
    res = {"joints": len(joints), "vertices": len(g["pos"]), "frames": rig_frames}
    for name, device_keys in (() if kernels_only else (("host_matrices", False), ("device_matrices", True))):
        frame_ms, up = [], []
        for r in range(runs):
            pt = context(B)
            skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints)
            skin.set_rig(*[rig[k] for k in ("parent", "base", "rest_pose", "knot_offsets", "knot_times", "knot_quats")])
            call = (lambda t: skin.pose_refit_at(t)) if device_keys else (lambda t: skin.pose_refit(skin.posed_at(t)))
            call(rts[0]); call(rts[1])
            b0 = pt.scene_counts()["uploaded_bytes"]
            t0 = time.perf_counter()
            for t in rts:
                call(t)
            pt.sync()
            frame_ms.append((time.perf_counter() - t0) / rig_frames * 1e3)
            up.append((pt.scene_counts()["uploaded_bytes"] - b0) / rig_frames)
            skin.close(); pt.close()
        res[name] = {"frame_ms": summary(frame_ms), "bytes_up_per_frame": summary(up)}
    pt = context(B)
    skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints)
    skin.set_rig(*[rig[k] for k in ("parent", "base", "rest_pose", "knot_offsets", "knot_times", "knot_quats")])
    d_posed = torch.zeros((len(joints), 16), device="cuda:0")
    for _ in range(20):
        skin.posed_at_device(1.0, d_posed.data_ptr())
    torch.cuda.synchronize()
    per_call = []
    for r in range(runs):
        e0.record()
        for k in range(reps):
            skin.posed_at_device(rts[k % len(rts)], d_posed.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        per_call.append(e0.elapsed_time(e1) / reps * 1e3)
    skin.close(); pt.close()
    res["anim_joint_kernels_us_per_call_of_two_launches"] = summary(per_call)
    print(json.dumps({"rig": res}), flush=True)


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:] if x != "kernels"]
    main(a[0] if len(a) > 0 else 4096, a[1] if len(a) > 1 else 200, a[2] if len(a) > 2 else 3, "kernels" in sys.argv[1:])
