"""Records tests/golden/ik_<name>.npz: what the reference's own Skeleton::set_time, Skeleton::do_ik / step_ik / Joint::compute_gradient,
Skeleton::joint_to_posed and Scene_Object::posed_mesh compute for the rigs, handles and targets of tests/_ik_cases.py.
Runs only where the reference is (integration/_build/libdropin_pt_full.so, harness/ik_ref.cpp):  python tests/golden/make_ik_golden.py [name ...]
The files hold data only: the rig that went in, in Skeleton::for_joints order (parents first); the handles' joints, targets and
enabled flags in the order do_ik visited the handles; and per call every joint's pose before and after do_ik, after the last call
joint_to_posed per joint and - for the two rigs of tests/_skin_cases.rigs() - posed_mesh()'s vertices.  Those two are stored in the
joint order of the committed skin_<name>.npz, so that a skin made from that fixture takes them as they are.  Every case the tests
rely on is asserted here, on the recorded values."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _anim_cases as AC  # noqa: E402
import _harness as H  # noqa: E402
import _ik_cases as IK  # noqa: E402

F = np.float32


def run_reference(lib, case):
    nj, nh, K = len(case["parent"]), len(case["handles"]), len(case["targets"])
    if "mesh" in case:
        pos, nrm, idx = (np.ascontiguousarray(a, t) for a, t in zip(case["mesh"](), (F, F, np.uint32)))
    else:
        pos, nrm, idx = np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, np.uint32)
    nv = len(pos)
    parent, extent, radius, base = np.array(case["parent"], np.int32), np.array(case["extent"], F), np.array(case["radius"], F), np.array(case["base"], F)
    rest = np.array(case["rest"], F)
    offs, times, quats = [0], [], []
    for j in range(nj):
        ts, qs = case["keys"].get(j, ([], []))
        times.extend(ts)
        quats.extend(qs)
        offs.append(len(times))
    offs, times, quats = np.array(offs, np.uint32), np.array(times + [0.0], F), np.array(quats + [[0, 0, 0, 1]], F).reshape(-1, 4)
    hj, targets, enabled = np.array(case["handles"], np.uint32), np.array(case["targets"], F), np.array(case["enabled"], np.uint8)
    set_times = np.array(case["set_times"], F)
    assert targets.shape == (K, nh, 3) and enabled.shape == (K, nh) and set_times.shape == (K,)
    order, horder = np.zeros(nj, np.uint32), np.zeros(nh, np.uint32)
    before, after, did = np.zeros((K, nj, 3), F), np.zeros((K, nj, 3), F), np.zeros(K, np.uint8)
    posed, mesh = np.zeros((nj, 16), F), np.zeros((max(nv, 1), 3), F)
    st = lib.dropin_ik_reference(H.P(pos), H.P(nrm), nv, H.P(idx), len(idx), H.P(parent), H.P(extent), H.P(radius), H.P(rest), nj, H.P(base), H.P(offs),
                                 H.P(times), H.P(quats), H.P(hj), nh, H.P(targets), H.P(enabled), H.P(set_times), K, H.P(order), H.P(horder), H.P(before),
                                 H.P(after), H.P(did), H.P(posed), H.P(mesh))
    assert st == 0
    return {"pos": pos, "order": order, "horder": horder, "before": before, "after": after, "did": did, "posed": posed, "mesh": mesh[:nv],
            "offs": offs, "times": times[:-1], "quats": quats[:-1]}


def record(lib, srt_lib, name, case):
    skin = np.load(os.path.join(HERE, f"skin_{name}.npz")) if name in IK.MESHED else None
    keep = []
    for attempt in range(200):
        r = run_reference(lib, case)
        # the skinned vertices depend on the order Skeleton::for_joints visits the joints in (children hang in an unordered_set of
        # pointers): they are only good for a skin in the committed fixture's order when this run visited the joints in that order
        if skin is None or np.array_equal(r["order"], skin["order"]):
            break
        keep.append(ctypes.create_string_buffer(16 * (attempt + 1)))     # (moves the next run's allocations)
    else:
        raise SystemExit(f"{name}: for_joints order {r['order']} never came out as the committed skin fixture's {skin['order']} - run again")
    order, horder = r["order"], r["horder"]
    nj, nh = len(order), len(horder)
    parent, extent = np.array(case["parent"], np.int32), np.array(case["extent"], F)
    inv = np.zeros(nj, np.int64)
    inv[order] = np.arange(nj)
    parent_fo = np.array([-1 if parent[j] < 0 else inv[parent[j]] for j in order], np.int32)
    assert all(p < k for k, p in enumerate(parent_fo))                                 # parents come first
    if skin is not None:
        assert np.array_equal(r["pos"], skin["pos"]) and np.array_equal(extent[order], skin["extent"])
    knot_offsets, ktimes, kquats = [0], [], []
    for j in order:
        ktimes.extend(r["times"][r["offs"][j]:r["offs"][j + 1]])
        kquats.extend(r["quats"][r["offs"][j]:r["offs"][j + 1]])
        knot_offsets.append(len(ktimes))
    g = {"order": order, "handle_order": horder, "parent": parent_fo, "extent": extent[order], "radius": np.array(case["radius"], F)[order],
         "base": np.array(case["base"], F), "rest_pose": np.array(case["rest"], F)[order], "knot_offsets": np.array(knot_offsets, np.uint32),
         "knot_times": np.array(ktimes, F), "knot_quats": np.array(kquats, F).reshape(-1, 4),
         "handle_joints": inv[np.array(case["handles"])[horder]].astype(np.uint32), "targets": np.array(case["targets"], F)[:, horder],
         "enabled": np.array(case["enabled"], np.uint8)[:, horder], "set_times": np.array(case["set_times"], F),
         "pose_before": r["before"], "pose": r["after"], "did": r["did"], "posed": r["posed"]}
    if skin is not None:
        g["mesh_pos"] = r["mesh"]
    check(srt_lib, name, g)
    path = os.path.join(HERE, f"ik_{name}.npz")
    np.savez_compressed(path, **g)
    moved = np.abs(g["pose"] - g["pose_before"]).max(axis=2).sum(axis=0)
    print(name, "joints", nj, "handles", g["handle_joints"], "order", horder, "calls", len(g["targets"]), "max angle", float(np.abs(g["pose"]).max()),
          "least movement in a chain", float(moved[moved > 0].min()), os.path.getsize(path), "bytes")


def check(srt_lib, name, g):
    """What the fixture must contain (tests/test_pt_ik_host.py asserts the same on the committed files)."""
    K, nj = g["pose"].shape[:2]
    chains = IK.chains(g["parent"], g["handle_joints"])
    assert np.isfinite(g["pose"]).all() and np.isfinite(g["pose_before"]).all() and np.isfinite(g["posed"]).all()
    assert np.abs(g["pose"]).max() < 1000 and np.abs(g["pose_before"]).max() < 1000
    reached = np.zeros(nj, bool)
    for c in range(K):
        assert bool(g["did"][c]) == bool(g["enabled"][c].any())
        for h, chain in enumerate(chains):
            if g["enabled"][c][h]:
                reached[chain] = True
    moved = np.abs(g["pose"] - g["pose_before"]).max(axis=2).sum(axis=0)               # degrees, summed over the calls
    assert reached.any() and np.all(moved[reached] > IK.LEAST_MOVED.get(name, 1.0)), (name, moved[reached].min())
    keyed = np.diff(g["knot_offsets"].astype(np.int64)) > 0
    later = [c for c in range(1, K) if np.isfinite(g["set_times"][c])]                # (a later set_time moves keyed joints outside do_ik)
    assert np.all(moved[~reached] == 0)                                               # do_ik leaves the others' bits alone
    assert all(np.array_equal(g["pose_before"][c][~keyed], g["pose"][c - 1][~keyed]) for c in later)
    if name == "blob_chain3":
        keyed = np.diff(g["knot_offsets"]) > 0
        assert 0 < keyed.sum() < nj and np.isfinite(g["set_times"]).any() and np.isnan(g["set_times"]).any()
        assert list(g["handle_joints"]) == [nj - 1] and len(chains[0]) == 3           # one handle, on the tip
        c = int(np.nonzero(np.isfinite(g["set_times"]))[0][1])                         # a later set_time: unkeyed joints keep IK's pose
        assert np.array_equal(g["pose_before"][c][~keyed], g["pose"][c - 1][~keyed]) and not np.array_equal(g["pose_before"][c][keyed], g["pose"][c - 1][keyed])
    if name == "blob128_tree5":
        hj, par = list(g["handle_joints"]), g["parent"]
        assert (par < 0).sum() == 2
        assert len(hj) != len(set(hj))                                                # two handles on one joint
        assert any(par[j] < 0 for j in hj)                                            # a handle on a root: a chain of one
        sets = [set(c) for c in chains]
        assert any(sets[a] & sets[b] and hj[a] not in sets[b] and hj[b] not in sets[a] for a in range(len(hj)) for b in range(a))   # branches that share an ancestor
        assert any(not e.any() for e in g["enabled"]) and any(e.any() and not e.all() for e in g["enabled"])
        assert np.array_equal(g["pose"][1], g["pose_before"][1]) or g["enabled"][1].any()
    if name in ("blob128_tree5", "wide200"):
        # the fixture can tell a wrong summation order: the handle list reversed gives other bits
        c = 0
        _, fwd = IK.step_host(srt_lib, g["parent"], g["extent"], g["pose_before"][c], g["handle_joints"], g["targets"][c], g["enabled"][c])
        _, rev = IK.step_host(srt_lib, g["parent"], g["extent"], g["pose_before"][c], g["handle_joints"][::-1], g["targets"][c][::-1], g["enabled"][c][::-1])
        assert AC.bits_equal(fwd, g["pose"][c]) and not AC.bits_equal(rev, g["pose"][c])
    if name == "deep262":
        assert nj > IK.BLOCK and nj > IK.LDS_JOINTS and max(len(c) for c in chains) >= 20 and len(chains) >= 3
    if name == "wide200":
        IK.check_wide(g)


def main():
    import srt_amd

    lib = ctypes.CDLL(os.path.join(ROOT, "integration", "_build", "libdropin_pt_full.so"))
    srt_lib = srt_amd.load_library()
    for name, case in IK.cases().items():
        if len(sys.argv) == 1 or name in sys.argv[1:]:                                 # (names as arguments: only those are recorded)
            record(lib, srt_lib, name, case)


if __name__ == "__main__":
    main()
