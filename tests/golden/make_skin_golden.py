"""Records tests/golden/skin_<name>.npz: what the reference's own Skeleton computes for the rigs of tests/_skin_cases.rigs().
Runs only where the reference is (integration/_build/libdropin_pt_full.so, harness/skin_ref.cpp):  python tests/golden/make_skin_golden.py
The files hold data only: the mesh, the joints in Skeleton::for_joints order (joint_to_bind, extent, radius), and per pose
joint_to_posed, the vertex_joints lists as CSR and posed_mesh()'s vertices with and without opt.smooth_normals."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _harness as H  # noqa: E402
import _skin_cases as SC  # noqa: E402

F = np.float32


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "integration", "_build", "libdropin_pt_full.so"))
    lib.dropin_skin_reference.restype = ctypes.c_long
    for name, rig in SC.rigs().items():
        pos, nrm, idx = rig["mesh"]()
        pos, nrm, idx = np.ascontiguousarray(pos, F), np.ascontiguousarray(nrm, F), np.ascontiguousarray(idx, np.uint32)
        nv, nj = len(pos), len(rig["parent"])
        parent, extent, radius, base = np.array(rig["parent"], np.int32), np.array(rig["extent"], F), np.array(rig["radius"], F), np.array(rig["base"], F)
        out = {"pos": pos, "nrm": nrm, "idx": idx, "posed": [], "smooth_pos": [], "smooth_nrm": [], "flat_pos": [], "flat_nrm": []}
        for angles in rig["poses"]:
            pose = np.array(angles, F)
            order, bind, posed = np.zeros(nj, np.uint32), np.zeros((nj, 16), F), np.zeros((nj, 16), F)
            off, jidx = np.zeros(nv + 1, np.uint32), np.zeros(nv * nj, np.uint32)
            sp, sn, fp, fn = (np.zeros((nv, 3), F) for _ in range(4))
            n = lib.dropin_skin_reference(H.P(pos), H.P(nrm), nv, H.P(idx), len(idx), H.P(parent), H.P(extent), H.P(radius), H.P(pose), nj, H.P(base),
                                          H.P(order), H.P(bind), H.P(posed), H.P(off), H.P(jidx), len(jidx), H.P(sp), H.P(sn), H.P(fp), H.P(fn))
            assert n >= 0, name
            # for_joints order is a property of one process's pointers: everything is stored under the canonical order "caller's
            # index ascending WITHIN what the reference visited" only if it IS that order; otherwise the visit order itself is kept
            fixed = {"order": order, "bind": bind, "extent": extent[order], "radius": radius[order], "off": off, "jidx": jidx[:n]}
            for k, v in fixed.items():
                assert k not in out or np.array_equal(out[k], v), (name, k, "differs between poses")
                out[k] = v
            for k, v in (("posed", posed), ("smooth_pos", sp), ("smooth_nrm", sn), ("flat_pos", fp), ("flat_nrm", fn)):
                out[k].append(v)
        for k in ("posed", "smooth_pos", "smooth_nrm", "flat_pos", "flat_nrm"):
            out[k] = np.stack(out[k])
        path = os.path.join(HERE, f"skin_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, "verts", nv, "joints", nj, "order", out["order"], "influences", len(out["jidx"]), "per-vertex max", int(np.diff(out["off"]).max()),
              "none", int((np.diff(out["off"]) == 0).sum()), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
