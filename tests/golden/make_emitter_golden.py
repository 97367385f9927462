"""Records tests/golden/emitter_<case>.npz: what the reference's own Scene_Particles::step (scene/particles.cpp:101-162, with
Particle::update, util/rand.cpp and the PT:: scene classes) computes frame by frame for the cases of tests/_emitter_cases.py.
Runs only where the reference is (integration/_build/libdropin_pt_full.so, harness/emitter_ref.cpp):
    python tests/golden/make_emitter_golden.py
The files hold data only: the collide scene and the pool by name, the capacity, Scene_Particles::radius, per frame the options, the
pose and dt, the uniforms the run consumed (proven by the harness against one more RNG::unit()), and per frame the particle vector
(pos, velocity, age), its size, the substep and spawn counts, last_update and particle_cooldown afterwards, and the birth ordinal of
every particle of the vector.  Every property the tests rely on is asserted here, on the recorded values."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _emitter_cases as EC  # noqa: E402
import _harness as H  # noqa: E402

F = np.float32
GRAVITY_ONLY = 1e-6          # a velocity's x and z change by more than this between two frames only through a bounce


def scene_arrays(scene):
    kind, vert_off, idx_off, pos, nrm, idx, radius, T = [], [0], [0], [], [], [], [], []
    for o in scene["objects"]:
        assert o["kind"] in ("mesh", "sphere")
        kind.append(1 if o["kind"] == "sphere" else 0)
        if o["kind"] == "mesh":
            pos.append(np.asarray(o["pos"], F).reshape(-1, 3)); nrm.append(np.asarray(o["nrm"], F).reshape(-1, 3)); idx.append(np.asarray(o["idx"], np.uint32).reshape(-1))
        vert_off.append(sum(len(p) for p in pos)); idx_off.append(sum(len(i) for i in idx))
        radius.append(o.get("radius", 0.0))
        T.append(np.asarray(o["T"], F).reshape(16))
    return (np.array(kind, np.uint32), np.array(vert_off, np.uint32), np.array(idx_off, np.uint32), np.ascontiguousarray(np.concatenate(pos), F),
            np.ascontiguousarray(np.concatenate(nrm), F), np.ascontiguousarray(np.concatenate(idx), np.uint32), np.array(radius, F), np.ascontiguousarray(T, F))


def run_reference(lib, case):
    dts, options, poses = case["frames"]
    n, cap = len(dts), case["record"]
    kind, vert_off, idx_off, pos, nrm, idx, radius, T = scene_arrays(EC.collide_scene())
    count, substeps, spawns = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    particles, schedule = np.zeros((n, cap, 7), F), np.zeros((n, 2), np.float64)
    uniforms, nuniforms = np.zeros(1 << 16, F), np.zeros(1, np.uint32)
    st = lib.dropin_emitter_reference(H.P(kind), H.P(vert_off), H.P(idx_off), H.P(pos), H.P(nrm), H.P(idx), H.P(radius), H.P(T), len(kind),
                                      ctypes.c_float(float(EC.RADIUS)), H.P(options), H.P(poses), H.P(dts), n, cap, H.P(count), H.P(particles), H.P(substeps),
                                      H.P(spawns), H.P(schedule), H.P(uniforms), len(uniforms), H.P(nuniforms))
    assert st == 0, f"dropin_emitter_reference returned {st}"
    return {"count": count, "substeps": substeps, "spawns": spawns, "particles": particles, "schedule": schedule,
            "uniforms": uniforms[:int(nuniforms[0])].reshape(-1, 2).copy()}


def number_births(case, r):
    """birth[f, k]: the ordinal of entry k of frame f's vector.  The spawns of a frame are the tail of its vector, numbered on from the
    ordinals consumed so far; what is in front are survivors - the tail of the previous vector (ages never decrease along it)."""
    dts, options, _ = case["frames"]
    n, cap = r["particles"].shape[:2]
    birth = np.zeros((n, cap), np.uint32)
    born, prev = 0, np.zeros(0, np.uint32)
    for f in range(n):
        c, k = int(r["count"][f]), int(r["spawns"][f])
        assert c <= cap and k <= c or c == 0
        age = r["particles"][f, :c, 6]
        assert np.all(np.diff(age) >= 0), f"frame {f}: ages decrease along the vector"
        if r["substeps"][f]:
            assert r["substeps"][f] * options[f][5] < options[f][3], "a particle could be born and die inside one frame"
        if c == 0 and not options[f][6]:
            prev = np.zeros(0, np.uint32)                   # clear()
        else:
            survivors = c - k
            assert survivors <= len(prev)
            prev = np.concatenate([prev[len(prev) - survivors:], np.arange(born, born + k, dtype=np.uint32)])
        born += k
        birth[f, :c] = prev
    assert 2 * born == r["uniforms"].size
    return birth


def check(name, case, g):
    """What the fixture must contain (tests/test_pt_emitter_host.py asserts the same on the committed files)."""
    n = len(g["dts"])
    assert np.isfinite(g["particles"]).all() and g["count"].max() <= case["capacity"] and g["count"].max() <= case["record"]
    deaths = reuse_same = bounces = 0
    for f in range(1, n):
        a, b = g["birth"][f - 1, :g["count"][f - 1]], g["birth"][f, :g["count"][f]]
        if not g["options"][f][6]:
            continue
        gone = np.setdiff1d(a, b)
        deaths += len(gone)
        if len(gone) and g["spawns"][f]:
            reuse_same += 1                                   # deaths and spawns in one frame: with the lowest-dead-slot rule the slots are reused
        both, ia, ib = np.intersect1d(a, b, return_indices=True)
        va, vb = g["particles"][f - 1, ia, 3:6], g["particles"][f, ib, 3:6]
        bounces += int(np.sum((np.abs(va[:, 0] - vb[:, 0]) > GRAVITY_ONLY) | (np.abs(va[:, 2] - vb[:, 2]) > GRAVITY_ONLY)))
    assert deaths >= 1 and reuse_same >= 1 and bounces >= 1, (name, deaths, reuse_same, bounces)
    if name == "small":
        en, odt = g["options"][:, 6] != 0, g["options"][:, 5]
        assert np.any((g["substeps"] == 0) & en & (odt >= 1e-5)) and np.any(g["substeps"] >= 3)
        assert np.any(~en) and np.any(en[1:] & ~en[:-1])      # a disabled frame, then enabled again
        assert np.any(odt < 1e-5)
        assert np.any((g["pose"][:, 3:] != 0).all(axis=1) & (g["options"][:, 1] > 0))
        off = int(np.flatnonzero(~en)[0])
        assert g["count"][off] == 0 and g["count"][off - 1] > 0 and g["count"][off + 1] > 0
        assert case["capacity"] % 64 != 0
    if name == "wide":
        assert g["count"].max() > 256 and g["substeps"].sum() >= 40 and g["count"].max() <= 1200
    return deaths, reuse_same, bounces


def record(lib, name, case):
    r = run_reference(lib, case)
    dts, options, poses = case["frames"]
    g = {"collide": np.array("cbox_particles without its particles"), "pool": np.array(case["pool"]), "capacity": np.uint32(case["capacity"]),
         "radius": EC.RADIUS, "dts": dts, "options": options, "pose": poses, "uniforms": r["uniforms"], "count": r["count"], "particles": r["particles"],
         "substeps": r["substeps"], "spawns": r["spawns"], "schedule": r["schedule"], "birth": number_births(case, r)}
    figures = check(name, case, g)
    path = os.path.join(HERE, f"emitter_{name}.npz")
    np.savez_compressed(path, **g)
    print(name, "frames", len(dts), "substeps", list(g["substeps"]), "spawns", list(g["spawns"]), "population", list(g["count"]),
          "deaths / frames with reuse / bounces", figures, os.path.getsize(path), "bytes")


def main():
    lib = ctypes.CDLL(os.path.join(ROOT, "integration", "_build", "libdropin_pt_full.so"))
    for name, case in EC.cases().items():
        record(lib, name, case)


if __name__ == "__main__":
    main()
