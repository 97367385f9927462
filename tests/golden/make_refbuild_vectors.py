#!/usr/bin/env python3
"""Generate the fixtures that pin the oracles against the REFERENCE build without it: the inputs of the reference-build
tests in tests/test_raster_oracle.py and tests/test_pt_oracle.py and what oracle/_ref/libref_*.so returned for them.

Run where the reference checkout is present and `make -C oracle ref` has built oracle/_ref:

    python tests/golden/make_refbuild_vectors.py            (every fixture)
    python tests/golden/make_refbuild_vectors.py sphere     (refbuild_sphere_edges.npz alone)
    python tests/golden/make_refbuild_vectors.py shade      (refbuild_shade_edges.npz alone)

refbuild_raster_random.npz  per supersample rate and seed: the primitive stream, the reference's RGBA8 and the SHA-256 of
                            its float supersample buffer
refbuild_pt_samples.npz     per scene: its digest, the sample list, the reference's per-sample radiance and RNG draw counts
refbuild_tonemap.npz        per seed: the radiance image (NaN and negative values included), the exposure, the reference's bytes
refbuild_sphere_edges.npz   the Sphere::hit edge sets of tests/_sphere_cases.py (fixture_sets: tangents, the validity chain, special
                            operands), the reference's scene.hit records {hit, distance, position, normal} of their rays on one-sphere
                            scenes - the sphere at the origin, and at (0.3, -0.2, 0.1) scaled (1.5, 0.5, 2) - and the scenes' digests
refbuild_shade_edges.npz    per case of tests/_shade_edge_cases.py the reference runs to the end (REFERENCE_SET): the scene's digest and the
                            reference's per-sample radiance and RNG draw counts on the first samples of the cases' sample list (regenerated,
                            not stored), seed 5, depth 8, with BVHs
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _harness as H  # noqa: E402
import _sphere_cases as SPH  # noqa: E402
from _cases import adversarial_stream, pt_sample_list, pt_scene, random_triangles, scene_digest, tonemap_image  # noqa: E402

RASTER_W, RASTER_H = 83, 59
RASTER_RATES = (1, 2, 3, 4, 7)
RASTER_SEEDS = (0, 1, 2)
PT_W, PT_H, PT_DEPTH, PT_SEED = 40, 30, 8, 123456789
PT_CASES = (("cbox", True), ("cbox_lambertian", False), ("cbox_blob512_glass", True))
TONEMAP_CASES = ((101, 1.0), (102, 0.8), (103, 3.0))
SHADE_STORED = 600      # samples of the list kept per case of refbuild_shade_edges.npz (the first ones): what keeps the file under 300 KB


def raster_stream(sr, seed):
    return np.concatenate([random_triangles(100 * sr + seed, 120, RASTER_W, RASTER_H, 50), adversarial_stream(seed, RASTER_W, RASTER_H)])


def tonemap_input(seed):
    rgb = tonemap_image("mixed", 96, 64, seed)
    rng = np.random.default_rng(seed)
    flat = rgb.reshape(-1)
    flat[rng.integers(0, flat.size, 200)] = np.float32(np.nan)
    flat[rng.integers(0, flat.size, 200)] = -np.abs(rng.normal(size=200)).astype(np.float32)
    return rgb


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def sphere_edges():
    index, radius, org, dirs, bounds, family, step = SPH.fixture_sets()
    rr, oo, dd, bb = SPH.rays_of(radius, org, dirs, bounds)
    assert len(rr) <= 20000 and set(family.tolist()) == set(range(len(SPH.FAMILIES)))
    out = {"seed": np.int64(SPH.FIXTURE_SEED), "index": index, "radius": radius, "org": org, "dirs": dirs, "bounds": bounds,
           "family": family, "step": step, "families": np.array(SPH.FAMILIES)}
    for kind in SPH.SCENE_KINDS:
        rec = SPH.scene_hits(lambda scene: H.RefPT(scene, 8, 8, 4, True), rr, oo, dd, bb, kind)
        assert (rec[:, 8] == np.where(rec[:, 0] != 0, 0.0, rec[:, 8])).all()      # (the material of a hit is the scene's one)
        out[f"ref_{kind}"] = rec[:, :8].copy()
        out[f"scene_sha256_{kind}"] = np.array(SPH.scenes_digest(rr, kind, scene_digest))
    path = os.path.join(HERE, "refbuild_sphere_edges.npz")
    np.savez_compressed(path, **out)
    # the stored inputs are what the generator of the cases makes today
    g = np.load(path)
    again = SPH.fixture_sets()
    for key, a in zip(("index", "radius", "org", "dirs", "bounds", "family", "step"), again):
        assert same_bits(g[key], a), key
    print("wrote refbuild_sphere_edges.npz", os.path.getsize(path), "bytes,", len(rr), "rays, hits",
          {kind: int((out[f"ref_{kind}"][:, 0] != 0).sum()) for kind in SPH.SCENE_KINDS})


def save_npz_reproducibly(path, arrays):
    """np.savez_compressed with the members' time stamps fixed (it writes the time of the run): the same arrays give the same bytes."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, value in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def shade_edges():
    import _shade_edge_cases as E

    # Left out, and why (nothing else is):
    #   emission_0, emission_negative   a light material whose emission has no positive luma is scattered like a BSDF, and the reference
    #                                   aborts there (rays/bsdf.h:102, "You scattered an emissive BSDF!"); E.ORACLE_ONLY
    #   an Env_Map lookup with a NaN direction would read outside HDR_Image: no case of E.CASES does (every case below ran to the end
    #   in the reference build, whose HDR_Image::at asserts its bounds)
    assert sorted(set(E.CASES) - set(E.REFERENCE_SET)) == ["emission_0", "emission_negative"]
    xs, ys, ss = E.sample_list()
    out = {"meta": np.array([E.W, E.H, E.DEPTH, E.SEED, E.NSAMPLES, SHADE_STORED], np.int64), "cases": np.array(E.REFERENCE_SET)}
    for name in E.REFERENCE_SET:
        scene = E.shade_edge_scene(name)
        rgb, draws = H.RefPT(scene, E.W, E.H, E.DEPTH, True).trace_samples(E.SEED, xs, ys, ss)
        assert draws.max() < 1 << 16
        out[f"rgb_{name}"], out[f"draws_{name}"] = rgb[:SHADE_STORED], draws[:SHADE_STORED].astype(np.uint16)
        out[f"scene_sha256_{name}"] = np.array(scene_digest(scene))
    path = os.path.join(HERE, "refbuild_shade_edges.npz")
    save_npz_reproducibly(path, out)
    print("wrote refbuild_shade_edges.npz", os.path.getsize(path), "bytes,", len(E.REFERENCE_SET), "cases,", SHADE_STORED, "of", E.NSAMPLES, "samples each")
    assert os.path.getsize(path) < 300 * 1000


def main():
    assert H.ref_raster() is not None and H.ref_pt_lib() is not None, "build oracle/_ref first: make -C oracle ref"
    if sys.argv[1:] == ["sphere"]:
        return sphere_edges()
    if sys.argv[1:] == ["shade"]:
        return shade_edges()
    sphere_edges()
    shade_edges()
    out = {}
    for sr in RASTER_RATES:
        for seed in RASTER_SEEDS:
            prims = raster_stream(sr, seed)
            rgba, ss = H.ref_raster_prims(prims, RASTER_W, RASTER_H, sr, want_samples=True)
            out[f"prims_sr{sr}_s{seed}"], out[f"rgba_sr{sr}_s{seed}"] = prims, rgba
            out[f"ss_sha256_sr{sr}_s{seed}"] = np.array(H.sha(ss))
    np.savez_compressed(os.path.join(HERE, "refbuild_raster_random.npz"), meta=np.array([RASTER_W, RASTER_H], np.int64), **out)

    out = {}
    for name, use_bvh in PT_CASES:
        xs, ys, ss = pt_sample_list(77, PT_W, PT_H, 6000, max_sample=1 << 20)
        rgb, draws = H.RefPT(pt_scene(name), PT_W, PT_H, PT_DEPTH, use_bvh).trace_samples(PT_SEED, xs, ys, ss)
        for k, v in (("xs", xs), ("ys", ys), ("ss", ss), ("rgb", rgb), ("draws", draws)):
            out[f"{k}_{name}"] = np.asarray(v)
        out[f"scene_sha256_{name}"] = np.array(scene_digest(pt_scene(name)))
    np.savez_compressed(os.path.join(HERE, "refbuild_pt_samples.npz"), meta=np.array([PT_W, PT_H, PT_DEPTH, PT_SEED], np.int64),
                        unqualified_sqrt_is_double=np.int64(H.ref_pt_lib().ref_pt_unqualified_sqrt_is_double()), **out)

    out = {}
    for seed, exposure in TONEMAP_CASES:
        rgb = tonemap_input(seed)
        out[f"rgb_{seed}"], out[f"exposure_{seed}"], out[f"rgba_{seed}"] = rgb, np.float32(exposure), H.ref_tonemap(rgb, exposure)
    np.savez_compressed(os.path.join(HERE, "refbuild_tonemap.npz"), **out)
    for f in ("refbuild_raster_random.npz", "refbuild_pt_samples.npz", "refbuild_tonemap.npz"):
        print("wrote", f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
