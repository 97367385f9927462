"""CPU: the skewed-tree scenes of tests/_cases.py (deep_*) are as deep as their names say, the product's host build of them equals
the oracle's, scenes beyond the traversal stacks are refused cleanly, and - from the host emulation of csrc/pt_flat.h over a stack
that counts - the rays the GPU tests of tests/test_pt_stack_depth_gpu.py trace really do fill the stacks: the per-lane frames of
the streamed ray-cast kernel beyond every LDS frame count those tests set, the 48 frames of a mesh's tree, and all
kFlatStack = 24 + 48 frames of the flattened walk."""
import numpy as np
import pytest

import _harness as H
from _cases import DEEP_CHAIN_TRIANGLES, DEEP_TLAS_SPHERES, camera_rays, chain_rays, pt_scene

K_MAX_TLAS, K_MAX_BLAS = 24, 48            # kMaxTlasDepth, kMaxBlasDepth (csrc/pt_trace.h)
IMAGE = (32, 24)                           # what the GPU tests render
BANDS = {                                  # name: ((lowest, highest max_tlas_depth), (lowest, highest max_blas_depth)); None: any
    "deep_mid": ((0, K_MAX_TLAS), (14, 20)),
    "deep_max": ((0, K_MAX_TLAS), (K_MAX_BLAS, K_MAX_BLAS)),
    "deep_over": ((0, K_MAX_TLAS), (K_MAX_BLAS + 1, 10 ** 6)),
    "deep_tlas": ((20, K_MAX_TLAS), (14, 20)),
    "deep_tlas_over": ((K_MAX_TLAS + 1, 10 ** 6), (14, 20)),
    "deep_both": ((K_MAX_TLAS, K_MAX_TLAS), (K_MAX_BLAS, K_MAX_BLAS)),
}
ACCEPTED = ("deep_mid", "deep_max", "deep_tlas", "deep_both")
REFUSED = ("deep_over", "deep_tlas_over")


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def interior_depth(links):
    """Interior-node nesting of a dumped tree (links = {start, size, l, r} per node, children after their parent)."""
    d = np.zeros(len(links), np.int64)
    for n in range(len(links) - 1, -1, -1):
        l, r = int(links[n, 2]), int(links[n, 3])
        if l != r:
            d[n] = 1 + max(d[l], d[r])
    return int(d[0]) if len(links) else 0


def leaf_level(links, prim_slot):
    """Interior nodes above the leaf that holds primitive slot `prim_slot`."""
    n, level = 0, 0
    while int(links[n, 2]) != int(links[n, 3]):
        l = int(links[n, 2])
        n = l if prim_slot < int(links[l, 0]) + int(links[l, 1]) else int(links[n, 3])
        level += 1
    return level


def tree_depths(dump, nobjects):
    """(max_tlas_depth, max_blas_depth, BVH<Object> level of the deepest mesh's leaf, its slot) from a dump_bvh callable."""
    tlas = dump(-1)
    t, b, slot = interior_depth(tlas[1]), 0, -1
    for k in range(nobjects):
        try:
            tree = dump(k)
        except Exception:                      # a sphere's slot
            tree = None
        if tree is not None and interior_depth(tree[1]) > b:
            b, slot = interior_depth(tree[1]), k
    return t, b, leaf_level(tlas[1], slot), slot


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def test_chain_family_sizes():
    assert set(BANDS) == set(DEEP_CHAIN_TRIANGLES) | set(DEEP_TLAS_SPHERES)
    assert len(pt_scene("deep_mid")["objects"]) <= 16 and len(pt_scene("deep_max")["objects"]) <= 16          # the streamed sweeps take them
    assert len(pt_scene("deep_tlas")["objects"]) > 31                    # more than the flattened walk and the sweeps take
    assert len(pt_scene("deep_both")["objects"]) <= 31                   # the flattened walk's scene.hit still takes it


@pytest.mark.parametrize("name", sorted(BANDS))
def test_depth_bands_from_the_oracle_build(name):
    """Every fixture, the refused ones included (the oracle has no stacks to outgrow): depths in their bands, every box finite."""
    scene = pt_scene(name)
    o = H.OraclePT(scene, 8, 8, 4, True)
    t, b, _, _ = tree_depths(o.dump_bvh, len(scene["objects"]))
    print(f"{name}: max_tlas_depth {t}, max_blas_depth {b}")
    (t0, t1), (b0, b1) = BANDS[name]
    assert t0 <= t <= t1 and b0 <= b <= b1
    for k in range(-1, len(scene["objects"])):
        tree = o.dump_bvh(k)
        if tree is not None:
            assert np.isfinite(tree[0]).all()


@pytest.mark.parametrize("name", ACCEPTED)
def test_host_build_of_skewed_trees_equals_the_oracle(srt, name):
    scene = pt_scene(name)
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 4, True)
    pt.build_scene(scene)
    t, b, _, slot = tree_depths(pt.dump_bvh, len(scene["objects"]))
    (t0, t1), (b0, b1) = BANDS[name]
    assert t0 <= t <= t1 and b0 <= b <= b1
    o = H.OraclePT(scene, 8, 8, 4, True)
    nobj = len(scene["objects"])
    pb, pl, po = pt.dump_bvh(-1)
    ob, ol, oo = o.dump_bvh(-1)
    assert bits_equal(pb, ob) and np.array_equal(pl, ol) and np.array_equal(po[:nobj], oo[:nobj])
    pb, pl, po = pt.dump_bvh(slot)
    ob, ol, oo = o.dump_bvh(slot)
    ntri = len(scene["objects"][int(oo_slot(pt, slot))]["idx"]) // 3
    assert len(pb) == len(ob) == 2 * (ntri - 4) + 1            # one triangle split off per level down to a leaf of four
    assert bits_equal(pb, ob) and np.array_equal(pl, ol) and np.array_equal(po[:ntri], oo[:ntri])
    pt.close()


def oo_slot(pt, slot):
    """Index into scene["objects"] of BVH<Object> slot `slot` (dump_bvh(-1)'s order holds object ids, 1-based)."""
    return pt.dump_bvh(-1)[2][slot] - 1


@pytest.mark.parametrize("name", REFUSED)
def test_too_deep_scenes_are_refused_and_the_context_lives_on(srt, name):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 4, True)
    with pytest.raises(srt.SrtError) as e:
        pt.build_scene(pt_scene(name))
    assert e.value.status == -4 and "too deep" in str(e.value)          # SRT_ERR_UNSUPPORTED
    with pytest.raises(srt.SrtError):
        pt.dump_bvh(-1)                                                  # nothing is committed
    cbox = pt_scene("cbox")
    pt.build_scene(cbox)
    o = H.OraclePT(cbox, 8, 8, 4, True)
    pb, pl, po = pt.dump_bvh(-1)
    ob, ol, oo = o.dump_bvh(-1)
    assert bits_equal(pb, ob) and np.array_equal(pl, ol) and np.array_equal(po[:8], oo[:8])
    pt.close()


def lds_frame_counts(t, b, mode):
    """The SRT_CAST_LDS_FRAMES values tests/test_pt_stack_depth_gpu.py sets and the kernels' defaults (13; 10 for the walk-only build
    of mode 7), as far as a frame index can reach them at all: render_epoch_stream reserves depth = t + b + 1 frames per lane
    (b + 1 in mode 7, whose walks start inside the mesh), the walk uses at most depth - 1 of them (checked below), so with
    depth - 1 or depth frames in LDS nothing spills - those two settings pin the no-spill shape against the others."""
    depth = (t if mode == 6 else 0) + b + 1
    return [k for k in (1, 2, 10, 13, b) if k <= depth - 2], depth


@pytest.mark.parametrize("name", ACCEPTED)
def test_gpu_test_rays_fill_the_stacks(name):
    """The non-vacuity conditions of the GPU tests, from the counting stack (tests/host_emu/flat_host.cpp)."""
    scene = pt_scene(name)
    emu = H.EmuPT(scene, True)
    org, dirs, bounds = camera_rays(scene["camera"], *IMAGE)
    deepest, flat, (t, b) = emu.hit_depth(org, dirs, bounds)
    assert np.array_equal(flat, emu.hit(org, dirs, bounds, 0)[1])        # the counting walk IS the flattened walk
    pt_dump = H.OraclePT(scene, 8, 8, 4, True).dump_bvh
    t_o, b_o, level, _ = tree_depths(pt_dump, len(scene["objects"]))
    assert (t, b) == (t_o, b_o)
    c_org, c_dirs, c_bounds = chain_rays(7, 3000, scene)
    c_deepest, c_flat, _ = emu.hit_depth(c_org, c_dirs, c_bounds)
    # the host's formula: no walk may touch frame max_tlas_depth + max_blas_depth or beyond (in fact the last one used is one below)
    assert max(deepest.max(), c_deepest.max()) < t + b + 1
    assert max(deepest.max(), c_deepest.max()) <= level + b - 1
    # the walk-only build (mode 7) starts inside the mesh: its frame index is the flattened walk's minus the BVH<Object> frames
    # below the mesh, at most `level` of them
    for mode, idx in ((6, deepest), (7, deepest - level)):
        if mode == 7 and len(scene["objects"]) > 16:
            continue
        ks, depth = lds_frame_counts(t, b, mode)
        for k in ks:
            n = int((idx >= k).sum())
            print(f"{name} mode {mode}: depth {depth}, {n} of {len(idx)} camera rays touch a frame index >= {k}")
            assert n >= 256
    top = int((deepest >= level + b - 3).sum())
    print(f"{name}: max_tlas_depth {t}, max_blas_depth {b}, mesh at BVH<Object> level {level}; deepest frame index {deepest.max()} (camera rays, "
          f"{top} within two of {level + b - 1}), {c_deepest.max()} (chain rays)")
    # within two of the deepest frame a walk of this scene can use, level + b - 1; for deep_both that is kFlatStack - 1 = 71
    assert top >= 1 and c_deepest.max() >= level + b - 3
    if name == "deep_both":
        assert level + b == K_MAX_TLAS + K_MAX_BLAS and c_deepest.max() == K_MAX_TLAS + K_MAX_BLAS - 1
    if name in ("deep_max", "deep_both"):
        assert (deepest - level).max() >= K_MAX_BLAS - 3                  # the nested walks' private arrays of 48 frames
    emu.close()
