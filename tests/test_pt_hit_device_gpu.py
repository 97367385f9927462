"""GPU: srt_pt_hit_device - scene.hit for rays in device memory, records / ids / flags into device memory, enqueue-only.

The yardstick is srt_pt_hit (the host form, untouched) and what the tree already pins: the reference build's records in the pt_*.npz
fixtures, the oracle, the CPU emulation of the device headers.  Every comparison is bit for bit (NaN == NaN).  The cast route - pack,
the streamed forms' persistent ray-cast kernel, resolve - is forced with kernel mode 6 and proven taken with srt_pt_hit_device_paths;
the per-lane route with modes 4 and 1.  Device arrays are torch tensors.

(The fixture of the 131 072-triangle scene is left out of test 1: that scene is not committed in a test here.)"""
import functools
import glob
import os

import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
from _cases import chain_rays, pt_scene, random_rays, unnormalised_rays

pytestmark = pytest.mark.gpu

GOLDENS = [g for g in sorted(glob.glob(os.path.join(H.GOLDEN, "pt_*.npz"))) if "blob131072" not in g]
DEV = "cuda:0"
NONE = 0xFFFFFFFF


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return IC.sweeps_scene() if name == "sweeps" else pt_scene(name)


def make_pt(srt, scene, use_bvh=True):
    pt = srt.Pathtracer(0)
    pt.set_params(8, 8, 1, 8, use_bvh)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


def to_dev(torch, *arrays):
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    torch.cuda.synchronize()
    return out


def query(pt, torch, rays, bounds=True, stream=0):
    """hit_device with all three outputs on `stream` (0: the default stream), then a synchronise: (out9, ids, flags) as numpy."""
    org, d, b = rays
    n = len(org)
    out9 = torch.full((n, 9), 7.0, device=DEV)
    ids = torch.full((n, 2), 7, dtype=torch.int32, device=DEV)
    flags = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    pt.hit_device(org.data_ptr(), d.data_ptr(), b.data_ptr() if bounds else 0, n, out9.data_ptr(), ids.data_ptr(), flags.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return out9.cpu().numpy(), ids.cpu().numpy().view(np.uint32), flags.cpu().numpy()


def consistent(out9, ids, flags):
    """The three outputs tell one story: flag == record's hit, ids are NONE exactly on a miss."""
    hit = out9[:, 0] != 0
    return np.array_equal(flags, hit.astype(np.uint8)) and np.array_equal(ids[:, 0] != NONE, hit) and bool((ids[~hit] == NONE).all())


# ---- 1. the pinned answers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(g)[3:-4] for g in GOLDENS])
def test_reference_golden(srt, torch, path):
    g = np.load(path)
    use_bvh, seed = bool(int(g["meta"][3])), int(g["seed"])
    scene = pt_scene(str(g["scene"]))
    pt = make_pt(srt, scene, use_bvh)
    rays = to_dev(torch, *H.golden_rays(g, scene, seed + 1))
    for mode in (6, 0):                  # (6: the cast kernel wherever it applies; 0: 2048 rays are below the automatic mode's threshold)
        pt.set_kernel(mode)
        out9, ids, flags = query(pt, torch, rays)
        assert bits_equal(out9, g["hits"]), f"hit_device (kernel mode {mode}) differs from the reference"
        assert np.array_equal(flags, (g["hits"][:, 0] != 0).astype(np.uint8)) and consistent(out9, ids, flags)
    paths = pt.hit_device_paths()
    pt.close()
    assert paths == ((1, 1, 0) if use_bvh else (0, 2, 0)), "mode 6: a BVH scene goes through the cast kernel, a list scene per lane"


def test_reference_golden_unnormalised(srt, torch):
    """The particle step's rays: un-normalised directions, bounds {0, inf} - given, and as the NULL default."""
    g = np.load(os.path.join(H.GOLDEN, "particles_cbox_blob512.npz"))
    scene = pt_scene(str(g["scene"]))
    pt = make_pt(srt, scene)
    org, d, b = unnormalised_rays(int(g["meta"][0]) + 7, 1024)
    assert (b[:, 0] == 0).all() and np.isinf(b[:, 1]).all()
    rays = to_dev(torch, org, d, b)
    for mode in (6, 4, 5):
        pt.set_kernel(mode)
        for bounds in (True, False):
            out9, ids, flags = query(pt, torch, rays, bounds=bounds)
            assert bits_equal(out9, g["hits_unnormalised"]), f"kernel mode {mode}, bounds {bounds}"
            assert np.array_equal(flags, (g["hits_unnormalised"][:, 0] != 0).astype(np.uint8)) and consistent(out9, ids, flags)
    assert pt.hit_device_paths() == (2, 2, 2)
    pt.close()


# ---- 2. both routes, the same bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cbox_particles", "sweeps"])
def test_both_routes_same_bits(srt, torch, name):
    scene = scene_of(name)
    pt = make_pt(srt, scene)
    org, d, b = random_rays(11, 4096)
    d[::2] *= np.linspace(0.25, 4.0, len(d[::2]), dtype=np.float32)[:, None]      # half of them un-normalised
    want = pt.hit(org, d, b)
    assert 1000 < int(want[:, 0].sum()) < 4096
    rays = to_dev(torch, org, d, b)
    results = {}
    for mode, route in ((6, 0), (7 if name == "sweeps" else 2, 0), (0, 1), (4, 1), (1, 1)):   # (0: below the automatic mode's threshold)
        pt.set_kernel(mode)
        before = pt.hit_device_paths()
        results[mode] = query(pt, torch, rays)
        after = pt.hit_device_paths()
        assert after[route] == before[route] + 1 and sum(after) == sum(before) + 1, f"kernel mode {mode} took another route: {before} -> {after}"
    pt.set_kernel(6)
    assert pt.kernel_form() == 3
    pt.close()
    for mode, (out9, ids, flags) in results.items():
        assert bits_equal(out9, want), f"kernel mode {mode} differs from srt_pt_hit"
        assert consistent(out9, ids, flags)
        assert np.array_equal(ids, results[4][1]) and np.array_equal(flags, results[4][2]), f"kernel mode {mode}: ids or flags differ from the per-lane route's"


def test_automatic_mode_routes_by_size_and_scene(srt, torch):
    """The automatic mode: the cast kernel from 2^19 rays on (the measured crossover), on the scenes whose render it streams as
    well; the per-lane walk below that size and on a Cornell box of single-leaf meshes.  Either way srt_pt_hit's bits."""
    n = 1 << 19
    org, d, b = random_rays(12, n)
    rays = to_dev(torch, org, d, b)
    for name, routes in (("cbox_particles", ((n, 0), (n - 1, 1))), ("cbox", ((n, 1),))):
        pt = make_pt(srt, scene_of(name))
        want = pt.hit(org, d, b)
        for m, route in routes:
            before = pt.hit_device_paths()
            out9, ids, flags = query(pt, torch, [a[:m] for a in rays])
            after = pt.hit_device_paths()
            assert after[route] == before[route] + 1 and sum(after) == sum(before) + 1, f"{name}, {m} rays: {before} -> {after}"
            assert bits_equal(out9, want[:m]) and consistent(out9, ids, flags)
        pt.close()


# ---- 3. sizes ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 31, 63, 64, 65, 255, 257, 2049)


@pytest.fixture(scope="module")
def particles_pt(srt):
    pt = make_pt(srt, scene_of("cbox_particles"))
    yield pt
    pt.close()


@pytest.fixture(scope="module")
def particles_rays(particles_pt):
    org, d, b = random_rays(21, max(SIZES))
    want = particles_pt.hit(org, d, b)
    want.setflags(write=False)
    return (org, d, b), want


@pytest.mark.parametrize("n", SIZES)
def test_sizes(particles_pt, torch, particles_rays, n):
    """Wave, block and pool (grab = 32) boundaries of the cast kernel, and lists so short that the share dealt out in advance
    rounds to no entry per wave.  The output tensors are over-allocated: nothing beyond row n is written."""
    pt = particles_pt
    (org, d, b), want = particles_rays
    cap = n + 70
    rays = to_dev(torch, org[:cap], d[:cap], b[:cap])
    out9 = torch.full((cap, 9), 7.0, device=DEV)
    ids = torch.full((cap, 2), 7, dtype=torch.int32, device=DEV)
    flags = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    only = torch.full((cap,), 7, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    pt.set_kernel(6)
    before = pt.hit_device_paths()
    pt.hit_device(rays[0].data_ptr(), rays[1].data_ptr(), rays[2].data_ptr(), n, out9.data_ptr(), ids.data_ptr(), flags.data_ptr())
    pt.hit_device(rays[0].data_ptr(), rays[1].data_ptr(), rays[2].data_ptr(), n, 0, 0, only.data_ptr())      # the shadow-ray question alone
    torch.cuda.synchronize()
    assert pt.hit_device_paths()[0] == before[0] + 2
    out9, ids, flags, only = out9.cpu().numpy(), ids.cpu().numpy(), flags.cpu().numpy(), only.cpu().numpy()
    assert bits_equal(out9[:n], want[:n])
    assert consistent(out9[:n], ids[:n].view(np.uint32), flags[:n]) and np.array_equal(only[:n], flags[:n])
    assert (out9[n:] == 7.0).all() and (ids[n:] == 7).all() and (flags[n:] == 7).all() and (only[n:] == 7).all(), "written beyond n"


# ---- 4. stacks ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(name):
    scene = scene_of(name)
    org, d, b = chain_rays(7, 3000, scene)
    want = H.OraclePT(scene, 8, 8, 8, True).hit(org, d, b)
    want.setflags(write=False)
    assert int(want[:, 0].sum()) > 2000
    return (org, d, b), want


@pytest.mark.parametrize("name", ["deep_both", "deep_max"])
@pytest.mark.parametrize("lds_frames", [None, 1])
def test_stacks(srt, torch, monkeypatch, name, lds_frames):
    """Trees at the limits of the traversal stacks (24 + 48 frames), rays aimed down the chain (axial ones, cut-short bounds): with
    the default frames in LDS and with one, where everything else goes through the spill columns.  The launch shape is derived once
    per committed scene: a fresh context per setting."""
    if lds_frames is None:
        monkeypatch.delenv("SRT_CAST_LDS_FRAMES", raising=False)
    else:
        monkeypatch.setenv("SRT_CAST_LDS_FRAMES", str(lds_frames))
    rays_np, want = chain_case(name)
    pt = make_pt(srt, scene_of(name))
    pt.set_kernel(6)
    out9, ids, flags = query(pt, torch, to_dev(torch, *rays_np))
    paths = pt.hit_device_paths()
    pt.close()
    assert paths == (1, 0, 0)
    assert bits_equal(out9, want), f"{name}, SRT_CAST_LDS_FRAMES={lds_frames}: differs from the oracle"
    assert consistent(out9, ids, flags)


# ---- 5. chunks ---------------------------------------------------------------------------------------------------------------------
def test_chunks(srt, torch, monkeypatch):
    pt = make_pt(srt, scene_of("cbox_blob512_glass"))
    pt.set_kernel(6)
    rays = to_dev(torch, *random_rays(31, 3000))
    monkeypatch.delenv("SRT_HIT_CHUNK", raising=False)
    whole = query(pt, torch, rays)
    monkeypatch.setenv("SRT_HIT_CHUNK", "1000")
    cut = query(pt, torch, rays)
    monkeypatch.setenv("SRT_HIT_CHUNK", "999")             # (a last chunk of three rays)
    odd = query(pt, torch, rays)
    assert pt.hit_device_paths() == (3, 0, 0)
    pt.close()
    assert 500 < int(whole[2].sum()) < 2500                # (hits and misses on both sides of every chunk boundary)
    for got in (cut, odd):
        assert bits_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1]) and np.array_equal(got[2], whole[2])


# ---- 6. ids ------------------------------------------------------------------------------------------------------------------------
def test_ids(srt, torch):
    """(object slot, global triangle) of the CPU emulation's nested walk, carried to (insertion index, place in the mesh's primitive
    order) through the top-level tree's order and the objects' triangle counts.  The emulation knows no instances: it is given the
    expansion, whose instance has triangles of its own - the query must name the instance and the SHARED mesh's place."""
    S = scene_of("sweeps")
    E = IC.expand(S)
    pt = make_pt(srt, S)
    org, d, b = random_rays(41, 4096)
    emu = H.EmuPT(E, True)
    nested, _ = emu.hit(org, d, b)
    emu.close()
    order = pt.dump_bvh(-1)[2][: len(S["objects"])].astype(np.int64) - 1      # object slot -> insertion index
    ntri = np.array([len(o["idx"]) // 3 if o["kind"] == "mesh" else 0 for o in E["objects"]], np.int64)
    base = np.concatenate([[0], np.cumsum(ntri[order])[:-1]])                 # the triangles are stored mesh by mesh in slot order
    is_sphere = np.array([o["kind"] == "sphere" for o in E["objects"]])
    hit = nested[:, 0] != 0
    slot = nested[:, 2].astype(np.int64)
    obj = order[slot]
    want = np.full((len(org), 2), NONE, np.uint32)
    want[hit, 0] = obj[hit]
    mesh_hit = hit & ~is_sphere[obj]
    want[mesh_hit, 1] = (nested[mesh_hit, 3].astype(np.int64) - base[slot[mesh_hit]]).astype(np.uint32)
    instance = len(S["objects"]) - 1
    assert S["objects"][instance]["kind"] == "instance"
    assert int((want[:, 0] == instance).sum()) > 20 and int((want[:, 0] == int(S["objects"][instance]["of"])).sum()) > 20
    assert (want[mesh_hit, 1] < ntri[obj[mesh_hit]]).all()
    rays = to_dev(torch, org, d, b)
    for mode in (6, 0, 4, 5):
        pt.set_kernel(mode)
        out9, ids, flags = query(pt, torch, rays)
        assert np.array_equal(ids, want), f"kernel mode {mode}"
        assert np.array_equal(out9[:, 1].view(np.uint32)[hit], nested[hit, 1]) and consistent(out9, ids, flags)
    pt.close()
    # a sphere: the second word is NONE
    S2 = scene_of("cbox")
    spheres = [k for k, o in enumerate(S2["objects"]) if o["kind"] == "sphere"]
    assert spheres
    pt = make_pt(srt, S2)
    pt.set_kernel(6)
    out9, ids, flags = query(pt, torch, to_dev(torch, *random_rays(42, 2048)))
    pt.close()
    on_sphere = np.isin(ids[:, 0], spheres)
    assert int(on_sphere.sum()) > 20 and (ids[on_sphere, 1] == NONE).all() and (ids[(ids[:, 0] != NONE) & ~on_sphere, 1] != NONE).all()


# ---- 7. the frame loop ---------------------------------------------------------------------------------------------------------------
def test_frame_loop_on_one_stream(srt, torch):
    """set_active_device -> repose_refit_device -> hit_device -> a torch copy of the outputs, on ONE stream with no synchronise in
    between: the query sees both updates (srt_pt_hit settles the host's record first, so it answers for the scene after both)."""
    S = scene_of("cbox_particles")
    pt = make_pt(srt, S)
    pt.set_kernel(6)
    idx, Ts = IC.repose_case(S)
    off = np.array([k for k in range(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + IC.PARTICLE_COUNT, 2) if k not in set(idx.tolist())], np.uint32)
    org, d, b = random_rays(51, 4096)
    rays = to_dev(torch, org, d, b)
    d_flags, d_T = to_dev(torch, np.zeros(len(off), np.uint8), Ts)
    before = pt.hit(org, d, b)
    n = len(org)
    out9, ids, flags = torch.zeros((n, 9), device=DEV), torch.zeros((n, 2), dtype=torch.int32, device=DEV), torch.zeros((n,), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        pt.set_active_device(off, d_flags.data_ptr(), stream=st.cuda_stream)
        pt.repose_refit_device(idx, d_T.data_ptr(), stream=st.cuda_stream)
        pt.hit_device(rays[0].data_ptr(), rays[1].data_ptr(), rays[2].data_ptr(), n, out9.data_ptr(), ids.data_ptr(), flags.data_ptr(), stream=st.cuda_stream)
        c9, cids, cflags = out9.clone(), ids.clone(), flags.clone()
    st.synchronize()
    assert pt.hit_device_paths() == (1, 0, 0)
    want = pt.hit(org, d, b)
    pt.close()
    assert not bits_equal(before, want), "the updates changed nothing these rays can see"
    c9, cids, cflags = c9.cpu().numpy(), cids.cpu().numpy().view(np.uint32), cflags.cpu().numpy()
    assert bits_equal(c9, want) and consistent(c9, cids, cflags)
    assert not np.isin(cids[:, 0], off).any(), "a ray reports an inactive object"
    assert np.isin(cids[:, 0], idx).any(), "no ray reaches a moved object"


# ---- 8. two streams ------------------------------------------------------------------------------------------------------------------
def test_two_streams(particles_pt, torch):
    pt = particles_pt
    pt.set_kernel(6)
    sets = [random_rays(61, 3000), random_rays(62, 2500)]
    wants = [pt.hit(*r) for r in sets]
    dev = [to_dev(torch, *r) for r in sets]
    outs = [(torch.zeros((len(r[0]), 9), device=DEV), torch.zeros((len(r[0]), 2), dtype=torch.int32, device=DEV),
             torch.zeros((len(r[0]),), dtype=torch.uint8, device=DEV)) for r in sets]
    streams = [torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)]
    torch.cuda.synchronize()
    before = pt.hit_device_paths()
    for r, o, s in zip(dev, outs, streams):
        pt.hit_device(r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), len(r[0]), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    assert pt.hit_device_paths()[0] == before[0] + 2
    for o, want in zip(outs, wants):
        out9, ids, flags = o[0].cpu().numpy(), o[1].cpu().numpy().view(np.uint32), o[2].cpu().numpy()
        assert bits_equal(out9, want) and consistent(out9, ids, flags)


# ---- 9. visibility -------------------------------------------------------------------------------------------------------------------
def test_torch_kernel_behind_the_query(particles_pt, torch, particles_rays):
    """hit_tensors enqueues on torch's current stream and returns without synchronising; torch kernels enqueued behind it on that
    stream - a reduction, a gather - read the outputs with no event and no synchronise in between."""
    pt = particles_pt
    (org, d, b), want = particles_rays
    pt.set_kernel(6)
    t_org, t_d, t_b = to_dev(torch, org, d, b)
    st = torch.cuda.Stream(device=DEV)
    before = pt.hit_device_paths()
    with torch.cuda.stream(st):
        out9, ids, flags = pt.hit_tensors(t_org, t_d, t_b, ids=True, flags=True)
        count = flags.sum(dtype=torch.int64)
        nearest = torch.where(flags.bool(), out9[:, 1], torch.full_like(out9[:, 1], float("inf"))).min()
        only9 = pt.hit_tensors(t_org, t_d)                    # bounds = None: {0, inf}
        total = only9[:, 0].sum()
    st.synchronize()
    assert pt.hit_device_paths()[0] == before[0] + 2
    hit = want[:, 0] != 0
    assert int(count.item()) == int(hit.sum()) and float(nearest.item()) == float(want[hit, 1].min())
    assert bits_equal(out9.cpu().numpy(), want) and consistent(out9.cpu().numpy(), ids.cpu().numpy().view(np.uint32), flags.cpu().numpy())
    open_b = np.zeros_like(b)
    open_b[:, 1] = np.inf
    want_open = pt.hit(org, d, open_b)
    assert bits_equal(only9.cpu().numpy(), want_open) and float(total.item()) == float(want_open[:, 0].sum())
    with pytest.raises(ValueError):
        pt.hit_tensors(t_org, t_d[:5])
