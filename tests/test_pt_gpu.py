"""GPU: parity of the HIP path tracer (through the C ABI) with the oracle and the reference goldens.
north_star asks for <= 1e-4 per-channel L-inf on radiance at a fixed RNG seed; the kernel is held to
the stricter bar the oracle makes possible: bit-exact per-sample radiance (NaN == NaN), RNG draw
counts, ray counts and scene.hit records."""
import glob
import os

import numpy as np
import pytest

import _harness as H
from _cases import pt_sample_list, pt_scene, random_rays, scene_digest

pytestmark = pytest.mark.gpu

GOLDENS = sorted(glob.glob(os.path.join(H.GOLDEN, "pt_*.npz")))
TOL = 1e-4  # north_star tolerance, per channel, L-inf (reported next to the bit-exact verdict)
# kernel modes (include/srt_pt.h) that take scenes with a real BVH<Triangle>; the second list also honours srt_pt_set_elision
MESH_KERNEL_MODES = (0, 1, 2, 4, 5, 6, 7)
MESH_ELISION_MODES = (2, 4, 6, 7)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def linf(a, b):
    m = np.isfinite(a) & np.isfinite(b)
    assert (np.isfinite(a) == np.isfinite(b)).all()
    return float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def make_pt(srt, scene, w, h, depth, use_bvh):
    pt = srt.Pathtracer(0)
    pt.set_params(w, h, 1, depth, use_bvh)
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])
    return pt


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(g)[3:-4] for g in GOLDENS])
def test_hip_matches_reference_golden(srt, path):
    g = np.load(path)
    w, h, depth, use_bvh, n = (int(x) for x in g["meta"])
    seed = int(g["seed"])
    scene = pt_scene(str(g["scene"]))
    assert scene_digest(scene) == str(g["scene_sha256"])
    pt = make_pt(srt, scene, w, h, depth, bool(use_bvh))
    xs, ys, ss = pt_sample_list(seed, w, h, n)
    rgb, draws, rays = pt.trace_samples(seed, xs, ys, ss)
    assert linf(rgb, g["rgb"]) <= TOL
    assert bits_equal(rgb, g["rgb"]), "per-sample radiance differs from the reference"
    assert np.array_equal(draws, g["draws"]), "RNG draw ledger differs from the reference"
    org, d, b = H.golden_rays(g, scene, seed + 1)
    assert bits_equal(pt.hit(org, d, b), g["hits"]), "scene.hit differs from the reference"
    pt.set_kernel(5)                     # the same query through the flattened per-lane walk (pt_flat.h)
    assert bits_equal(pt.hit(org, d, b), g["hits"]), "scene.hit through the flattened walk differs from the reference"
    pt.set_kernel(0)
    if "epoch" in g:
        ew, eh, spp, base = (int(x) for x in g["epoch_meta"])
        pt.set_params(ew, eh, spp, depth, bool(use_bvh))
        img = pt.render_epoch(seed, base, spp)
        assert linf(img, g["epoch"]) <= TOL
        assert bits_equal(img, g["epoch"]), "epoch image differs from the reference"
    pt.close()


@pytest.mark.parametrize("name,use_bvh,depth", [("cbox", True, 8), ("cbox_lambertian", True, 2), ("cbox", False, 8),
                                                ("cbox_blob2048_mirror", True, 8), ("cbox_blob512_glass", False, 4)])
def test_hip_matches_oracle_samples(srt, name, use_bvh, depth):
    scene = pt_scene(name)
    w, h = 57, 43
    pt = make_pt(srt, scene, w, h, depth, use_bvh)
    o = H.OraclePT(scene, w, h, depth, use_bvh, math_mode=1)
    xs, ys, ss = pt_sample_list(4242, w, h, 20000, max_sample=1 << 24)
    cnt = np.zeros(8, np.uint64)
    o_rgb, o_draws, o_rays = o.trace_samples(987654321, xs, ys, ss, cnt)
    rgb, draws, rays = pt.trace_samples(987654321, xs, ys, ss)
    assert bits_equal(rgb, o_rgb)
    assert np.array_equal(draws, o_draws) and np.array_equal(rays, o_rays)
    # the instrumented kernel walks the same nodes / objects / triangles as the oracle
    got = pt.counters()
    want = dict(zip(H.COUNTER_NAMES, (int(v) for v in cnt)))
    assert got == want, (got, want)
    pt.close()


def test_kernel_math_is_glibc_sincosf(srt):
    pt = srt.Pathtracer(0)
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(500000, dtype=np.float32) * np.float32(2 * np.pi), rng.random(500000, dtype=np.float32) * 2 - 1,
                        np.array([0.0, -0.0, 1e-5, 2 ** -13, 0.785398, 0.7853982, 1.5707964, 3.1415927, 6.2831855, 100.0, 119.9], np.float32)])
    c, s = pt.math_cos_sin(x)
    import ctypes

    oc, os_ = np.zeros_like(x), np.zeros_like(x)
    H.oracle().srt_oracle_math_cos_sin(H.P(x), ctypes.c_size_t(len(x)), H.P(oc), H.P(os_))
    assert bits_equal(c, oc) and bits_equal(s, os_)
    pt.close()


def test_kernel_math_is_glibc_atan2f(srt):
    from test_pt_oracle import _atan2_args
    import ctypes

    pt = srt.Pathtracer(0)
    y, x = _atan2_args(6, 300_000)
    got = pt.math_atan2(y, x)
    want = np.zeros_like(y)
    H.oracle().srt_oracle_math_atan2(H.P(y), H.P(x), ctypes.c_size_t(len(y)), H.P(want))
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert ok.all()
    pt.close()


def test_kernel_math_is_glibc_expf_powf(srt):
    """The epilogue's expf / powf on the device against the oracle's restatement (itself swept against the host libm):
    random arguments over every exponent, the overflow / underflow edges, the two arguments where an unfused evaluation
    rounds the other way, and powf over the sRGB range at 1/2.4 and over wide ranges at other exponents."""
    import ctypes

    pt = srt.Pathtracer(0)
    rng = np.random.default_rng(31)
    x = np.concatenate([rng.integers(0, 1 << 32, 2_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        -np.exp(rng.uniform(np.log(1e-8), np.log(120.0), 1_000_000)).astype(np.float32),
                        np.array([0.0, -0.0, 88.0, 88.72284, 88.7229, -103.97, -103.98, -104.5, np.inf, -np.inf, np.nan], np.float32),
                        np.array([0x4202422f, 0xc27c65d9], np.uint32).view(np.float32)])
    got = pt.math_exp(x)
    want = np.zeros_like(x)
    H.oracle().srt_oracle_math_exp(H.P(x), ctypes.c_size_t(len(x)), H.P(want))
    assert ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
    px = np.concatenate([rng.uniform(0.0031308, 1.0, 1_500_000).astype(np.float32),
                         np.exp(rng.uniform(np.log(1e-30), np.log(1e30), 1_500_000)).astype(np.float32),
                         np.array([0.0031308, 1.0, 0.5, 1e-45, 0.0, -1.0, np.inf, np.nan], np.float32)])
    py = np.concatenate([np.full(1_500_000, np.float32(1.0) / np.float32(2.4), np.float32),
                         rng.uniform(-12.0, 12.0, 1_500_000).astype(np.float32),
                         np.full(8, np.float32(1.0) / np.float32(2.4), np.float32)])
    got = pt.math_pow(px, py)
    want = np.zeros_like(px)
    H.oracle().srt_oracle_math_pow(H.P(px), H.P(py), ctypes.c_size_t(len(px)), H.P(want))
    assert ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
    pt.close()


def test_tonemap_matches_reference_golden(srt):
    """srt_pt_tonemap (HDR_Image::tonemap_to + Spectrum::to_srgb on the device) against the bytes the reference produced
    (tests/golden/tonemap_*.npz), against the oracle on a larger image with NaN / negative radiance, and the device-pointer
    form on a torch tensor."""
    import glob
    import os
    import torch
    from _cases import tonemap_image

    pt = srt.Pathtracer(0)
    paths = sorted(glob.glob(os.path.join(H.GOLDEN, "tonemap_*.npz")))
    assert len(paths) >= 4
    for path in paths:
        g = np.load(path)
        assert np.array_equal(pt.tonemap(g["rgb"], float(g["exposure"])), g["rgba"]), os.path.basename(path)
    rgb = tonemap_image("mixed", 1024, 768, 77)
    flat = rgb.reshape(-1)
    rng = np.random.default_rng(78)
    flat[rng.integers(0, flat.size, 5000)] = np.float32(np.nan)
    flat[rng.integers(0, flat.size, 5000)] = -np.abs(rng.normal(size=5000)).astype(np.float32)
    want = H.oracle_tonemap(rgb, 1.7)
    assert np.array_equal(pt.tonemap(rgb, 1.7), want)
    d_rgb = torch.from_numpy(rgb).cuda()
    d_out = torch.zeros((768, 1024, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pt.tonemap_device(d_rgb.data_ptr(), 1024, 768, 1.7, d_out.data_ptr())     # stream 0 = the HIP default stream = torch's
    assert np.array_equal(d_out.cpu().numpy(), want)
    # ordering on the caller's stream, no host synchronisation in between: accumulate_device then tonemap_device on one
    # (non-default) torch stream - the tone map must see the accumulated radiance, not the buffer's previous content
    S = torch.cuda.Stream()
    with torch.cuda.stream(S):
        d_acc = torch.full((768 * 1024 * 3,), 1e9, dtype=torch.float32, device="cuda")       # stale content: saturates every byte
        d_out2 = torch.zeros((768, 1024, 4), dtype=torch.uint8, device="cuda")
        big = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
        for _ in range(4):
            big.add_(1.0)                                                                       # keep the stream busy ahead of the pair
        d_acc.zero_()
        pt.accumulate_device(S.cuda_stream, d_acc.data_ptr(), d_rgb.data_ptr(), d_acc.numel(), 1)   # acc += (rgb - acc) * 1
        pt.tonemap_device(d_acc.data_ptr(), 1024, 768, 1.7, d_out2.data_ptr(), stream=S.cuda_stream)
    S.synchronize()
    assert np.array_equal(d_out2.cpu().numpy(), want)
    with pytest.raises(srt.SrtError):
        pt.tonemap(rgb, 0.0)
    assert pt.tonemap(np.zeros((0, 0, 3), np.float32), 1.0).shape == (0, 0, 4)
    pt.close()


def _div_sqrt_operands(seed, lanes):
    """Operands for srt_pt_math_div_sqrt: whole waves inside the fast paths' ranges (with their edges), then waves
    salted with the values that must send a wave through the full IEEE sequences."""
    rng = np.random.default_rng(seed)
    n3 = 3 * lanes

    def mags(lo_e, hi_e, n):
        m = np.ldexp(1.0 + rng.random(n), rng.integers(lo_e, hi_e, n)).astype(np.float32)
        return m * rng.choice(np.array([-1.0, 1.0], np.float32), n)

    planes = [mags(-40, 40, n3) for _ in range(4)]            # num0, num1, num2, den in [2^-40, 2^40)
    x = np.abs(mags(-96, 127, n3))
    edge = np.array([2.0 ** -40, 2.0 ** 40, -(2.0 ** -40), -(2.0 ** 40), 1.0, 3.0, 1.0 / 3.0], np.float32)
    for pl in planes:
        idx = rng.integers(0, n3 // 2, 4096)
        pl[idx] = rng.choice(edge, 4096)
    planes[2][rng.integers(0, n3 // 2, 20000)] = 0.0           # numerator of t: origin on the plane
    planes[2][rng.integers(0, n3 // 2, 2000)] = -0.0
    x[rng.integers(0, n3 // 2, 20000)] = 0.0
    x[rng.integers(0, n3 // 2, 4096)] = rng.choice(np.array([2.0 ** -96, 3.4028235e38, 1.0, 2.0, 4.0, 0.25], np.float32), 4096)
    # second half: specials sprinkled in (about four per wave)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 2.0 ** -41, 2.0 ** 41, 2.0 ** -126, 2.0 ** -100, 2.0 ** 100, 3.4028235e38,
                        -3.4028235e38, np.inf, -np.inf, np.nan, 2.0 ** -97, 2.0 ** -149, 1.1754942e-38], np.float32)
    for pl in planes + [x]:
        idx = rng.integers(n3 // 2, n3, n3 // 96)
        pl[idx] = rng.choice(special, len(idx))
    x[rng.integers(n3 // 2, n3, 3000)] = -1.0
    return planes[0], planes[1], planes[2], planes[3], x


def test_exact_division_and_sqrt_fast_paths(srt):
    """div3x3 / sqrt3 of the wave kernel (refinement shared per denominator, range handling hoisted to one verdict per wave)
    return the correctly rounded quotient and root for every operand: compared bit for bit with the host's `/` and sqrt."""
    pt = srt.Pathtracer(0)
    lanes = 1 << 19
    for seed, shared in ((21, False), (22, True), (23, True)):
        n0, n1, n2, den, x = _div_sqrt_operands(seed, lanes)
        if shared:
            n2 = np.repeat(n2[0::3], 3)
        q0, q1, q2, root = pt.math_div_sqrt(n0, n1, n2, den, x, shared_c2=shared)
        with np.errstate(all="ignore"):
            want = [n0 / den, n1 / den, n2 / den, np.sqrt(x)]
        for got, w in zip((q0, q1, q2, root), want):
            assert w.dtype == np.float32
            ok = (got.view(np.uint32) == w.view(np.uint32)) | (np.isnan(got) & np.isnan(w))
            bad = np.flatnonzero(~ok)
            assert bad.size == 0, (seed, bad[:5], got[bad[:5]], w[bad[:5]])
    pt.close()


def test_delta_lights(srt):
    """Point, spot and directional lights (Pathtracer::point_lighting): the per-lane kernels and the wave kernel's
    shadow batches against the oracle, the shadow rays counted; the builds without point_lighting (flattened walk,
    stamped) refuse such scenes instead of ignoring the lights."""
    scene = pt_scene("cbox_deltalights")
    w, h, spp = 40, 32, 5
    want = H.OraclePT(scene, w, h, 8, True).epoch(3, 2, spp)
    plain = H.OraclePT(pt_scene("cbox"), w, h, 8, True).epoch(3, 2, spp)
    assert not bits_equal(want, plain)
    pt = make_pt(srt, scene, w, h, 8, True)
    rays = []
    for mode in (0, 1, 2, 4, 6):
        pt.set_kernel(mode)
        pt.ray_count(reset=True)
        assert bits_equal(pt.render_epoch(3, 2, spp), want), f"kernel mode {mode}"
        rays.append(pt.ray_count()[0])
    assert len(set(rays)) == 1
    for mode in (3, 5):
        pt.set_kernel(mode)
        with pytest.raises(srt.SrtError):
            pt.render_epoch(3, 2, spp)
    pt.close()


def test_many_objects(srt):
    """A BVH<Object> of 74 objects (what a particle system becomes): the streamed form and the per-lane kernels against the
    oracle, BVH and list; the wave-uniform sweeps refuse it."""
    scene = pt_scene("cbox_particles")
    w, h, spp = 40, 32, 3
    pt = make_pt(srt, scene, w, h, 6, True)
    want = H.OraclePT(scene, w, h, 6, True).epoch(4, 0, spp)
    for mode in (0, 1, 4, 6):                # auto = the streamed form (logic + ray-cast kernels): any number of objects
        pt.set_kernel(mode)
        assert bits_equal(pt.render_epoch(4, 0, spp), want), f"kernel mode {mode}"
    pt.set_kernel(6)
    pt.set_elision(True)
    pt.rays_elided(reset=True)
    assert bits_equal(pt.render_epoch(4, 0, spp), want) and pt.rays_elided() > 0
    pt.set_elision(False)
    pt.set_kernel(0)
    org, d, b = random_rays(5, 3000)
    assert bits_equal(pt.hit(org, d, b), H.OraclePT(scene, w, h, 6, True).hit(org, d, b))
    for mode in (2, 5):
        pt.set_kernel(mode)
        with pytest.raises(srt.SrtError):
            pt.render_epoch(4, 0, spp)
    pt.close()
    pt = make_pt(srt, scene, w, h, 6, False)
    assert bits_equal(pt.render_epoch(4, 0, 2), H.OraclePT(scene, w, h, 6, False).epoch(4, 0, 2))
    pt.close()


def test_particle_step_and_unnormalised_rays(srt):
    """srt_pt_particles_step (Scene_Particles::Particle::update on the device) against the reference-built
    fixture over three steps and against the oracle on a larger cloud in the 74-object particle scene; srt_pt_hit with the rays
    the step sends: un-normalised directions, bounds [0, inf]."""
    from _cases import particle_cloud, unnormalised_rays

    g = np.load(os.path.join(H.GOLDEN, "particles_cbox_blob512.npz"))
    scene = pt_scene(str(g["scene"]))
    assert scene_digest(scene) == str(g["scene_sha256"])
    seed, n, steps = (int(v) for v in g["meta"])
    pt = make_pt(srt, scene, 8, 8, 8, True)
    pos, vel, age = particle_cloud(seed, n)
    for s in range(steps):
        pos, vel, age, alive = pt.particles_step(pos, vel, age, float(g["dt"]), float(g["radius"]))
        assert bits_equal(pos, g[f"pos{s}"]) and bits_equal(vel, g[f"vel{s}"]) and bits_equal(age, g[f"age{s}"]), f"step {s}"
        assert np.array_equal(alive, g[f"alive{s}"])
    org, d, b = unnormalised_rays(seed + 7, 1024)
    assert bits_equal(pt.hit(org, d, b), g["hits_unnormalised"]), "scene.hit with un-normalised directions differs from the reference"
    pt.set_kernel(5)
    assert bits_equal(pt.hit(org, d, b), g["hits_unnormalised"])
    pt.close()
    scene = pt_scene("cbox_particles")
    pt = make_pt(srt, scene, 8, 8, 8, True)
    o = H.OraclePT(scene, 8, 8, 8, True)
    pos, vel, age = particle_cloud(99, 50000)
    for s in range(2):
        want = o.particles_update(pos, vel, age, 0.01, 0.015)
        got = pt.particles_step(pos, vel, age, 0.01, 0.015)
        assert all(bits_equal(x, y) for x, y in zip(got[:3], want[:3])) and np.array_equal(got[3], want[3]), f"step {s}"
        pos, vel, age = got[:3]
    assert pt.particles_step(pos[:0], vel[:0], age[:0], 0.01, 0.015)[3].shape == (0,)
    pt.close()


def test_emissive_sphere(srt):
    """An emissive analytic sphere (intersected as a sphere, sampled through its mesh approximation) on every kernel."""
    scene = pt_scene("cbox_spherelight")
    w, h, spp = 36, 28, 6
    want = H.OraclePT(scene, w, h, 8, True).epoch(8, 1, spp)
    pt = make_pt(srt, scene, w, h, 8, True)
    for mode in (0, 1, 2, 4, 5, 6):
        pt.set_kernel(mode)
        assert bits_equal(pt.render_epoch(8, 1, spp), want), f"kernel mode {mode}"
    pt.close()


def test_environment_map(srt):
    """Env_Map (image environment light): the per-lane kernels and the wave kernel (camera rays that leave the scene look the
    map up from their regenerated direction when the sample is resolved) against the oracle."""
    scene = pt_scene("cbox_envmap")
    w, h, spp = 36, 28, 6
    want = H.OraclePT(scene, w, h, 8, True).epoch(8, 1, spp)
    pt = make_pt(srt, scene, w, h, 8, True)
    rays = set()
    for mode in (0, 1, 2, 4, 6):
        pt.set_kernel(mode)
        pt.ray_count(reset=True)
        assert bits_equal(pt.render_epoch(8, 1, spp), want), f"kernel mode {mode}"
        rays.add(pt.ray_count()[0])
    assert len(rays) == 1
    pt.close()


@pytest.mark.parametrize("name", ["cbox_envsphere", "cbox_envhemi", "cbox_envonly"])
def test_environment_lights(srt, name):
    """Env_Sphere / Env_Hemisphere: rays that leave the scene, sample_area_lights' coin flip, area_lights_pdf's mean -
    per-lane kernels and the wave kernel against the oracle; the builds without environment lights (flattened walk,
    stamped) refuse the scene instead of ignoring the light."""
    scene = pt_scene(name)
    w, h, spp = 36, 28, 7
    want = H.OraclePT(scene, w, h, 8, True).epoch(8, 1, spp)
    pt = make_pt(srt, scene, w, h, 8, True)
    for mode in (0, 1, 2, 4, 6):
        pt.set_kernel(mode)
        assert bits_equal(pt.render_epoch(8, 1, spp), want), f"kernel mode {mode}"
    for mode in (3, 5):
        pt.set_kernel(mode)
        with pytest.raises(srt.SrtError):
            pt.render_epoch(8, 1, spp)
    pt.close()


def test_kernel_math_is_glibc_acosf(srt):
    pt = srt.Pathtracer(0)
    x = np.concatenate([np.random.default_rng(3).random(300000, dtype=np.float32) * 2 - 1,
                        np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.49999997, 1e-20, 1.5, np.nan], np.float32)])
    got = pt.math_acos(x)
    import ctypes
    want = np.zeros_like(x)
    H.oracle().srt_oracle_math_acos(H.P(x), ctypes.c_size_t(len(x)), H.P(want))
    assert ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all()
    pt.close()


def test_epoch_image_and_tiling(srt):
    """cfg3-shaped run at reduced size: epoch images equal the oracle's; sharding the image over 1, 2 and 3
    ranks (tile round-robin) produces the same pixels; the device untile + accumulate path equals the host one."""
    import torch

    scene = pt_scene("cbox_lambertian")
    w, h, spp = 72, 40, 6   # not a multiple of the tile size
    o = H.OraclePT(scene, w, h, 8, True)
    want = o.epoch(11, 5, spp)
    pt = make_pt(srt, scene, w, h, 8, True)
    full = pt.render_epoch(11, 5, spp)
    assert bits_equal(full, want)
    for world in (2, 3):
        img = np.full((h, w, 3), -1.0, np.float32)
        for rank in range(world):
            pt.set_tiling(16, 8, rank, world)
            pt.render_epoch(11, 5, spp, out=img)
        assert bits_equal(img, want)
    # device path: per-rank tile buffers -> "gather" (concatenate rank-major) -> untile -> accumulate
    world = 3
    bufs = []
    for rank in range(world):
        pt.set_tiling(16, 8, rank, world)
        local, per_rank, fpt = pt.tile_info()
        t = torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda")
        pt.render_epoch_device(torch.cuda.current_stream().cuda_stream, 11, 5, spp, t.data_ptr())
        bufs.append(t)
    gathered = torch.cat(bufs)
    image = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    pt.untile_device(torch.cuda.current_stream().cuda_stream, gathered.data_ptr(), image.data_ptr())
    torch.cuda.synchronize()
    assert bits_equal(image.cpu().numpy().reshape(h, w, 3), want), "gather + untile differs from the single-rank image"
    acc = torch.full_like(image, 0.25)
    for k in (1, 2, 3):
        pt.accumulate_device(torch.cuda.current_stream().cuda_stream, acc.data_ptr(), image.data_ptr(), image.numel(), k)
    torch.cuda.synchronize()
    ref_acc = np.full((h, w, 3), 0.25, np.float32)
    for k in (1, 2, 3):
        H.oracle_accumulate(ref_acc, want, k)
    assert bits_equal(acc.cpu().numpy().reshape(h, w, 3), ref_acc)
    pt.close()


def test_pathtracer_surface_running_mean(srt):
    """set_params -> begin_render -> get_output with the reference's epoch scheme (running mean of epoch means)."""
    scene = pt_scene("cbox")
    w, h, n = 24, 24, 10
    pt = srt.Pathtracer(0, n_threads=1)        # samples_per_epoch = max(1, 10 // 10) = 1 -> 10 epochs
    pt.set_params(w, h, n, 8, True)
    pt.begin_render(scene)
    assert not pt.in_progress() and pt.progress() == 1.0 and pt.total_epochs == 10
    o = H.OraclePT(scene, w, h, 8, True)
    acc = np.zeros((h, w, 3), np.float32)
    for k in range(n):
        H.oracle_accumulate(acc, o.epoch(0, k, 1), k + 1)
    assert bits_equal(pt.get_output(), acc)
    # "Add Samples" keeps the accumulator and continues the sample index (rays/pathtracer.cpp:258-264)
    pt.set_samples(4)
    pt.begin_render(scene, add_samples=True, samples_per_epoch=2)
    for k in range(2):
        H.oracle_accumulate(acc, o.epoch(0, n + 2 * k, 2), n + k + 1)
    assert bits_equal(pt.get_output(), acc)
    pt.close()


def test_full_size_properties(srt):
    """BASELINE configs[3] image size (1024x1024) at 1 spp: (1) deterministic — two runs are bit-identical;
    (2) samples are independent of the launch shape — a random subset re-traced one by one matches the epoch;
    (3) every pixel that sees the light directly returns exactly the emitted radiance (10,10,10)."""
    scene = pt_scene("cbox")
    w = h = 1024
    pt = make_pt(srt, scene, w, h, 8, True)
    a = pt.render_epoch(7, 0, 1)
    b = pt.render_epoch(7, 0, 1)
    assert bits_equal(a, b)
    xs, ys, _ = pt_sample_list(3, w, h, 5000)
    rgb, _, rays = pt.trace_samples(7, xs, ys, np.zeros(5000, np.uint32))
    assert bits_equal(rgb, a[ys, xs])
    direct = rays == 1
    assert set(map(tuple, rgb[direct].tolist())) <= {(10.0, 10.0, 10.0), (0.0, 0.0, 0.0)}
    pt.close()


FULLSIZE = H.load_fullsize()


@pytest.mark.parametrize("case", sorted(FULLSIZE), ids=sorted(FULLSIZE))
def test_full_size_epoch_equals_reference_hash(srt, case):
    """BASELINE configs[2..4] at their image sizes through the PRODUCTION kernels: `auto` mode with the default population
    (the persistent wave kernel for the Cornell boxes, the streamed sweeps with 2 Mi path slots for the box + large mesh),
    with and without dead-ray elision (what the drop-in class runs), and - for the streamed forms - once more with 4096
    path slots so that every slot is recycled hundreds of times.  Expected: the SHA-256 of the epoch image the REFERENCE's own
    code (oracle/_ref/libref_pt.so) produced in the authoring container, tests/golden/pt_fullsize.json
    (make_pt_fullsize_golden.py); nothing of the reference is needed on the GPU box."""
    g = FULLSIZE[case]
    scene = pt_scene(g["scene"])
    assert scene_digest(scene) == g["scene_sha256"]
    pt = make_pt(srt, scene, g["w"], g["h"], g["max_depth"], True)
    pt.set_kernel(0)

    def check(what):
        img = pt.render_epoch(g["seed"], g["sample_base"], g["spp"])
        fin = np.isfinite(img).all(axis=2)
        x0, y0 = g["crop_origin"]
        crop = np.frombuffer(bytes.fromhex(g["crop_hex"]), np.float32).reshape(16, 16, 3)
        assert int((~fin).sum()) == g["nonfinite_pixels"], what
        assert bits_equal(img[y0:y0 + 16, x0:x0 + 16], crop), f"{what}: centre crop differs from the reference"
        assert H.sha(img) == g["sha256"], f"{what}: epoch image differs from the reference (mean {img[fin].mean(dtype=np.float64):.6f} vs {g['mean_finite']:.6f})"

    form = pt.kernel_form()
    assert form in (0, 4), f"auto mode took kernel form {form} for {case}"
    check(f"auto (form {form})")
    pt.set_elision(True)
    check(f"auto (form {form}) with dead-ray elision")
    pt.set_elision(False)
    if form >= 3:
        pt.set_stream_slots(4096)
        check("streamed, 4096 path slots")
        pt.set_stream_slots(0)
    pt.close()


@pytest.mark.parametrize("name,use_bvh,wh,spp,depth", [
    ("cbox", True, (72, 40), 6, 8),               # edge tiles with padding pixels
    ("cbox_lambertian", True, (64, 64), 70, 3),   # > 64 spp: two launches, running (sum, count)
    ("cbox", False, (32, 32), 5, 8),              # List<Object> / List<Triangle>
    ("cbox_blob512_glass", True, (40, 40), 4, 8), # one object with a real BVH<Triangle> (per-lane walk inside)
    ("cbox_nolight", True, (32, 32), 3, 4),       # NaN rays, every sample invalid
    ("cbox_refract", True, (32, 32), 3, 8),
])
def test_wave_kernel_equals_general_kernel_and_oracle(srt, name, use_bvh, wh, spp, depth):
    """The wave-uniform persistent kernel (mode 2), the same kernel with the flattened per-lane walk (mode 5), the
    streamed form (mode 6: logic + ray-cast kernels) and the general per-lane kernels (modes 1, 4) are independent device
    implementations of the epoch; all must reproduce the oracle's epoch image bit for bit."""
    scene = pt_scene(name)
    w, h = wh
    want = H.OraclePT(scene, w, h, depth, use_bvh).epoch(5, 9, spp)
    pt = make_pt(srt, scene, w, h, depth, use_bvh)
    rays = []
    for mode in (1, 2, 4, 5, 6):
        pt.set_kernel(mode)
        pt.ray_count(reset=True)
        img = pt.render_epoch(5, 9, spp)
        assert bits_equal(img, want), f"kernel mode {mode} differs from the oracle"
        rays.append(pt.ray_count()[0])
    assert len(set(rays)) == 1 and rays[0] > 0               # all kernels trace exactly the same rays
    pt.set_kernel(2)
    pt.set_tiling(16, 8, 1, 3)         # sharded: rank 1 of 3
    part = np.full((h, w, 3), -1.0, np.float32)
    pt.render_epoch(5, 9, spp, out=part)
    mask = part[..., 0] != -1.0
    assert mask.any() and not mask.all() and bits_equal(part[mask], want[mask])
    pt.close()


@pytest.mark.parametrize("scene_name,size,min_hits", [("cbox_blob131072_glass", 1024, 600), ("cbox_beast_glass", 512, 200)])
def test_cfg5_large_mesh_every_kernel(srt, scene_name, size, min_hits):
    """BASELINE configs[4] at size: the Cornell box with a 131 072-triangle glass mesh (80 127-node BVH<Triangle>, depth 18),
    and with the reference's own largest asset (media/beast.dae, 64 618 triangles, posed by a rotation + scale).
    Per-sample radiance, RNG ledger, per-sample ray counts and the traversal counters against the oracle (4 k samples of
    the 1024 x 1024 image), 2 k scene.hit records through the nested and the flattened walk, and one epoch image through
    every kernel mode - the wave kernel's compacted BLAS walks with three- and two-ray batches (dead-ray elision), lane
    per sample, lane per pixel, flattened walk, streamed wavefront - plus a shard of it.  The reference-built fixture of
    the same scene is covered by test_hip_matches_reference_golden."""
    scene = pt_scene(scene_name)
    w = h = size
    pt = make_pt(srt, scene, w, h, 8, True)
    o = H.OraclePT(scene, w, h, 8, True, math_mode=1)
    xs, ys, ss = pt_sample_list(77, w, h, 4096, max_sample=1024)
    cnt = np.zeros(8, np.uint64)
    o_rgb, o_draws, o_rays = o.trace_samples(5, xs, ys, ss, cnt)
    rgb, draws, rays = pt.trace_samples(5, xs, ys, ss)
    assert bits_equal(rgb, o_rgb) and np.array_equal(draws, o_draws) and np.array_equal(rays, o_rays)
    assert pt.counters() == dict(zip(H.COUNTER_NAMES, (int(v) for v in cnt)))
    org, d, b = random_rays(78, 2048)
    org = (org * np.float32(0.6) + np.array([0.05, 0.15, 0.1], np.float32)).astype(np.float32)   # most rays meet the mesh
    want_hits = o.hit(org, d, b)
    assert int(want_hits[:, 0].sum()) > min_hits
    for mode in (0, 5):
        pt.set_kernel(mode)
        assert bits_equal(pt.hit(org, d, b), want_hits), f"scene.hit (kernel mode {mode}) differs from the oracle"
    ew, eh, spp = 96, 64, 3
    pt.set_params(ew, eh, spp, 8, True)
    want = H.OraclePT(scene, ew, eh, 8, True).epoch(11, 2, spp)
    counts = []
    for mode in MESH_KERNEL_MODES:
        pt.set_kernel(mode)
        pt.ray_count(reset=True)
        assert bits_equal(pt.render_epoch(11, 2, spp), want), f"kernel mode {mode} differs from the oracle on the large mesh"
        counts.append(pt.ray_count()[0])
    assert len(set(counts)) == 1 and counts[0] > 0
    pt.set_elision(True)
    for mode in MESH_ELISION_MODES:
        pt.set_kernel(mode)
        pt.ray_count(reset=True); pt.rays_elided(reset=True)
        assert bits_equal(pt.render_epoch(11, 2, spp), want), f"kernel mode {mode} with elision differs from the oracle"
        assert pt.ray_count()[0] == counts[0] and pt.rays_elided() > 0
    pt.set_elision(False)
    pt.set_kernel(0)
    pt.set_tiling(32, 16, 2, 5)        # rank 2 of 5
    part = np.full((eh, ew, 3), -1.0, np.float32)
    pt.render_epoch(11, 2, spp, out=part)
    mask = part[..., 0] != -1.0
    assert mask.any() and not mask.all() and bits_equal(part[mask], want[mask])
    pt.close()


@pytest.mark.parametrize("name,use_bvh,wh,spp,depth,expect_elided", [
    ("cbox", True, (72, 40), 6, 8, True),                # mirror + glass + Lambertian walls, edge tiles
    ("cbox_lambertian", True, (64, 64), 71, 3, True),    # two launches, odd sample count (pairs + single-sample units)
    ("cbox", False, (32, 32), 5, 8, True),               # List<Object> / List<Triangle>
    ("cbox", True, (24, 16), 1, 8, True),                # bursts of one sample
    ("cbox", True, (16, 16), 2, 0, False),               # depth 0: no bounce, nothing to elide
    ("cbox_blob512_glass", True, (40, 40), 4, 8, True),  # real BVH<Triangle> inside the sweeps
    ("cbox_nolight", True, (32, 32), 3, 4, True),        # NaN radiance either way
    ("cbox_refract", True, (32, 32), 3, 8, True),
    ("cbox_deltalights", True, (32, 24), 3, 8, False),   # point_lighting != 0: the ray is live, the switch is ignored
    ("cbox_envsphere", True, (32, 24), 3, 8, False),     # environment light: ignored too
])
def test_dead_ray_elision_is_bit_identical(srt, name, use_bvh, wh, spp, depth, expect_elided):
    """srt_pt_set_elision: the wave kernel's two-ray batches (BSDF-sampled direct ray of a Lambertian bounce not traced)
    give the oracle's epoch image bit for bit, count the same reference rays, and report how many were not traced."""
    scene = pt_scene(name)
    w, h = wh
    want = H.OraclePT(scene, w, h, depth, use_bvh).epoch(5, 9, spp)
    pt = make_pt(srt, scene, w, h, depth, use_bvh)
    pt.set_kernel(2)
    pt.ray_count(reset=True)
    full = pt.render_epoch(5, 9, spp)
    rays_full = pt.ray_count(reset=True)[0]
    assert bits_equal(full, want) and pt.rays_elided(reset=True) == 0
    pt.set_elision(True)
    counts = []
    for mode in (2, 4, 1):                                # wave kernel (two-ray batches), lane per sample, lane per pixel
        pt.set_kernel(mode)
        img = pt.render_epoch(5, 9, spp)
        rays, elided = pt.ray_count(reset=True)[0], pt.rays_elided(reset=True)
        assert bits_equal(img, want), f"elision changed the image (mode {mode})"
        assert rays == rays_full, "the reference-equivalent ray count must not depend on elision"
        assert (0 < elided < rays) if expect_elided else elided == 0
        counts.append(elided)
    assert counts[0] == counts[1] == counts[2]            # the same rays are dead for every kernel
    if "delta" not in name and "env" not in name:         # (the flattened walk has no point_lighting: it refuses those scenes)
        pt.set_kernel(5)                                  # flattened walk: the switch is ignored
        assert bits_equal(pt.render_epoch(5, 9, spp), want) and pt.rays_elided(reset=True) == 0
    pt.ray_count(reset=True)
    pt.set_kernel(2)
    pt.set_tiling(16, 8, 2, 3)          # sharded + elided
    part = np.full((h, w, 3), -1.0, np.float32)
    pt.render_epoch(5, 9, spp, out=part)
    mask = part[..., 0] != -1.0
    assert bits_equal(part[mask], want[mask])
    pt.close()


def test_random_scenes_all_kernels(srt):
    """Differential check on seeded random scenes (tests/_cases.py:random_pt_scene - jittered walls, spheres, one-leaf meshes
    and blobs with a real BVH<Triangle> under random poses and materials): every kernel, with and without dead-ray elision,
    reproduces the oracle's epoch image bit for bit and counts the same rays.  tools/fuzz_pt.py runs the same loop over
    thousands of seeds."""
    from _cases import random_pt_scene

    checked = 0
    # the second range also draws delta / uniform environment lights, the third image environment maps, the fourth a world off
    # unit scale: translated, scaled in the geometry or in the pose, now and then projective (300025: a commit both refuse)
    for seed in list(range(300, 340)) + list(range(100000, 100016)) + list(range(200000, 200010)) + list(range(300000, 300010)) + [300025]:
        scene, w, h, depth, use_bvh, spp = random_pt_scene(seed)
        try:
            want = H.OraclePT(scene, w, h, depth, use_bvh).epoch(seed, 3, spp)
        except AssertionError:              # the reference's BVH build does not terminate on this input; the product refuses it too
            pt = srt.Pathtracer(0)
            pt.set_params(w, h, 1, depth, use_bvh)
            with pytest.raises(srt.SrtError):
                pt.build_scene(scene)
            pt.close()
            continue
        pt = make_pt(srt, scene, w, h, depth, use_bvh)
        rays = set()
        for mode, elide in ((2, False), (2, True), (4, True), (1, False), (5, False), (6, False), (6, True), (7, False), (7, True)):
            pt.set_kernel(mode)
            pt.set_elision(elide)
            pt.ray_count(reset=True)
            try:
                img = pt.render_epoch(seed, 3, spp)
            except srt.SrtError as e:       # a kernel that does not take scenes of this size says so
                assert "objects" in str(e)     # too many objects, or a build without point_lighting for a scene with lights
                continue
            assert bits_equal(img, want), f"seed {seed} mode {mode} elide {elide}"
            rays.add(pt.ray_count()[0])
        assert len(rays) == 1
        pt.close()
        checked += 1
    assert checked >= 40


@pytest.mark.parametrize("w,h,depth,spp,tile,world", [
    (1, 1, 8, 7, (8, 8), 1),        # one pixel
    (5, 3, 0, 4, (8, 8), 1),        # max_depth 0: only emitted light seen directly
    (19, 11, 16, 2, (16, 8), 1),    # deepest supported recursion
    (40, 24, 2, 1, (64, 32), 1),    # tile larger than the image, 1 spp (burst with a single sample)
    (16, 16, 3, 5, (8, 8), 7),      # more ranks than some ranks have tiles for
])
def test_edge_shapes(srt, w, h, depth, spp, tile, world):
    scene = pt_scene("cbox")
    want = H.OraclePT(scene, w, h, depth, True).epoch(2**40 + 12345, 2**31 - 3, spp)   # large seed / sample base
    pt = make_pt(srt, scene, w, h, depth, True)
    for mode in (2, 4, 5, 6):
        pt.set_kernel(mode)
        img = np.full((h, w, 3), -7.0, np.float32)
        for rank in range(world):
            pt.set_tiling(tile[0], tile[1], rank, world)
            pt.render_epoch(2**40 + 12345, 2**31 - 3, spp, out=img)
        assert bits_equal(img, want), f"mode {mode}"
    pt.close()


def test_zero_samples_and_reuse(srt):
    """An epoch of zero samples is an image of zeros (do_trace with samples = 0); a context can be re-committed."""
    pt = make_pt(srt, pt_scene("cbox"), 16, 16, 8, True)
    assert not pt.render_epoch(1, 0, 0).any()
    a = pt.render_epoch(1, 0, 3)
    pt.build_scene(pt_scene("cbox_lambertian"))      # new scene in the same context
    b = pt.render_epoch(1, 0, 3)
    want = H.OraclePT(pt_scene("cbox_lambertian"), 16, 16, 8, True).epoch(1, 0, 3)
    assert bits_equal(b, want) and not bits_equal(a, b)
    pt.close()


def test_large_image_multi_launch(srt):
    """An image large enough that one launch handles fewer than 64 samples per pixel (the per-sample buffer is capped):
    4096x2048 at 20 spp = two launches of 16 + 4; 64 random pixels are checked against per-sample radiance from the
    instrumented kernel, summed in sample order the way do_trace does."""
    scene = pt_scene("cbox_lambertian")
    w, h, spp = 4096, 2048, 20
    pt = make_pt(srt, scene, w, h, 8, True)
    img = pt.render_epoch(11, 5, spp)
    rng = np.random.default_rng(0)
    xs = rng.integers(0, w, 64).astype(np.uint32)
    ys = rng.integers(0, h, 64).astype(np.uint32)
    for x, y in zip(xs, ys):
        rgb, _, _ = pt.trace_samples(11, np.full(spp, x, np.uint32), np.full(spp, y, np.uint32), np.arange(5, 5 + spp, dtype=np.uint32))
        acc = np.zeros(3, np.float32)
        n = 0
        for s in range(spp):
            if np.isfinite(rgb[s]).all():
                acc = (acc + rgb[s]).astype(np.float32)
                n += 1
        want = (acc * np.float32(1.0 / n)).astype(np.float32) if n else acc
        assert bits_equal(img[y, x], want), (x, y)
    pt.close()


def test_epochs_on_two_streams_overlap_safely(srt):
    """Epochs launched alternately on two streams (each stream has its own epoch scratch in the library, so consecutive
    launches may overlap on the device) give the same tiles as the same epochs on one stream."""
    import torch

    scene = pt_scene("cbox")
    w, h, spp = 96, 64, 9
    pt = make_pt(srt, scene, w, h, 8, True)
    pt.set_tiling(32, 32, 0, 1)
    _, per_rank, fpt = pt.tile_info()
    one = torch.cuda.current_stream()
    want = []
    for i in range(6):
        t = torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda")
        pt.render_epoch_device(one.cuda_stream, 3, i * spp, spp, t.data_ptr())
        want.append(t)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    got = [torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    for i in range(6):
        pt.render_epoch_device(streams[i % 2].cuda_stream, 3, i * spp, spp, got[i].data_ptr())
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    pt.close()


@pytest.mark.parametrize("scene_name,min_prims", [("cbox_blob512_glass", 1), ("cbox_blob2048_mirror", 1), ("cbox_beast_glass", 16384),
                                                  ("cbox_blob131072_glass", 16384),
                                                  ("deep_max", 1)])      # a skewed tree: one level per triangle, 48 = kMaxBlasDepth deep
def test_device_bvh_build_equals_host_build(srt, scene_name, min_prims):
    """BVH::build on the GPU (csrc/pt_bvh_device.hip): node boxes, links and primitive order of every tree - the BVH<Object> too
    when min_prims = 1 - equal the host build's bit for bit (the host build equals the reference's: tests/test_pt_host.py and
    the goldens' node arrays), and scene.hit agrees with the oracle through the device-built trees."""
    import time
    scene = pt_scene(scene_name)
    built = []
    for device in (False, True):
        pt = srt.Pathtracer(0)
        pt.set_params(64, 64, 1, 8, True)
        pt.set_bvh_builder(device, min_prims)
        t0 = time.perf_counter()
        pt.build_scene(scene)
        dt = time.perf_counter() - t0
        pt.set_camera(scene["camera"])
        trees = [pt.dump_bvh(-1)]
        for slot in range(len(scene["objects"])):          # (slots of BVH<Object> order; spheres have no tree)
            try:
                trees.append(pt.dump_bvh(slot))
            except Exception:
                pass
        built.append((pt, trees, dt))
    (pt_h, trees_h, dt_h), (pt_d, trees_d, dt_d) = built
    print(f"{scene_name}: build_scene host {dt_h * 1e3:.1f} ms, device {dt_d * 1e3:.1f} ms")
    assert len(trees_h) == len(trees_d)
    for (bh, lh, oh), (bd, ld, od) in zip(trees_h, trees_d):
        assert bits_equal(bh, bd) and np.array_equal(lh, ld) and np.array_equal(oh, od)
    org, d, b = random_rays(91, 1024)
    assert bits_equal(pt_h.hit(org, d, b), pt_d.hit(org, d, b))
    if scene_name.startswith("deep_"):
        # a generated scene without a reference-built fixture: the oracle's build stands in for it (tests/test_pt_stack_depth_host.py)
        o = H.OraclePT(scene, 8, 8, 4, True)
        checked = 0
        for k in range(-1, len(scene["objects"])):
            want = o.dump_bvh(k)
            if want is not None:
                bd, ld, od = pt_d.dump_bvh(k)
                n = len(scene["objects"]) if k < 0 else len(want[0])
                assert bits_equal(bd, want[0]) and np.array_equal(ld, want[1]) and np.array_equal(od[:n], want[2][:n])
                checked += int(k >= 0 and len(want[0]) > 90)
        assert checked == 1, "the chain's BVH<Triangle> was not compared"
        pt_h.close(); pt_d.close()
        return
    # ... and, directly, the REFERENCE build's node arrays of the same scene (the goldens of tests/golden/make_pt_golden.py)
    gpath = glob.glob(os.path.join(H.GOLDEN, f"pt_{scene_name}_*_bvh.npz"))
    assert gpath, scene_name
    g = np.load(gpath[0])
    assert scene_digest(scene) == str(g["scene_sha256"])
    boxes, links, order = pt_d.dump_bvh(-1)
    assert bits_equal(boxes, g["tlas_boxes"]) and np.array_equal(links, g["tlas_links"]) and np.array_equal(order[: len(scene["objects"])], g["tlas_order"])
    checked = 0
    for k in range(len(scene["objects"])):
        try:
            checked += bool(H.check_blas_against_golden(g, k, pt_d.dump_bvh))
        except srt.SrtError:
            pass                                             # an object slot without a mesh
    assert checked >= 1, "no BVH<Triangle> of this scene was compared with the reference's"
    pt_h.close(); pt_d.close()


@pytest.mark.parametrize("name", ["lone_blob_env", "lone_blob_env_lambertian"])
def test_single_object_scene_every_kernel(srt, name):
    """A scene of one mesh with a real BVH<Triangle> (BVH<Object> root = leaf: the sweeps have no interior node, the streamed
    sweeps queue the mesh from the object fold) under an environment light: every kernel form against the oracle."""
    scene = pt_scene(name)
    w, h, spp = 48, 40, 5
    want = H.OraclePT(scene, w, h, 6, True).epoch(3, 1, spp)
    pt = make_pt(srt, scene, w, h, 6, True)
    pt.set_params(w, h, spp, 6, True)
    forms = {}
    for mode in (0, 1, 2, 4, 6, 7):
        pt.set_kernel(mode)
        forms[mode] = pt.kernel_form()
        assert bits_equal(pt.render_epoch(3, 1, spp), want), f"kernel mode {mode} (form {forms[mode]}) differs from the oracle"
    assert forms[7] == 4 and forms[6] == 3, forms
    pt.close()


LOG_GOLDENS = sorted(glob.glob(os.path.join(H.GOLDEN, "ptlog_*.npz")))


@pytest.mark.parametrize("path", LOG_GOLDENS, ids=[os.path.basename(g)[6:-4] for g in LOG_GOLDENS])
def test_ray_log_equals_reference_golden(srt, path):
    """Pathtracer::log_ray: the rays the 0.0005 coin of sample_direct_lighting selects are recorded by
    every kernel form and come back through srt_pt_read_ray_log exactly as the reference build handed them to the GUI - point,
    direction, t = 5, per (pixel, sample) in bounce order - and their number is what the coin's probability predicts."""
    g = np.load(path)
    w, h, depth, use_bvh, spp, base = (int(x) for x in g["meta"])
    scene = pt_scene(str(g["scene"]))
    assert scene_digest(scene) == str(g["scene_sha256"])
    seed = int(g["seed"])
    order = np.lexsort((g["bounce"], g["sample"], g["pixel"]))           # the C ABI's order: pixel, sample, bounce
    pt = make_pt(srt, scene, w, h, depth, bool(use_bvh))
    forms = set()
    for mode in (0, 1, 2, 4, 5, 6, 7):
        for elide in (False, True):
            pt.set_kernel(mode)
            pt.set_elision(elide)
            pt.set_ray_log(4096)
            try:
                img = pt.render_epoch(seed, base, spp)
            except srt.SrtError:
                continue                                                  # a form that does not take this scene
            forms.add((pt.kernel_form(), elide))
            rays, dropped = pt.read_ray_log()
            assert dropped == 0 and bits_equal(img, g["epoch"]), (mode, elide)
            assert len(rays) == len(order), (mode, elide, len(rays), len(order))
            assert bits_equal(rays["point"], g["point"][order]) and bits_equal(rays["dir"], g["dir"][order]), (mode, elide)
            assert np.array_equal(rays["pixel"], g["pixel"][order]) and np.array_equal(rays["sample"], g["sample"][order])
            assert np.array_equal(rays["bounce"], g["bounce"][order]) and (rays["t"] == 5.0).all()
            again, _ = pt.read_ray_log()
            assert len(again) == 0                                         # a read empties the ring
    assert len(forms) >= 4, forms
    # a ring that is too small drops the surplus and says so; a switched-off log records nothing
    pt.set_kernel(0); pt.set_elision(False); pt.set_ray_log(5)
    pt.render_epoch(seed, base, spp)
    rays, dropped = pt.read_ray_log()
    assert len(rays) == 5 and dropped == len(order) - 5
    pt.set_ray_log(0)
    pt.render_epoch(seed, base, spp)
    assert len(pt.read_ray_log()[0]) == 0
    pt.close()


def test_ray_log_rate_and_group(srt):
    """log_ray's rate over a larger epoch: one call per 2000 shading points of a continuous BSDF (binomial, 5 sigma), identical
    from a group of three logical ranks (tiles on different members, merged in log order)."""
    scene = pt_scene("cbox_lambertian")
    w, h, spp = 256, 192, 32
    pt = make_pt(srt, scene, w, h, 8, True)
    pt.set_ray_log(1 << 16)
    pt.render_epoch(11, 0, spp)
    rays, dropped = pt.read_ray_log()
    rays_total, _ = pt.ray_count(True)
    # every continuous bounce issues three scene.hit calls (two direct, one indirect) and flips the coin once; camera rays: one each
    shading = (rays_total - w * h * spp) / 3.0
    expect = shading * 0.0005
    assert dropped == 0 and abs(len(rays) - expect) < 5.0 * np.sqrt(expect) + 1, (len(rays), expect)
    pt.close()
    grp = srt.PathtracerGroup([0, 0, 0])
    grp.set_params(w, h, 1, 8, True)
    grp.build_scene(scene)
    grp.set_camera(scene["camera"])
    grp.set_ray_log(1 << 16)
    grp.render_epoch(11, 0, spp)
    grays, gdropped = grp.read_ray_log(0)
    assert gdropped == 0 and len(grays) == len(rays)
    for f in ("point", "dir", "pixel", "sample", "bounce"):
        assert np.array_equal(grays[f].view(np.uint32), rays[f].view(np.uint32)), f
    grp.close()


@pytest.mark.parametrize("scene_name,size,spp", [("cbox", 1024, 2048), ("cbox_blob131072_glass", 1024, 256)])
def test_cancel_ends_an_epoch_in_flight(srt, scene_name, size, spp):
    """Pathtracer::cancel (rays/pathtracer.cpp:224,282-290): srt_pt_cancel from another thread ends a
    2048-spp epoch of BASELINE configs[3] - about two seconds of kernels - within a few milliseconds; the call returns
    SRT_CANCELLED, nothing further is enqueued until srt_pt_clear_cancel, and the next epoch is bit-identical to one rendered by a
    context that was never cancelled.  The same for the streamed forms (BASELINE configs[4]'s stand-in)."""
    import threading
    import time

    scene = pt_scene(scene_name)
    pt = make_pt(srt, scene, size, size, 8, True)
    pt.render_epoch(1, 0, 1)                                   # buffers, code objects
    t0 = time.perf_counter()
    pt.render_epoch(1, 0, 8)
    per_sample = (time.perf_counter() - t0) / 8
    assert per_sample * spp > 0.25, "the epoch is too short to be cancelled half way"
    bar_ms = 5.0 if scene_name == "cbox" else 25.0
    latencies = []
    for attempt in range(3):                                   # (the bar is the device's; a late wake-up of this process's threads gets another try)
        result = {}

        def worker():
            try:
                pt.render_epoch(1, 0, spp)
                result["status"] = "finished"
            except srt.SrtCancelled:
                result["status"] = "cancelled"
            result["t_return"] = time.perf_counter()

        th = threading.Thread(target=worker)
        t_start = time.perf_counter()
        th.start()
        time.sleep(min(0.12, 0.3 * per_sample * spp))
        t_cancel = time.perf_counter()
        pt.cancel_device()
        th.join()
        assert result["status"] == "cancelled"
        latency_ms = (result["t_return"] - t_cancel) * 1e3
        latencies.append(latency_ms)
        print(f"{scene_name}: cancelled {1e3 * (t_cancel - t_start):.0f} ms into a ~{1e3 * per_sample * spp:.0f} ms epoch, returned after {latency_ms:.2f} ms")
        if latency_ms < bar_ms:
            break
        assert pt.cancel_requested()
        pt.clear_cancel()
    assert min(latencies) < bar_ms, latencies
    assert pt.cancel_requested()
    with pytest.raises(srt.SrtCancelled):
        pt.render_epoch(1, 0, 1)                               # refused while the flag is up
    pt.clear_cancel()
    assert not pt.cancel_requested()
    got = pt.render_epoch(5, 3, 2)
    fresh = make_pt(srt, scene, size, size, 8, True)
    want = fresh.render_epoch(5, 3, 2)
    assert bits_equal(got, want)
    pt.close(); fresh.close()


@pytest.mark.parametrize("w,h,slots", [(40, 24, 256), (70, 45, 512), (33, 33, 256)])
def test_streamed_forms_with_padding_pixels_and_a_small_population(srt, w, h, slots):
    """Images whose sides are no multiples of the 32 x 32 tiles hand out PADDING units (pixels of an edge tile outside the image): a path
    slot that draws one has nothing to render and must draw again in the next generation - with the alive-slot list of round 4 it
    has to stay on that list although it is idle (found by tools/fuzz_pt.py: with a small population the launch ran out of slots and
    ended with unfinished units).  Both streamed forms, populations far smaller than the unit count, against the oracle."""
    scene = pt_scene("cbox_blob512_glass")
    spp = 7
    want = H.OraclePT(scene, w, h, 6, True).epoch(9, 2, spp)
    pt = make_pt(srt, scene, w, h, 6, True)
    pt.set_stream_slots(slots)
    for mode in (6, 7):
        for elide in (False, True):
            pt.set_kernel(mode)
            pt.set_elision(elide)
            assert pt.kernel_form() in (3, 4)
            assert bits_equal(pt.render_epoch(9, 2, spp), want), (mode, elide)
    pt.close()
