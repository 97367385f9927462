"""GPU: the persistent wave forms take their camera rays from a per-launch table (pt_camera_kernel, csrc/pt_wave.h): one lane per
(pixel slot, sample of the launch) computes Rng::key, the two jitter draws and camera_ray at full wave width in front of the launch,
and the loop's refill and shade load the direction and the RNG state where they used to compute them.  The lane-per-sample form
(kernel mode 4) keeps the inline arithmetic, so every render here is held to it: equal bits (NaN = NaN), equal ray counts.
(Of the forms below the stamped and the two-ray build of the Cornell form - mode 3, and mode 2 with elision on `cbox` - keep the
inline arithmetic too, for the sake of their scratch; they stay in the cases, as the issue lists them, and so stay held to mode 4.)

The shapes are the smallest at which the table's indexing can go wrong: an image that is no multiple of the 32 x 32 tile or the
8 x 8 block (padding pixels), launches shorter than a burst and on both sides of the rule for single-sample units, several launches
per epoch with a non-zero sample base, every persistent form, tiled shards, settings that change between renders of one context,
and two streams with a table each."""
import numpy as np
import pytest

from _cases import pt_scene

pytestmark = pytest.mark.gpu

SEED = 7
W, H = 37, 29                                       # two tiles by one, both with padding pixels; 29 is no multiple of 8 either


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def context(srt, scene, w, h, mode, camera=None):
    p = srt.Pathtracer(0)
    p.set_params(w, h, 1, 8, True)
    p.build_scene(scene)
    p.set_camera(camera or scene["camera"])
    p.set_kernel(mode)
    return p


def render(p, seed, base, spp):
    p.ray_count(reset=True)
    img = p.render_epoch(seed, base, spp)
    return img, p.ray_count(reset=True)[0]


_REFERENCE = {}


def reference(srt, name, w, h, seed, base, spp):
    """The lane-per-sample render (mode 4) of a scene of _cases.pt_scene: computed once, shared, never written to."""
    key = (name, w, h, seed, base, spp)
    if key not in _REFERENCE:
        p = context(srt, pt_scene(name), w, h, 4)
        try:
            img, rays = render(p, seed, base, spp)
        finally:
            p.close()
        assert rays >= w * h * spp and (img > 0).any()
        img.setflags(write=False)
        _REFERENCE[key] = (img, rays)
    return _REFERENCE[key]


def check(got, rays, want, want_rays, what):
    same = same_bits(got, want)
    assert same.all(), f"{what}: differs from the lane-per-sample form in {int((~same).sum())} values"
    assert rays == want_rays, f"{what}: counted {rays} rays, the lane-per-sample form {want_rays}"


# 1, 2: shorter than a burst of either form; 3, 4, 7: remainders; 8 and 12 are where `singles` sets in for two- and three-ray
# batches (n >= 4 * burst), so 7 / 12 / 13 stand on both sides of both; 64 is a full launch
@pytest.mark.parametrize("spp", [1, 2, 3, 4, 7, 12, 13, 64])
def test_padding_pixels_and_unit_arithmetic(srt, spp):
    want, want_rays = reference(srt, "cbox", W, H, SEED, 0, spp)
    p = context(srt, pt_scene("cbox"), W, H, 2)
    try:
        for mode, two in ((2, False), (3, False), (2, True)):
            p.set_kernel(mode)
            p.set_elision(two)
            got, rays = render(p, SEED, 0, spp)
            check(got, rays, want, want_rays, f"{spp} spp, mode {mode}{', two-ray batches' if two else ''}")
    finally:
        p.close()


@pytest.mark.parametrize("base,spp", [(5, 9), (0, 130)], ids=["base5", "launches_64_64_2"])
def test_sample_base_and_several_launches(srt, base, spp):
    want, want_rays = reference(srt, "cbox", W, H, SEED, base, spp)
    p = context(srt, pt_scene("cbox"), W, H, 2)
    try:
        got, rays = render(p, SEED, base, spp)
        check(got, rays, want, want_rays, f"samples [{base}, {base + spp})")
    finally:
        p.close()


# the sweeps with a per-lane BVH<Triangle> walk, the flattened walk, the delta-light build, and two scenes whose camera rays leave
# into an environment light (the image map is evaluated from the sample's camera direction when the sample is resolved)
@pytest.mark.parametrize("name,mode,two", [("cbox_blob512_glass", 2, False), ("cbox_blob512_glass", 2, True), ("cbox", 5, False),
                                           ("cbox_deltalights", 2, False), ("cbox_envmap", 2, False), ("cbox_envonly", 2, False)])
def test_other_persistent_forms(srt, name, mode, two):
    want, want_rays = reference(srt, name, 64, 64, SEED, 0, 8)
    p = context(srt, pt_scene(name), 64, 64, mode)
    try:
        p.set_elision(two)                         # (the two-ray build of the sweeps with a per-lane walk reads the table)
        got, rays = render(p, SEED, 0, 8)
        check(got, rays, want, want_rays, f"{name}, mode {mode}{', two-ray batches' if two else ''}")
    finally:
        p.close()


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_tiled_shards(srt, rank):
    w, h, spp = 70, 45, 5                          # 3 x 2 tiles of 32 x 32 dealt to three ranks
    want, _ = reference(srt, "cbox", w, h, SEED, 0, spp)
    p = context(srt, pt_scene("cbox"), w, h, 2)
    try:
        p.set_tiling(32, 32, rank, 3)
        img = np.full((h, w, 3), -1.0, np.float32)
        p.render_epoch(SEED, 0, spp, out=img)
    finally:
        p.close()
    yy, xx = np.mgrid[0:h, 0:w]
    mine = ((yy // 32) * 3 + xx // 32) % 3 == rank
    assert mine.any() and not mine.all()
    assert same_bits(img, want)[mine].all(), f"rank {rank}: its tiles differ from the un-tiled render"
    assert (img[~mine] == -1.0).all(), f"rank {rank} wrote pixels of another rank"


def moved_camera(scene):
    cam = dict(scene["camera"])
    iv = np.array(cam["iview"], np.float32).reshape(4, 4).copy()
    iv[3, :3] += np.float32([0.125, -0.0625, 0.25])  # (rows are columns of the matrix: the last row is the eye)
    cam["iview"] = iv.reshape(-1)
    return cam


def test_nothing_stale_between_renders(srt):
    """One context, mode 2: a render after each change of camera, size, tiling and seed equals a fresh context's."""
    scene = pt_scene("cbox")
    cam2 = moved_camera(scene)

    def fresh(w, h, camera, seed, tiling=None):
        q = context(srt, scene, w, h, 2, camera)
        try:
            if tiling:
                q.set_tiling(*tiling)
            out = np.full((h, w, 3), -1.0, np.float32)
            return q.render_epoch(seed, 0, 4, out=out)
        finally:
            q.close()

    p = context(srt, scene, W, H, 2)
    try:
        first = p.render_epoch(SEED, 0, 4)
        assert same_bits(first, fresh(W, H, scene["camera"], SEED)).all()
        p.set_camera(cam2)
        moved = p.render_epoch(SEED, 0, 4)
        assert same_bits(moved, fresh(W, H, cam2, SEED)).all(), "after set_camera"
        assert not same_bits(moved, first).all(), "the second camera sees the same image: the case tests nothing"
        p.set_params(50, 41, 1, 8, True)
        assert same_bits(p.render_epoch(SEED, 0, 4), fresh(50, 41, cam2, SEED)).all(), "after set_params"
        p.set_tiling(16, 8, 1, 2)
        out = np.full((41, 50, 3), -1.0, np.float32)
        p.render_epoch(SEED, 0, 4, out=out)
        assert same_bits(out, fresh(50, 41, cam2, SEED, (16, 8, 1, 2))).all(), "after set_tiling"
        out2 = np.full((41, 50, 3), -1.0, np.float32)
        p.render_epoch(SEED + 1, 0, 4, out=out2)
        assert same_bits(out2, fresh(50, 41, cam2, SEED + 1, (16, 8, 1, 2))).all(), "after a seed change"
        assert not same_bits(out2, out).all()
    finally:
        p.close()


def test_two_streams_have_a_table_each(srt):
    """Epochs with different sample bases alternately on two streams, as bench.py's step enqueues them: the same tiles as on one."""
    import torch

    p = context(srt, pt_scene("cbox"), W, H, 2)
    try:
        _, per_rank, fpt = p.tile_info()
        one = torch.cuda.current_stream()
        want = [torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda") for _ in range(4)]
        got = [torch.zeros(per_rank * fpt, dtype=torch.float32, device="cuda") for _ in range(4)]
        for i in range(4):
            p.render_epoch_device(one.cuda_stream, SEED, i * 6, 6, want[i].data_ptr())
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for i in range(4):
            p.render_epoch_device(streams[i % 2].cuda_stream, SEED, i * 6, 6, got[i].data_ptr())
        torch.cuda.synchronize()
        for i in range(4):
            assert torch.equal(want[i].view(torch.int32), got[i].view(torch.int32)), f"epoch {i}"
        assert not torch.equal(want[0], want[1])
    finally:
        p.close()
