"""GPU: the end of a path in the wave kernel (csrc/pt_wave.h).  A finished path folds its per-bounce records back from device memory,
deepest level first.  The kernel loads the records of four consecutive levels - one 128-byte line - before it folds any of them and
skips the levels of a group the path never reached; the operations and their order are the lane-per-sample form's (kernel mode 4),
which keeps a path's records in registers.  So every render here is held to mode 4: equal bits (NaN = NaN), equal ray counts.

max_depth is the lever: it bounds `level`, and the depths below cover every residue of a group of four, the group boundaries, one
past them and kMaxPathDepth itself.  The image is 24 x 20 at 7 spp: two bursts and a single-sample unit per pixel, padding pixels in
the edge tiles, and the ceiling light in view, so that camera hits end at level 0 when a parked hit takes over (depth 0 asserts it)."""
import numpy as np
import pytest

import _harness as H
from _cases import pt_scene

pytestmark = pytest.mark.gpu

SEED = 11
W, HEIGHT, SPP = 24, 20, 7
DEPTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16]
FORM_DEPTHS = [3, 8, 16]


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


_CONTEXTS = {}


def context(srt, name, mode, two=False):
    """One context per (scene, mode, two-ray build), kept for the module: max_depth changes between its renders."""
    key = (name, mode, two)
    if key not in _CONTEXTS:
        scene = pt_scene(name)
        p = srt.Pathtracer(0)
        p.set_params(W, HEIGHT, 1, 8, True)
        p.build_scene(scene)
        p.set_camera(scene["camera"])
        p.set_kernel(mode)
        p.set_elision(two)
        _CONTEXTS[key] = p
    return _CONTEXTS[key]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for p in _CONTEXTS.values():
        p.close()
    _CONTEXTS.clear()


def render(p, depth):
    p.set_params(W, HEIGHT, 1, depth, True)
    p.ray_count(reset=True)
    img = p.render_epoch(SEED, 0, SPP)
    return img, p.ray_count(reset=True)[0]


_REFERENCE = {}


def reference(srt, name, depth):
    """The lane-per-sample render (mode 4): computed once per (scene, depth), shared, never written to."""
    key = (name, depth)
    if key not in _REFERENCE:
        img, rays = render(context(srt, name, 4), depth)
        assert rays >= W * HEIGHT * SPP and (img > 0).any()
        img.setflags(write=False)
        _REFERENCE[key] = (img, rays)
    return _REFERENCE[key]


def check(got, rays, want, want_rays, what):
    same = same_bits(got, want)
    print(f"{what}: {int((~same).sum())} values differ, {rays} rays against {want_rays}")
    assert same.all(), f"{what}: differs from the lane-per-sample form in {int((~same).sum())} values"
    assert rays == want_rays, f"{what}: counted {rays} rays, the lane-per-sample form {want_rays}"


@pytest.mark.parametrize("depth", DEPTHS)
def test_depth_sweep(srt, depth):
    want, want_rays = reference(srt, "cbox", depth)
    if depth == 0:
        # nothing is shaded: what the image holds is the emission of camera hits, so the light is in view - and not everywhere
        assert want_rays == W * HEIGHT * SPP
        lit = (want > 0).any(axis=2)
        assert lit.any() and not lit.all()
    for mode in (2, 3):
        got, rays = render(context(srt, "cbox", mode), depth)
        check(got, rays, want, want_rays, f"cbox, max_depth {depth}, mode {mode}")


@pytest.mark.parametrize("depth", [8, 16])
def test_depth_against_the_oracle(srt, depth):
    want = H.OraclePT(pt_scene("cbox"), W, HEIGHT, depth, True).epoch(SEED, 0, SPP)
    got, _ = render(context(srt, "cbox", 2), depth)
    same = same_bits(got, want)
    assert same.all(), f"max_depth {depth}: differs from the oracle in {int((~same).sum())} values"
    assert same_bits(reference(srt, "cbox", depth)[0], want).all()


# no discrete lanes (in the plain and in the stamped build); two-ray batches (the elision build); delta lights (the shadow batches
# hold the C hit back).  Mode 3 takes no scene with delta lights and has no two-ray build, so those two run in mode 2 alone.
@pytest.mark.parametrize("depth", FORM_DEPTHS)
@pytest.mark.parametrize("name,mode,two", [("cbox_lambertian", 2, False), ("cbox_lambertian", 3, False), ("cbox", 2, True),
                                           ("cbox_deltalights", 2, False)],
                         ids=["lambertian", "lambertian_stamped", "two_ray", "deltalights"])
def test_other_sweep_forms(srt, name, mode, two, depth):
    want, want_rays = reference(srt, name, depth)
    p = context(srt, name, mode, two)
    assert p.kernel_form() == 0
    got, rays = render(p, depth)
    check(got, rays, want, want_rays, f"{name}, mode {mode}{', two-ray batches' if two else ''}, max_depth {depth}")


# the flattened walk and the two streamed forms share the terminate code; the streamed ones reload `level` from saved state
@pytest.mark.parametrize("depth", FORM_DEPTHS)
@pytest.mark.parametrize("mode,form", [(5, 2), (6, 3), (7, 4)])
def test_walk_and_streamed_forms(srt, mode, form, depth):
    want, want_rays = reference(srt, "cbox_blob512_glass", depth)
    p = context(srt, "cbox_blob512_glass", mode)
    assert p.kernel_form() == form
    got, rays = render(p, depth)
    check(got, rays, want, want_rays, f"cbox_blob512_glass, mode {mode}, max_depth {depth}")


@pytest.mark.parametrize("name", ["cbox", "cbox_lambertian", "cbox_deltalights", "cbox_blob512_glass"])
def test_deep_levels_are_read_back(srt, name):
    """Paths do go past level 8 at max_depth 16: the runs above fold records of the third and fourth group."""
    assert reference(srt, name, 16)[1] > reference(srt, name, 8)[1]
