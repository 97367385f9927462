"""GPU: the leaf section's point transform (mat_point_affine, csrc/pt_device.h) against the plain mat_point through
srt_pt_math_point_affine, bit for bit, on 256 waves of 64 lanes with one matrix each (tests/_point_affine_cases.py): affine matrices
(with -0 in the bottom row) - the wave leaves w out; w = 2 and a perspective row - it does not; one lane with an inf or NaN
component, with a first row that overflows, or with 0 * inf in it, in an otherwise finite wave - the whole wave computes w.  Which
waves left w out is asserted against the CPU build's per-lane verdicts, and the device's values against the host's.

Then renders, 64 x 64, 4 spp, depth 8, through the leaf section's transforms and the top-down step (topdown_step, csrc/pt_trace.h):
the wave forms (kernel modes 2, 3 and - with a mesh that has a real BVH<Triangle> - 2 and 7) against the lane-per-sample form, equal
bits and equal ray counts, on the box, the all-Lambertian box, the box with a sphere of infinite radius (non-finite object-space
points) and the box with w = 2 on a wall and a perspective row on the light (rows that are not affine, next to rows that are)."""
import numpy as np
import pytest

from _cases import pt_scene
from _point_affine_cases import KINDS, cases
from _scale_cases import projective
from test_pt_point_affine_host import run_host, same_bits

pytestmark = pytest.mark.gpu


def test_point_affine_equals_mat_point_on_the_device():
    import srt_amd

    c = cases(82, 256)
    pt = srt_amd.Pathtracer(0)
    try:
        a, b, skipped = pt.math_point_affine(c["mats"], c["points"])
    finally:
        pt.close()
    assert same_bits(a, b).all(), np.argwhere(~same_bits(a, b))[:5]
    ha, hb, hskipped, _ = run_host(c)
    assert same_bits(b, hb).all() and same_bits(a, ha).all()
    want = hskipped.reshape(-1, 64).all(axis=1)          # a wave leaves w out iff every lane of it may
    assert np.array_equal(skipped, want), (np.argwhere(skipped != want).ravel()[:8], [KINDS[k] for k in c["kind"][skipped != want][:8]])
    assert np.array_equal(skipped, c["skips"])
    print("waves:", len(skipped), "w left out in", int(skipped.sum()))


SPHERES, BLOB = "cbox", "cbox_blob512_glass"       # object 6: the glass sphere / a 512-triangle glass mesh (modes 2 and 7 walk it)


def cornell(base):
    return pt_scene(base)


def lambertian(base):
    s = pt_scene("cbox_lambertian")
    if base == BLOB:                                    # the mesh in the second sphere's place, white Lambertian like that sphere
        s["objects"] = list(s["objects"])
        s["objects"][6] = dict(pt_scene(BLOB)["objects"][6], material=6)
    return s


def infinite_sphere(base):
    s = pt_scene(base)
    s["objects"] = list(s["objects"])
    assert s["objects"][5]["kind"] == "sphere"
    s["objects"][5] = dict(s["objects"][5], radius=np.inf)
    return s


def projective_wall_and_light(base):
    return projective(pt_scene(base), (4, 7), ((0.0, 0.0, 0.0, 2.0), (0.0, 0.25, 0.0, 1.0)))


SCENES = [cornell, lambertian, infinite_sphere, projective_wall_and_light]
CASES = [(make, SPHERES, (2, 3)) for make in SCENES] + [(make, BLOB, (2, 7)) for make in SCENES]


@pytest.mark.parametrize("make,base,modes", CASES, ids=[f"{c[0].__name__}-{'spheres' if c[1] == SPHERES else 'blob'}" for c in CASES])
def test_wave_forms_equal_lane_per_sample(make, base, modes):
    import srt_amd

    scene = make(base)
    p = srt_amd.Pathtracer(0)
    p.set_params(64, 64, 4, 8, True)
    p.build_scene(scene)
    p.set_camera(scene["camera"])
    try:
        p.set_kernel(4)
        p.ray_count(reset=True)
        want = p.render_epoch(0, 0, 4)
        want_rays = p.ray_count(reset=True)[0]
        assert want_rays > 64 * 64 * 4 and np.isfinite(want).any()
        for mode in modes:
            p.set_kernel(mode)
            got = p.render_epoch(0, 0, 4)
            rays = p.ray_count(reset=True)[0]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{make.__name__}: kernel mode {mode} differs from mode 4 in {int((~same).sum())} values"
            assert rays == want_rays, f"{make.__name__}: kernel mode {mode} counted {rays} rays, mode 4 {want_rays}"
    finally:
        p.close()
