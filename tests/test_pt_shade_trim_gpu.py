"""GPU: the shade section of the wave kernel where it no longer does what the result does not need - the point transforms of
surface_of, light_sample and light_pdf skip the divide by a w that is 1 in every active lane (mat_point_uniform, csrc/pt_device.h;
the W1 forms of the three functions, csrc/pt_trace.h).  Small images of the wave forms - kernel modes 2, 3 (the same with section
stamps) and, with a mesh that has a real BVH<Triangle> in the glass sphere's place, 7 (the streamed sweeps: the resolve kernel
shades) - against the lane-per-sample form (mode 4), which keeps the plain transforms: equal bits, equal ray counts.

  cornell            glass and mirror lanes beside Lambertian ones; every matrix affine
  light_projective   w = 2 on the area light: light_sample's and light_pdf's ballots send the wave down the dividing path
  sphere_projective  a perspective row on the mirror sphere: surface_of's ballots see w != 1 in some lanes of a wave and 1 in others
  translated_light   the all-Lambertian box: its only light is posed by a pure translation, every w is exactly 1
  two_glass          two glass objects of different ior: the discrete lanes, which take none of the light transforms, beside the rest"""
import numpy as np
import pytest

from _cases import pt_scene
from _scale_cases import projective

pytestmark = pytest.mark.gpu

SPHERES, BLOB = "cbox", "cbox_blob512_glass"       # object 6: the glass sphere / a 512-triangle glass mesh (mode 7 takes it)


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def cornell(base):
    return pt_scene(base)


def light_projective(base):
    return projective(pt_scene(base), (7,), ((0.0, 0.0, 0.0, 2.0),))


def sphere_projective(base):
    return projective(pt_scene(base), (5,), ((0.0, 0.25, 0.0, 1.0),))


def translated_light(base):
    s = pt_scene("cbox_lambertian")
    if base == BLOB:                                # the blob in the second sphere's place, white Lambertian like the sphere it replaces
        s["objects"] = list(s["objects"])
        s["objects"][6] = dict(pt_scene(BLOB)["objects"][6], material=6)
    T = np.asarray(s["objects"][7]["T"], np.float32).reshape(4, 4).T
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=np.float32)) and np.array_equal(T[3], [0, 0, 0, 1]) and T[:3, 3].any()
    assert sum(bool(o.get("is_light")) for o in s["objects"]) == 1
    return s


def two_glass(base):
    s = pt_scene(base)
    mats = list(s["materials"])
    assert int(mats[6]["type"]) == 2 and float(mats[6]["ior"]) == 1.5
    mats[5] = dict(mats[6], ior=1.33)               # the mirror sphere becomes a second glass object
    s["materials"] = mats
    return s


SCENES = [cornell, light_projective, sphere_projective, translated_light, two_glass]
CASES = [(make, SPHERES, (2, 3)) for make in SCENES] + [(make, BLOB, (7,)) for make in SCENES]


@pytest.mark.parametrize("make,base,modes", CASES, ids=[f"{c[0].__name__}-{'spheres' if c[1] == SPHERES else 'blob'}" for c in CASES])
def test_wave_forms_equal_lane_per_sample(srt, make, base, modes):
    scene = make(base)
    p = srt.Pathtracer(0)
    p.set_params(64, 64, 1, 8, True)
    p.build_scene(scene)
    p.set_camera(scene["camera"])
    try:
        p.set_kernel(4)
        p.ray_count(reset=True)
        want = p.render_epoch(0, 0, 8)
        want_rays = p.ray_count(reset=True)[0]
        assert want_rays > 64 * 64 * 8 and np.isfinite(want).any() and (want > 0).any()
        for mode in modes:
            p.set_kernel(mode)
            got = p.render_epoch(0, 0, 8)
            rays = p.ray_count(reset=True)[0]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{make.__name__}: kernel mode {mode} differs from mode 4 in {int((~same).sum())} values"
            assert rays == want_rays, f"{make.__name__}: kernel mode {mode} counted {rays} rays, mode 4 {want_rays}"
    finally:
        p.close()
