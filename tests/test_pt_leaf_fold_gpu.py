"""GPU: the leaf fold of the wave kernel's mesh branch (leaf_foldN, csrc/pt_device.h: a candidate pass over the leaf's triangles,
then one quotient and one root per ray; a wave with a flagged lane folds the leaf with the plain tri_hit) returns, for every
lane, the {hit, triangle, t, dist} of the plain ordered fold ret = Trace::min(ret, Triangle::hit) - equal bits - through
srt_pt_math_leaf_fold, on waves of 64 lanes with one leaf each (tests/_leaf_fold_cases.py):

  * group F - coplanar leaves of 1, 2, 3, 4 and 12 triangles, targets at barycentric distance >= 2^-8 from every edge, lanes that
    miss, candidates behind the origin and cut by either bound, origins on the plane: every wave reports the fast path;
  * group M - exact dyadic points on the shared diagonal and on shared vertices, stacked pairs in different planes (nearer first,
    second, equal distances), tetrahedra: every wave reports the fallback;
  * group A - sets scaled by 2^+-41, det == 0, NaN / inf operands;
  * 2^16 random lanes.

Which waves fall back is predicted on the CPU (tests/test_pt_leaf_fold_host.py: the same bookkeeping compiled for the host) and
asserted wave by wave.  Then a render: a Cornell box whose sphere is a tetrahedron (a closed mesh in one leaf: two candidates are
the rule), every wave form against the lane-per-sample form."""
import numpy as np
import pytest

from _cases import pt_scene
from _leaf_fold_cases import group_a, group_f, group_m, random_sets
from test_pt_leaf_fold_host import run_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import srt_amd

    p = srt_amd.Pathtracer(0)
    yield p
    p.close()


def _run(pt, s):
    leaf, plain, fell = pt.math_leaf_fold(s["tris"], s["ntri"], s["org"], s["dirs"], s["bounds"])
    for key in ("hit", "tri", "t", "dist"):
        a, b = leaf[key], plain[key]
        ok = (a == b) if key in ("hit", "tri") else (a.view(np.uint32) == b.view(np.uint32))
        bad = np.argwhere(~ok)
        assert bad.size == 0, (key, len(bad), bad[:5], a[~ok][:5], b[~ok][:5])
    bad_lane, out = run_host(s)
    # the plain fold on the device is the plain fold on the host
    assert np.array_equal(plain["hit"], out[..., 5] != 0) and np.array_equal(plain["tri"], out[..., 6])
    for key, col in (("t", 7), ("dist", 8)):             # (a NaN's sign and payload are the machine's: x86 and the device differ)
        h = out[..., col].view(np.float32)
        assert ((plain[key].view(np.uint32) == out[..., col]) | (np.isnan(plain[key]) & np.isnan(h))).all(), key
    want = bad_lane.any(axis=1)
    assert np.array_equal(fell, want), ("waves that fell back", np.argwhere(fell != want).ravel()[:8])
    return plain, fell


def test_group_f_takes_the_fast_path(pt):
    plain, fell = _run(pt, group_f(51))
    print("group F:", len(fell), "waves, hits", int(plain["hit"].sum()), "of", plain["hit"].size)
    assert not fell.any(), np.argwhere(fell).ravel()
    assert plain["hit"].any() and not plain["hit"].all()


def test_group_m_falls_back(pt):
    plain, fell = _run(pt, group_m(52))
    print("group M:", len(fell), "waves, hits", int(plain["hit"].sum()), "of", plain["hit"].size)
    assert fell.all(), np.argwhere(~fell).ravel()
    assert plain["hit"].any()


def test_group_a(pt):
    plain, fell = _run(pt, group_a(53))
    print("group A:", len(fell), "waves,", int(fell.sum()), "fell back; NaN distances", int(np.isnan(plain["dist"]).sum()))
    assert fell.any()


def test_random_sets(pt):
    plain, fell = _run(pt, random_sets(54, 1024))
    print("random:", len(fell), "waves,", int(fell.sum()), "fell back; hits", int(plain["hit"].sum()), "of", plain["hit"].size)
    assert fell.any() and not fell.all()
    assert 0.05 < plain["hit"].mean() < 0.6


_TETRA_V = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]], np.float32)
_TETRA_F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def _tetra_pose(x, y, z, size=0.15, turn=0.4):
    c, s = np.float32(np.cos(turn)) * np.float32(size), np.float32(np.sin(turn)) * np.float32(size)
    return [c, 0, s, x, 0, size, 0, y, -s, 0, c, z, 0, 0, 0, 1]


def tetrahedron_box():
    """The Cornell box with a glass tetrahedron in the place of the glass sphere: four triangles, one leaf, posed by a matrix."""
    from soft_rendering_toolsets_amd import scenes

    return scenes.cornell_with_asset(_TETRA_V, _TETRA_F, _tetra_pose(0.2, 0.2, 0.1), "glass", "tetra")


def tetrahedron_and_blob():
    """The box with the 512-triangle glass mesh (a real BVH<Triangle>: the lazy and the streamed sweeps) and a mirror tetrahedron
    in the place of the mirror sphere."""
    from soft_rendering_toolsets_amd import scenes

    s = pt_scene("cbox_blob512_glass")
    t = scenes.cornell_with_asset(_TETRA_V, _TETRA_F, _tetra_pose(-0.25, 0.2, -0.1), "mirror", "tetra")["objects"][6]
    s["objects"][5] = t
    return s


RENDER_CASES = [
    # name, scene, use_bvh, wave-form modes (2 the sweeps, 3 their stamped build, 7 the streamed sweeps)
    ("tetrahedron_bvh", tetrahedron_box, True, (2, 3)),
    ("tetrahedron_list", tetrahedron_box, False, (2, 3)),
    ("tetrahedron_and_blob512", tetrahedron_and_blob, True, (2, 7)),
]


@pytest.mark.parametrize("name,make,use_bvh,modes", RENDER_CASES, ids=[c[0] for c in RENDER_CASES])
def test_tetrahedron_box_wave_forms_equal_lane_per_sample(name, make, use_bvh, modes):
    import srt_amd

    scene = make()
    p = srt_amd.Pathtracer(0)
    p.set_params(32, 24, 4, 4, use_bvh)
    p.build_scene(scene)
    p.set_camera(scene["camera"])
    try:
        p.set_kernel(4)
        p.ray_count(reset=True)
        want = p.render_epoch(0, 0, 4)
        want_rays = p.ray_count(reset=True)[0]
        assert want_rays > 0 and np.isfinite(want).any()
        for mode in modes:
            p.set_kernel(mode)
            got = p.render_epoch(0, 0, 4)
            rays = p.ray_count(reset=True)[0]
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), f"{name}: kernel mode {mode} differs from mode 4 in {int((~same).sum())} values"
            assert rays == want_rays, f"{name}: kernel mode {mode} counted {rays} rays, mode 4 {want_rays}"
    finally:
        p.close()
