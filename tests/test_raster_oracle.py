"""CPU: pin oracle/raster_oracle.c against the golden vectors produced by the reference's own code
(tests/golden/make_raster_golden.py) and, in the authoring container, against the reference build."""
import ctypes
import glob
import os

import numpy as np
import pytest

import _harness as H
from _cases import adversarial_stream, random_triangles

GOLDENS = sorted(glob.glob(os.path.join(H.GOLDEN, "raster_*.npz")))


def test_goldens_present():
    names = [os.path.basename(g) for g in GOLDENS]
    assert "raster_cfg1_triangle1_256_ss1.npz" in names  # BASELINE.json configs[0]
    assert "raster_cfg2_test3_1024_ss4.npz" in names     # BASELINE.json configs[1]
    assert len(names) >= 16


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(g)[7:-4] for g in GOLDENS])
def test_oracle_matches_reference_golden(path):
    g = np.load(path)
    w, h, sr = (int(x) for x in g["meta"])
    tex = H.Textures.from_npz(g)
    rgba, ss, counts = H.oracle_raster_frame(g["prims"], w, h, sr, want_samples=True, textures=tex)
    assert np.array_equal(rgba, g["rgba"]), "RGBA8 differs from the reference"
    assert H.sha(ss) == str(g["ss_sha256"]), "float supersample buffer differs from the reference"
    assert counts[1] <= counts[0] and counts[2] <= counts[1]
    # the mip chains in the fixture are the reference's (Sampler2DImp::generate_mips); the oracle's restatement
    # must rebuild every level from level 0
    for t in range(len(tex)):
        chain = tex.texture(t)
        mine = H.oracle_generate_mips(chain[0][2])
        assert len(mine) == len(chain)
        for k, ((w1, h1, a), (w2, h2, b)) in enumerate(zip(mine, chain)):
            assert (w1, h1) == (w2, h2)
            # a level built from a 1-texel-wide or 1-texel-high level reads one column / row past that level in the
            # reference (texture.cpp:104, undefined; zeros in the oracle): only the defined levels are compared
            if k == 0 or (chain[k - 1][0] >= 2 and chain[k - 1][1] >= 2):
                assert np.array_equal(a, b), f"mip level {k} differs from the reference"


def test_cfg_counts_match_survey():
    """cfg2 = 50 000 979 sample tests, ~3.87 M fragments; cfg1 = 11 310 tests."""
    g = np.load(os.path.join(H.GOLDEN, "raster_cfg1_triangle1_256_ss1.npz"))
    _, _, c = H.oracle_raster_frame(g["prims"], 256, 256, 1)
    assert int(c[0]) == 11310
    g = np.load(os.path.join(H.GOLDEN, "raster_cfg2_test3_1024_ss4.npz"))
    _, _, c = H.oracle_raster_frame(g["prims"], 1024, 1024, 4)
    assert int(c[0]) == 50000979
    assert abs(int(c[2]) - 3874153) <= 2


def test_adversarial_generator_is_stable():
    """The committed adversarial fixtures are regenerable: same seed -> same stream."""
    for sr in (1, 2, 3, 4, 5):
        g = np.load(os.path.join(H.GOLDEN, f"raster_adversarial_ss{sr}.npz"))
        p = adversarial_stream(seed=1234 + sr, w=97, h=61)
        assert p.tobytes() == np.ascontiguousarray(g["prims"]).tobytes()


def test_empty_stream_is_white():
    rgba, ss, counts = H.oracle_raster_frame(np.zeros(0, H.PRIM_DTYPE), 5, 3, 2, want_samples=True)
    assert (rgba == 255).all() and (ss == 255.0).all() and not counts.any()


def test_opaque_cover_hides_history():
    """Painter's order: an opaque target-covering triangle erases whatever was drawn before it."""
    w, h, sr = 40, 24, 3
    under = random_triangles(7, 50, w, h, 30)
    cover = random_triangles(8, 1, w, h, 1)
    cover["v"] = np.array([-100, -100, 500, -100, -100, 500], np.float32).view(np.float64)
    cover["rgba"] = [0.25, 0.5, 0.75, 1.0]
    a, _, _ = H.oracle_raster_frame(np.concatenate([under, cover]), w, h, sr)
    b, _, _ = H.oracle_raster_frame(cover, w, h, sr)
    assert np.array_equal(a, b)
    assert (b[..., :3] == [63, 127, 191]).all() and (b[..., 3] == 255).all()


@pytest.mark.parametrize("sr", [1, 2, 3, 4, 7])
def test_oracle_matches_reference_build_random(sr):
    """Seeded random + adversarial streams against the reference build's frames of them (tests/golden/refbuild_raster_random.npz,
    make_refbuild_vectors.py); where oracle/_ref is built, against the reference itself as well."""
    g = np.load(os.path.join(H.GOLDEN, "refbuild_raster_random.npz"))
    w, h = (int(x) for x in g["meta"])
    for seed in range(3):
        prims = g[f"prims_sr{sr}_s{seed}"]
        assert np.array_equal(prims, np.concatenate([random_triangles(100 * sr + seed, 120, w, h, 50), adversarial_stream(seed, w, h)]))
        o_rgba, o_ss, _ = H.oracle_raster_frame(prims, w, h, sr, want_samples=True)
        assert np.array_equal(g[f"rgba_sr{sr}_s{seed}"], o_rgba)
        assert H.sha(o_ss) == str(g[f"ss_sha256_sr{sr}_s{seed}"])
        if H.ref_raster() is not None:
            r_rgba, r_ss = H.ref_raster_prims(prims, w, h, sr, want_samples=True)
            assert np.array_equal(r_rgba, o_rgba)
            assert np.array_equal(r_ss.view(np.uint32), o_ss.view(np.uint32))


def _svg_files():
    """Every SVG of the reference when its tree is here, else the three committed under tests/golden/svg."""
    import glob
    ref = sorted(glob.glob("/root/reference/Assignments/DrawSVG/svg/*/*.svg"))
    return ref or sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "svg", "*.svg")))


@pytest.mark.ref
@pytest.mark.skipif(H.ref_raster() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_host_walk_shortcuts_keep_the_stream_byte_identical():
    """host/svg_stream.cpp transforms a polygon's points inline and once per point; with set_reference_transforms(true) every
    corner goes through the reference's SVGRenderer::transform instead.  The two streams must not differ in one byte, in the
    initial framing and under a skewed projective matrix, cold and on warm triangulation caches."""
    lib = H.ref_raster()
    lib.ref_raster_svg_stream_ab.restype = ctypes.c_long
    files = _svg_files()
    assert files
    for path in files:
        for variant in (0, 1):
            for (w, h, sr) in ((256, 256, 1), (1024, 768, 4)):
                assert lib.ref_raster_svg_stream_ab(path.encode(), w, h, sr, variant) == 0, (path, variant, w, h, sr)
