"""GPU: the wave kernel's batch Triangle::hit (tri_hitN, csrc/pt_device.h: inside / outside verdict from the numerators and det,
only t divided) returns, for every lane, the {hit, t, dist} of the plain per-ray tri_hit - bit for bit, NaN == NaN as in the other
parity tests - on random sets in and around the Cornell box and on sets built around every comparison of the verdict."""
import numpy as np
import pytest

from _tri_verdict_cases import constructed_sets, random_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    import srt_amd

    p = srt_amd.Pathtracer(0)
    yield p
    p.close()


def _same(got, want):
    for key in ("hit", "t", "dist"):
        a, b = got[key], want[key]
        if key == "hit":
            ok = a == b
        else:
            ok = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        bad = np.argwhere(~ok)
        assert bad.size == 0, (key, len(bad), bad[:5], a[~ok][:5], b[~ok][:5])


def test_random_sets(pt):
    tri, org, dirs, bounds = random_sets(31, 1 << 20)
    batch, plain, ambiguous = pt.math_tri_verdict(tri, org, dirs, bounds)
    print("random sets: hits", int(plain["hit"].sum()), "of", plain["hit"].size, "- waves through the ambiguous branch:", ambiguous)
    assert 0.1 < plain["hit"].mean() < 0.6           # the sets do exercise both verdicts
    _same(batch, plain)


def test_constructed_sets(pt):
    tri, org, dirs, bounds = constructed_sets(32)
    batch, plain, ambiguous = pt.math_tri_verdict(tri, org, dirs, bounds)
    print("constructed sets:", len(tri), "hits", int(plain["hit"].sum()), "- waves through the ambiguous branch:", ambiguous)
    _same(batch, plain)
    assert ambiguous > 0, "no wave took the ambiguous branch: the fallback was never run"
    assert plain["hit"].any() and not plain["hit"].all()
