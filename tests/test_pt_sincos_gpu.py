"""GPU: srt_sincosf2 as the kernels run it (csrc/pt_device.h, the branch-free form) through the probe srt_pt_math_sincos2, against
the oracle's restatement of glibc's sinf / cosf bit for bit.  One launch.  The arguments are shuffled so that every wave of 64 lanes
holds several quadrants and arguments on both sides of pi / 4 - where the former control flow diverged - followed by waves that are
uniform in the quadrant, below 2^-12, or beyond the range.  The host build of the same functions is swept exhaustively by
tests/test_pt_sincos_host.py."""
import numpy as np
import pytest

import _sincos_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


def _arguments():
    phi, cosine = SC.randoms(12)
    mixed = np.concatenate([SC.thresholds(), SC.quadrant_edges(), phi, cosine, SC.specials()])
    mixed = mixed[np.random.default_rng(13).permutation(len(mixed))]
    mixed = mixed[:len(mixed) // 64 * 64]                 # whole waves; the arguments cut off here are appended below
    rest = np.concatenate([SC.thresholds(), SC.quadrant_edges(), SC.specials()])
    # waves uniform in n: 64 arguments spread over the inside of quadrant n's interval ((n - 1/2) pi/2, (n + 1/2) pi/2)
    t = np.linspace(-0.45, 0.45, 64)
    uniform = [((n + t) * (np.pi / 2)).astype(np.float32) for n in (0, 1, 2, 3, 4, -1, -2, 37, -75)]
    uniform.append(np.linspace(-2.0 ** -13, 2.0 ** -13, 64).astype(np.float32))          # all below 2^-12: {1, y}
    uniform.append(np.linspace(120.0, 1e30, 64).astype(np.float32))                      # all refused: NaN
    uniform.append(np.full(64, np.nan, np.float32))
    return mixed, np.concatenate(uniform), rest


def test_sincos2_equals_the_oracle(srt):
    mixed, uniform, rest = _arguments()
    # the layout is what it claims to be
    w = mixed.reshape(-1, 64)
    top = (w.view(np.uint32) >> 20) & 0x7ff
    in_range = top < 0x42f
    n = np.where(in_range, SC.quadrant(np.where(in_range, w, 0)), 0)
    assert ((n.max(axis=1) - n.min(axis=1)) >= 2).all()                                  # three quadrants or more in every wave
    assert ((top < 0x3f4).any(axis=1) & ((top >= 0x3f4) & in_range).any(axis=1)).all()   # both sides of pi / 4 in every wave
    u = uniform.reshape(-1, 64)
    nu = SC.quadrant(u[:9])
    assert (nu == nu[:, :1]).all() and list(nu[:, 0]) == [0, 1, 2, 3, 4, -1, -2, 37, -75]

    x = np.concatenate([mixed, uniform, rest])
    pt = srt.Pathtracer(0)
    c, s = pt.math_sincos2(x)
    pt.close()
    oc, os_ = SC.oracle_cos_sin(x)
    for name, got, want in (("cos", c, oc), ("sin", s, os_)):
        wrong = np.flatnonzero(~SC.same_bits(got, want))
        assert wrong.size == 0, (name, len(wrong), wrong[:4], x[wrong[:4]], got[wrong[:4]], want[wrong[:4]])
    assert np.isnan(c[np.abs(x) >= 120]).all() and np.isnan(c[np.isnan(x)]).all()
