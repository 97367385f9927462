"""CPU: the leaf section's point transform (mat_point_affine / mat_affine_row, csrc/pt_device.h: for a bottom row of (+-0, +-0, +-0, 1)
and a finite first output row, w is 1 without being computed) compiled for the host (tests/host_emu/point_affine_host.cpp) against
the plain projective product mat_point, bit for bit, one lane at a time: affine matrices (with -0 in the bottom row), w = 2, a
perspective row, points with inf and NaN, points that overflow the first row only, 0 * inf in the first row.  The wave-wide form
(one bad lane sends its whole wave through w) is the GPU test's: tests/test_pt_point_affine_gpu.py."""
import ctypes

import numpy as np

import _harness as H
from _point_affine_cases import KINDS, cases

_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("point_affine_host", ["point_affine_host.cpp"]))
    return _lib


def run_host(c):
    """-> (affine (n, 3), plain (n, 3), skipped (n,) bool, affine_row (n,) bool), every lane a wave of its own."""
    sets = np.ascontiguousarray(np.concatenate([np.repeat(c["mats"], 64, axis=0), c["points"]], axis=1), np.float32)
    out = np.zeros((len(sets), 8), np.uint32)
    assert _host().point_affine_host(H.P(sets), ctypes.c_size_t(len(sets)), H.P(out)) == 0
    f = lambda a: np.ascontiguousarray(a).view(np.float32)
    return f(out[:, 0:3]), f(out[:, 3:6]), out[:, 6] != 0, out[:, 7] != 0


def same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_point_affine_equals_mat_point():
    c = cases(81, 256)
    a, b, skipped, row = run_host(c)
    assert same_bits(a, b).all(), np.argwhere(~same_bits(a, b))[:5]
    lane_kind = np.repeat(c["kind"], 64)
    not_affine = np.isin(lane_kind, [KINDS.index("w2"), KINDS.index("perspective")])
    assert np.array_equal(row, ~not_affine), "which bottom rows count as affine"
    assert not skipped[not_affine].any()
    finite0 = np.isfinite(b[:, 0]) | not_affine          # (w == 1 there: mat_point's x is the first row)
    assert np.array_equal(skipped, row & finite0)
    assert skipped[np.repeat(c["skips"], 64)].all()
    for k in ("one_lane_inf", "one_lane_nan", "row0_overflows", "affine_infinite_entry"):
        lanes = lane_kind == KINDS.index(k)
        assert (~skipped[lanes]).reshape(-1, 64).sum(axis=1).min() >= 1, k
    print("lanes:", len(a), "w left out in", int(skipped.sum()), "; non-finite results", int((~np.isfinite(b)).any(axis=1).sum()))
