"""CPU: the logic of Triangle::hit's verdict from the numerators (tri_verdict, csrc/pt_device.h) compiled for the host
(tests/host_emu/tri_verdict_host.cpp): wherever a lane is inside the fast path's window and not ambiguous, the verdict equals the
reference's u < 0 || v < 0 || (1 - u - v) < 0 on the correctly rounded quotients.  The HIP build of the same function, and the
fallback of the ambiguous lanes, are checked by tests/test_pt_tri_verdict_gpu.py."""
import ctypes

import numpy as np

import _harness as H
from _tri_verdict_cases import constructed_sets, random_sets

_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("tri_verdict_host", ["tri_verdict_host.cpp"]))
    return _lib


def _run(tri, org, dirs, bounds):
    n = len(tri)
    out = np.zeros((n, 3, 7), np.uint32)
    arrs = [np.ascontiguousarray(a, np.float32) for a in (tri, org, dirs, bounds)]
    assert _host().tri_verdict_host(*(a.ctypes.data_as(ctypes.c_void_p) for a in arrs), ctypes.c_size_t(n), out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def _check(out):
    in_window, outside, ambiguous, reference = (out[..., k] != 0 for k in range(4))
    decided = in_window & ~ambiguous
    bad = np.argwhere(decided & (outside != reference))
    assert bad.size == 0, (len(bad), bad[:5])
    return in_window, ambiguous, decided


def test_verdict_on_constructed_sets():
    out = _run(*constructed_sets(32))
    in_window, ambiguous, decided = _check(out)
    print("constructed:", out.shape[0] * 3, "pairs, in the window", int(in_window.sum()), "ambiguous", int((in_window & ambiguous).sum()))
    assert (in_window & ambiguous).sum() > 1000 and decided.sum() > 100000 and (~in_window).sum() > 1000
    hit = out[..., 4] != 0
    assert hit.any() and not hit.all()


def test_verdict_on_random_sets():
    out = _run(*random_sets(31, 1 << 18))
    in_window, ambiguous, decided = _check(out)
    print("random:", out.shape[0] * 3, "pairs, in the window", int(in_window.sum()), "ambiguous", int((in_window & ambiguous).sum()))
    assert decided.mean() > 0.99                      # the branch the fallback takes is cold on ordinary rays
