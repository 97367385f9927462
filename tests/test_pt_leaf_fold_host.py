"""CPU: the candidate bookkeeping of the wave kernel's leaf fold (leaf_cand_add / tri_verdict, csrc/pt_device.h) compiled for the
host (tests/host_emu/leaf_fold_host.cpp): wherever no lane of a leaf's batch is flagged bad, the plain tri_hit of the ray's single
candidate - the default Trace when it has none or the candidate misses - equals the ordered fold of the plain tri_hit over the
whole leaf, bit for bit.  Also that the constructed groups lie where they claim to: group F without a flagged lane, group M with
every lane flagged.  The HIP build of the leaf code, and its fallback, are checked by tests/test_pt_leaf_fold_gpu.py."""
import ctypes

import numpy as np

import _harness as H
from _leaf_fold_cases import group_a, group_f, group_m, random_sets

_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("leaf_fold_host", ["leaf_fold_host.cpp"]))
    return _lib


def run_host(s):
    """-> (bad (W, 64) bool, out (W, 64, 3, 9) uint32) of leaf_fold_host on a set of tests/_leaf_fold_cases.py."""
    W = len(s["ntri"])
    bad = np.zeros((W, 64), np.uint32)
    out = np.zeros((W, 64, 3, 9), np.uint32)
    arrs = [np.ascontiguousarray(s[k], np.uint32 if k == "ntri" else np.float32) for k in ("tris", "ntri", "org", "dirs", "bounds")]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert _host().leaf_fold_host(*(p(a) for a in arrs), ctypes.c_size_t(W), p(bad), p(out)) == 0
    return bad != 0, out


def _check(bad, out):
    """Lanes that are not flagged: at most one candidate per ray, and the candidate's own test is the fold's result."""
    good = ~bad
    assert (out[good][..., 0] <= 1).all()
    cand, fold = out[good][..., 1:5], out[good][..., 5:9]
    wrong = np.argwhere((cand != fold).any(axis=-1))
    assert wrong.size == 0, (len(wrong), wrong[:5], cand[(cand != fold).any(axis=-1)][:5], fold[(cand != fold).any(axis=-1)][:5])
    return good


def test_group_f_has_no_flagged_lane():
    bad, out = run_host(group_f(51))
    assert not bad.any(), np.argwhere(bad)[:8]
    _check(bad, out)
    hit, count = out[..., 5] != 0, out[..., 0]
    print("group F:", bad.shape[0], "waves; rays with a candidate", int((count == 1).sum()), "hits", int(hit.sum()), "of", hit.size)
    assert hit.any() and (~hit).any() and (count == 0).any()
    assert ((count == 1) & ~hit).any()                # candidates behind the origin or cut by the bounds
    assert (hit & (out[..., 7] << 1 == 0)).any()      # t == +-0: hits of origins on the plane


def test_group_m_flags_every_lane():
    s = group_m(52)
    bad, out = run_host(s)
    assert bad.all(), np.argwhere(~bad)[:8]
    two = out[..., 0] >= 2
    print("group M:", bad.shape[0], "waves; rays with two candidates or more", int(two.sum()), "of", two.size)
    assert two.any()
    # the stacked pairs: the fold keeps the nearer triangle, and the later one at equal distances
    stacked = slice(9, 13)
    tri = out[stacked][..., 6]
    assert (out[stacked][..., 5] != 0).all()
    assert (tri[0] == 0).all() and (tri[1] == 1).all() and (tri[2] == 1).all() and (tri[3] == 1).all()


def test_group_a_and_random_sets():
    for name, s in (("group A", group_a(53)), ("random", random_sets(54, 1024))):
        bad, out = run_host(s)
        good = _check(bad, out)
        print(name + ":", bad.shape[0], "waves,", int(good.sum()), "lanes not flagged, waves without a flagged lane", int((~bad.any(axis=1)).sum()))
        if name == "random":
            assert 0.2 < good.mean() < 0.95 and (~bad.any(axis=1)).any() and bad.any(axis=1).any()
        else:
            assert bad.any() and bad.any(axis=1).mean() > 0.9
