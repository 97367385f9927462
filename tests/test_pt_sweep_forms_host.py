"""CPU: the bottom-up sweep on the two-word hit (packed_fold, packed_combine, csrc/pt_trace.h) compiled for the host
(tests/host_emu/sweep_forms_host.cpp) against the four-field form it replaces - fold / left_wins, the visit rule
`cur_far_t.x < ret.distance || (!ret.hit && hitboth)` and Trace::min on Hit {hit, dist, obj, tri} - over every combination of
child results, flags and far times; bit for bit, NaN payloads included.  The HIP build of the same functions is what
tests/test_pt_sweep_forms_gpu.py renders with."""
import ctypes
import itertools

import numpy as np

import _harness as H

MISS = 0xFFFFFFFF
NAN = np.float32(np.nan)
INF = np.float32(np.inf)
_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("sweep_forms_host", ["sweep_forms_host.cpp"]))
    return _lib


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _check(out, what):
    out = out.reshape(-1, 5)
    bad = np.argwhere((out[:, 0] != out[:, 2]) | (out[:, 1] != out[:, 3]))
    assert bad.size == 0, (what, len(bad), bad[:5].ravel(), out[bad[:5].ravel()])
    miss = out[:, 1] == MISS
    assert (miss == (out[:, 4] == 0)).all(), what
    assert (out[miss, 0] == 0).all(), (what, "a miss carries distance +0")
    return out


def test_combine_enumerated():
    """Both children over {miss} + {hit} x {1, 2, 3, +0, inf, NaN} (nearer / farther / equal among them), every flag triple
    {either box hit, left nearer, hitboth}, far times below, between, on and above the distances, NaN, +0, inf and negative."""
    dists = [1.0, 2.0, 3.0, 0.0, INF, NAN]
    left = [(0.0, MISS)] + [(d, (2 << 27) | 5) for d in dists]
    right = [(0.0, MISS)] + [(d, (7 << 27) | 1) for d in dists]
    farx = [0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, NAN, 0.0, INF, -1.0]
    cases = [[_bits(l[0]), l[1], _bits(r[0]), r[1], f, _bits(x)] for l, r, f, x in itertools.product(left, right, range(8), farx)]
    a = np.ascontiguousarray(cases, np.uint32)
    out = np.zeros((len(a), 5), np.uint32)
    assert _host().sweep_combine_host(H.P(a), ctypes.c_size_t(len(a)), H.P(out)) == 0
    out = _check(out, "combine")
    assert len(a) == 7 * 7 * 8 * 11
    flags = a[:, 4]
    assert (out[(flags & 1) == 0, 1] == MISS).all(), "a node whose boxes were both missed returns the default Trace"
    took_l, took_r = out[:, 1] == ((2 << 27) | 5), out[:, 1] == ((7 << 27) | 1)
    assert took_l.any() and took_r.any() and (out[:, 1] == MISS).any()
    # the farther child's result is selected somewhere although the nearer one hit (farx below its distance), and skipped somewhere
    nearer_is_left = (flags & 2) != 0
    assert (took_r & nearer_is_left & (a[:, 1] != MISS)).any() and (took_l & nearer_is_left & (a[:, 3] != MISS)).any()


def test_fold_enumerated():
    """Leaves of one to four candidates, each a miss (distance +0, or whatever an object test leaves there: 5, NaN) or a hit at
    1, 2, 2 again (ties: the later one wins), +0, inf or NaN."""
    cands = [(0, 0.0), (0, 5.0), (0, NAN), (1, 1.0), (1, 2.0), (1, 0.0), (1, INF), (1, NAN)]
    for m in (1, 2, 3, 4):
        rows = []
        for combo in itertools.product(range(len(cands)), repeat=m):
            for j, c in enumerate(combo):
                rows.append([cands[c][0], _bits(cands[c][1]), 3 + j, 11 * j])
        a = np.ascontiguousarray(rows, np.uint32)
        n = len(a) // m
        out = np.zeros((n, 5), np.uint32)
        assert _host().sweep_fold_host(H.P(a), ctypes.c_size_t(n), ctypes.c_size_t(m), H.P(out)) == 0
        out = _check(out, f"fold of {m}")
        assert n == len(cands) ** m
        if m > 1:
            assert len(np.unique(out[:, 1])) == m + 1        # every position wins somewhere, and a leaf of misses stays a miss
