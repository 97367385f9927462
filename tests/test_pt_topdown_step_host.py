"""CPU: one (node, ray) step of the wave kernel's top-down sweep (topdown_step, csrc/pt_trace.h: each child's `times` from one select
per field on a mask) compiled for the host (tests/host_emu/topdown_step_host.cpp) against the long form it replaces - closer and
second chosen as student/bvh.inl:186-209 chooses them, then handed to the children - bit for bit: the flag nibble, cur_far_t.x and
both children's times, on 2^16 random cases (both boxes hit, one, none; ties) and with incoming times that are NaN, inverted or
infinite.  Renders through it: tests/test_pt_point_affine_gpu.py."""
import ctypes

import numpy as np

import _harness as H

_lib = None
F = np.float32


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("topdown_step_host", ["topdown_step_host.cpp"]))
    return _lib


def _cases(seed, n):
    rng = np.random.default_rng(seed)

    def box():
        a, b = rng.uniform(-1, 1, (n, 3)).astype(F), rng.uniform(-1, 1, (n, 3)).astype(F)
        return np.minimum(a, b), np.maximum(a, b)

    (ll, lh), (rl, rh) = box(), box()
    same = rng.random(n) < 0.1                          # the same box twice: equal entry times, the right child goes first
    rl, rh = np.where(same[:, None], ll, rl), np.where(same[:, None], lh, rh)
    org = rng.uniform(-2, 2, (n, 3)).astype(F)
    d = (rng.uniform(-0.7, 0.7, (n, 3)).astype(F) - org).astype(F)
    d = np.where(d == 0, F(0.125), d)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    with np.errstate(divide="ignore"):
        inv = (F(1) / d).astype(F)
    cam = rng.random(n) < 0.5
    rb = np.stack([np.where(cam, F(0), F(0.001)), np.where(cam, F(np.inf), np.finfo(F).max)], axis=1).astype(F)
    times = rb.copy()
    k = rng.integers(0, 8, n)
    times[k == 1] = (np.nan, np.inf)
    times[k == 2] = (3.0, 1.0)
    times[k == 3] = (0.0, np.nan)
    times[k == 4] = (1.0, 2.5)
    return np.ascontiguousarray(np.concatenate([ll, lh, rl, rh, org, inv, times, rb], axis=1), F)


def test_topdown_step_equals_the_long_form():
    c = _cases(91, 1 << 16)
    out = np.zeros((len(c), 12), np.uint32)
    assert _host().topdown_step_host(H.P(c), ctypes.c_size_t(len(c)), H.P(out)) == 0
    bad = np.argwhere((out[:, :6] != out[:, 6:]).any(axis=1)).ravel()
    assert bad.size == 0, (len(bad), out[bad[:5]])
    flags = np.bincount(out[:, 0], minlength=16)
    print("flag nibbles:", flags)
    assert all(flags[f] > 100 for f in (0, 2, 5, 11, 15)) and flags[[1, 3, 4, 6, 7, 8, 9, 10, 12, 13, 14]].sum() == 0
