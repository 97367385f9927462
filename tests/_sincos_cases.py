"""Arguments for the SRT-MATH v2 sin / cos checks (tests/test_pt_sincos_host.py, tests/test_pt_sincos_gpu.py), and the oracle's
values for them.  The thresholds are glibc's abstop12 values: 0x398 (2^-12), 0x3f4 (pi / 4 as a float) and 0x42f (120)."""
import ctypes

import numpy as np

import _harness as H

THRESHOLD_TOPS = (0x398, 0x3f4, 0x42f)


def around(bits, ulps=64):
    """The floats within `ulps` steps of the positive float with these bits, in both signs."""
    b = np.arange(int(bits) - ulps, int(bits) + ulps + 1, dtype=np.int64)
    b = b[(b >= 0) & (b < 0x7f800000)].astype(np.uint32)
    return np.concatenate([b, b | np.uint32(0x80000000)]).view(np.float32)


def thresholds():
    return np.concatenate([around(t << 20) for t in THRESHOLD_TOPS])


def quadrant_edges():
    """+-64 ulps around every k * pi / 4, k = 0 .. 152 (152 * pi / 4 = 119.4: the last one below 120), both signs."""
    k = np.arange(0, 153, dtype=np.float64) * (np.pi / 4)
    return np.concatenate([around(c) for c in k.astype(np.float32).view(np.uint32)])


def randoms(seed):
    """2^20 arguments in [0, 2 pi) and 2^20 in [-1, 1]: the two ranges the renderer evaluates."""
    rng = np.random.default_rng(seed)
    return (rng.random(1 << 20, dtype=np.float32) * np.float32(2 * np.pi)).astype(np.float32), rng.random(1 << 20, dtype=np.float32) * 2 - 1


def specials():
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x39000000, 0xb9000000,
                     0x42efcccd, 0xc2efcccd, 0x42f00000, 0xc2f00000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f7fffff],
                    np.uint32)             # +-0, denormals, the smallest normal, +-2^-13, +-119.9, +-120, +-inf, NaN, FLT_MAX
    return bits.view(np.float32)


def oracle_cos_sin(x):
    x = np.ascontiguousarray(x, np.float32)
    c, s = np.zeros_like(x), np.zeros_like(x)
    H.oracle().srt_oracle_math_cos_sin(H.P(x), ctypes.c_size_t(len(x)), H.P(c), H.P(s))
    return c, s


def same_bits(a, b):
    """Elementwise: equal bit patterns, any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def quadrant(x):
    """n of the reduction, as the functions compute it (for the arguments below 120)."""
    r = x.astype(np.float64) * float.fromhex("0x1.45F306DC9C883p+23")
    return (np.trunc(r).astype(np.int64) + 0x800000) >> 24
