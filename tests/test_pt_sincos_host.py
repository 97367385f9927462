"""CPU: the branch-free srt_sincosf / srt_sincosf2 (csrc/pt_device.h) compiled for the host (tests/host_emu/sincos_host.cpp).
Held bit for bit to the _plain forms beside them (glibc's control flow) on every float below 256 in magnitude - every argument the
functions reduce, and one exponent step of those they refuse - and to the oracle's committed restatement on the threshold
neighbourhoods, the quadrant edges and the renderer's two ranges.  The double -> int32 conversion of the reduction is run under
-fsanitize=undefined,float-cast-overflow on NaN, infinities and large arguments by a program of its own.
The HIP build of the same functions is checked by tests/test_pt_sincos_gpu.py."""
import ctypes
import os

import numpy as np

import _harness as H
import _sincos_cases as SC

_lib = None


def _host():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(H.build_host_lib("sincos_host", ["sincos_host.cpp"], extra=("-pthread",)))
        _lib.sincos_sweep.restype = ctypes.c_uint64
        _lib.sincos_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        _lib.sincos_eval.restype = None
        _lib.sincos_eval.argtypes = [ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    return _lib


def host_eval(x):
    """-> (cos, sin) of srt_sincosf2, (cos, sin) of the single-function forms."""
    x = np.ascontiguousarray(x, np.float32)
    out = [np.zeros_like(x) for _ in range(4)]
    _host().sincos_eval(H.P(x), len(x), *(H.P(o) for o in out))
    return out


def test_every_float_below_256_equals_the_plain_forms():
    """Magnitude bits 0 .. 0x43800000 in both signs: all of |y| < 120 = 0x42f00000, then [120, 128) and the whole exponent of
    [128, 256), where both forms answer NaN."""
    first = ctypes.c_uint32(0)
    threads = max(1, min(16, os.cpu_count() or 1))
    bad = _host().sincos_sweep(0, 0x43800000, threads, ctypes.byref(first))
    print("arguments:", 2 * 0x43800000, "threads:", threads, "mismatches:", bad)
    assert bad == 0, (bad, hex(first.value))


def _held_to_the_oracle(x, what):
    oc, os_ = SC.oracle_cos_sin(x)
    c2, s2, c1, s1 = host_eval(x)
    for name, got, want in (("sincosf2 cos", c2, oc), ("sincosf2 sin", s2, os_), ("sincosf cos", c1, oc), ("sincosf sin", s1, os_)):
        wrong = np.flatnonzero(~SC.same_bits(got, want))
        assert wrong.size == 0, (what, name, len(wrong), x[wrong[:4]], got[wrong[:4]], want[wrong[:4]])


def test_thresholds_and_quadrant_edges_equal_the_oracle():
    x = SC.thresholds()
    tops = (x.view(np.uint32) >> 20) & 0x7ff
    for t in SC.THRESHOLD_TOPS:                       # both sides of every threshold are present
        assert (tops == t).any() and (tops == t - 1).any()
    _held_to_the_oracle(x, "thresholds")
    _held_to_the_oracle(SC.quadrant_edges(), "quadrant edges")
    _held_to_the_oracle(SC.specials(), "specials")


def test_renderer_ranges_equal_the_oracle():
    phi, cosine = SC.randoms(11)
    assert len(phi) == len(cosine) == 1 << 20 and phi.min() >= 0 and phi.max() < np.float32(2 * np.pi) + 1e-6 and np.abs(cosine).max() <= 1
    assert set(np.unique(SC.quadrant(phi))) == {0, 1, 2, 3, 4} and set(np.unique(SC.quadrant(cosine))) == {-1, 0, 1}
    _held_to_the_oracle(phi, "[0, 2 pi)")
    _held_to_the_oracle(cosine, "[-1, 1]")


def test_sanitized_program(tmp_path):
    """-fsanitize=undefined,float-cast-overflow over NaN, +-inf, +-0, denormals and |y| >= 120 (up to FLT_MAX): the conversion of the
    reduction must see a value in range for every one of them.  A program of its own, run as its own process."""
    H.run_sanitized_main(tmp_path, "sincos_host.cpp", scene_layer=False, expect="sincos_sanitized: ok", extra=("-DSINCOS_HOST_MAIN", "-pthread"),
                         flags=("-O1", "-g", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"))
