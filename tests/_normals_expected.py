"""Expected values of the normal-colors debug view (srt_pt_set_normal_colors; debug_data.normal_colors,
student/pathtracer.cpp:199), assembled from pieces that are already pinned to the reference build:

  * SRT-RNG v1's key and first two draws (csrc/pt_device.h: Rng) in Python integers,
  * Camera::generate_ray (student/camera.cpp:7-34) + Ray::transform (lib/ray.h:31-37) in float32, operation by operation
    as camera_ray / ray_transform do them - numpy rounds after every operation, nothing is fused - with screen_h from
    libm's tanf, the function the host calls,
  * scene.hit through the oracle (srt_oracle_pt_hit, pinned to the reference's ref_pt_hit), Spectrum::direction
    (lib/spectrum.h:47-52, lib/vec3.h:141-159) applied to the hit's normal in float32,
  * for a camera ray that leaves the scene, what the oracle's ordinary render returns for the same (x, y, sample):
    env_light.evaluate(ray.dir) or zero (student/pathtracer.cpp:182-188).

tests/test_pt_normals_host.py checks the ray construction against rays the reference build logged."""
import ctypes
import ctypes.util

import numpy as np

import _harness as H

F = np.float32
M64 = (1 << 64) - 1
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = ctypes.c_float
_libm.tanf.argtypes = [ctypes.c_float]


def first_two_draws(seed, pixel, sample):
    """Rng::key(seed, pixel, sample) and the first two Rng::unit() values, as float32."""
    k = ((pixel << 32) | sample) & M64
    z = (seed + 0x9E3779B97F4A7C15 * (k + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    inc = ((k << 1) | 1) & M64
    state = (z * 6364136223846793005 + inc) & M64
    out = []
    for _ in range(2):
        old = state
        state = (old * 6364136223846793005 + inc) & M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        nxt = ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF
        out.append(F(nxt >> 8) * F(1.0 / 16777216.0))
    return out


def screen_size(camera):
    """(screen_h, screen_w) as make_camera computes them (student/camera.cpp:17-18) with the host's tanf."""
    vfov, ar = F(camera["vfov"]), F(camera["ar"])
    pi = F(3.14159265358979323846264338327950288)
    half = F(F(vfov * F(pi / F(180.0))) / F(2.0))
    sh = F(F(F(_libm.tanf(ctypes.c_float(float(half)))) * F(1.0)) * F(2.0))
    return sh, F(ar * sh)


def camera_rays(camera, w, h, seed, xs, ys, ss):
    """(origins [n, 3], directions [n, 3], bounds [n, 2]) of trace_pixel's camera rays for the (x, y, sample) triples."""
    xs, ys, ss = (np.asarray(a, np.int64) for a in (xs, ys, ss))
    n = len(xs)
    j = np.zeros((n, 2), F)
    for i in range(n):
        j[i] = first_two_draws(int(seed), int(ys[i]) * int(w) + int(xs[i]), int(ss[i]))
    sh, sw = screen_size(camera)
    sx = ((xs.astype(F) + j[:, 0] * F(1.0)).astype(F) / F(w)).astype(F)
    sy = ((ys.astype(F) + j[:, 1] * F(1.0)).astype(F) / F(h)).astype(F)
    d = np.stack([(sx * sw).astype(F) - F(F(0.5) * sw), (sy * sh).astype(F) - F(F(0.5) * sh), np.full(n, -1.0, F)], 1).astype(F)
    m = np.asarray(camera["iview"], F).reshape(4, 4)            # m[c][j]: column-major, Mat4::data order
    zero, one = F(0.0), F(1.0)
    # Mat4 * Vec3 of the origin (0, 0, 0), projective (lib/mat4.h:125-131)
    o4 = [F(F(F(m[0][k] * zero + m[1][k] * zero) + m[2][k] * zero) + m[3][k] * one) for k in range(4)]
    org = np.tile(np.array([F(o4[0] / o4[3]), F(o4[1] / o4[3]), F(o4[2] / o4[3])], F), (n, 1))
    # Mat4::rotate of the direction (w = 0; the 0 * column-3 term is kept)
    r = np.stack([((((m[0][k] * d[:, 0]).astype(F) + (m[1][k] * d[:, 1]).astype(F)).astype(F) + (m[2][k] * d[:, 2]).astype(F)).astype(F)
                   + F(m[3][k] * zero)).astype(F) for k in range(3)], 1)
    dn = np.sqrt((((r[:, 0] * r[:, 0]).astype(F) + (r[:, 1] * r[:, 1]).astype(F)).astype(F) + (r[:, 2] * r[:, 2]).astype(F)).astype(F)).astype(F)
    bounds = np.stack([(zero * dn).astype(F), np.full(n, np.inf, F)], 1).astype(F)      # dist_bounds (0, inf) times the norm
    dirs = (r / dn[:, None]).astype(F)
    return org.astype(F), dirs, bounds


def direction(v):
    """Spectrum::direction: Vec3::normalize (n = sqrtf(x*x + y*y + z*z), three divisions), then absolute values; no sRGB curve."""
    v = np.asarray(v, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        n = np.sqrt((((v[:, 0] * v[:, 0]).astype(F) + (v[:, 1] * v[:, 1]).astype(F)).astype(F) + (v[:, 2] * v[:, 2]).astype(F)).astype(F)).astype(F)
        return np.abs((v / n[:, None]).astype(F)).astype(F)


def expected_samples(oracle, scene, w, h, seed, xs, ys, ss):
    """(rgb [n, 3], hit [n] bool) of the view's samples; `oracle` is an H.OraclePT of `scene` at w x h."""
    xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
    org, dirs, bounds = camera_rays(scene["camera"], w, h, seed, xs, ys, ss)
    t = oracle.hit(org, dirs, bounds)
    hit = t[:, 0] != 0
    rgb = np.zeros((len(xs), 3), F)
    rgb[hit] = direction(t[hit, 5:8])
    if (~hit).any():
        rgb[~hit] = oracle.trace_samples(seed, xs[~hit], ys[~hit], ss[~hit])[0]
    return (rgb + F(0.0)).astype(F), hit                        # `emissive + reflected`, reflected == {}


def valid_mean(samples):
    """do_trace's epoch mean (rays/pathtracer.cpp:216-226): samples [s, ..., 3] in sample order, the sum of the valid ones times
    1.0f / count; zero where none is valid."""
    samples = np.asarray(samples, F)
    acc = np.zeros(samples.shape[1:], F)
    cnt = np.zeros(samples.shape[1:-1], np.int64)
    for s in samples:
        ok = np.isfinite(s).all(axis=-1)
        acc[ok] = (acc[ok] + s[ok]).astype(F)
        cnt += ok
    some = cnt > 0
    acc[some] = (acc[some] * (F(1.0) / cnt[some].astype(F)).astype(F)[..., None]).astype(F)
    return acc


def expected_epoch(oracle, scene, w, h, seed, base, n):
    """([n, h, w, 3] per-sample radiance, [h, w, 3] epoch image) of the view."""
    ys, xs = (a.reshape(-1) for a in np.mgrid[0:h, 0:w])
    per = np.stack([expected_samples(oracle, scene, w, h, seed, xs, ys, np.full(w * h, base + k))[0].reshape(h, w, 3) for k in range(n)])
    return per, valid_mean(per)
