"""Cases of srt_pt_set_env_sampling("image"): Env_Map's importance sampler, Samplers::Sphere::Image (student/samplers.cpp:27-137).

MAPS: the environment maps of the component fixture (tests/golden/env_image_components.npz) - the sampler's tables, sample() for
chosen draws and pdf() for chosen directions, recorded from the reference's own class.  PATH_SCENES: the scenes of the path fixture
(tests/golden/env_image_paths.npz) - renders of the reference's path tracer with the image sampler switched on.  Same name ->
same arrays, every time."""
import numpy as np

from _cases import pt_scene

F = np.float32
W, H, DEPTH, SEED = 32, 24, 6, 20261021
SAMPLE_INDICES = (0, 1, 5, 300)              # per-sample radiance and draw counts of every pixel at these sample indices
EPOCH_SPP, EPOCH_BASE = 6, 2


def _random(h, w, seed):
    return np.ascontiguousarray(np.random.default_rng(seed).uniform(0.0, 1.5, (h, w, 3)).astype(F))


def _sun():
    img = (F(0.1) + np.random.default_rng(61).uniform(0.0, 0.02, (8, 16, 3))).astype(F)
    img[2, 11] = F(1e4)
    return np.ascontiguousarray(img)


def _zero_runs():
    img = _random(5, 6, 62)
    img[0, 0:3] = 0       # a run at the very start: the first CDF entries are equal (and zero)
    img[2, 1:5] = 0       # a run inside a row
    img[3, 4:] = 0        # a run across a row boundary ...
    img[4, 0:2] = 0
    img[4, 5] = 0         # ... and one at the very end
    return np.ascontiguousarray(img)


def _negative():
    from _shade_edge_cases import shade_edge_scene

    return np.ascontiguousarray(shade_edge_scene("envmap_3x4_negative")["env"]["image"], F)


MAPS = {
    "1x1": lambda: _random(1, 1, 63),
    "2x1": lambda: _random(1, 2, 64),          # w = 2, h = 1
    "1x2": lambda: _random(2, 1, 65),          # w = 1, h = 2
    "3x4": lambda: _random(4, 3, 66),
    "cbox_envmap": lambda: np.ascontiguousarray(pt_scene("cbox_envmap")["env"]["image"], F),   # 37 x 19
    "sun16x8": _sun,
    "zero_runs": _zero_runs,
    "negative": _negative,
    "black": lambda: np.zeros((3, 4, 3), F),
}


def env_map(name):
    return MAPS[name]()


def draws(name, cdf):
    """The draws sample() is recorded for: 0, every CDF value and its float32 neighbours (the exact boundaries of upper_bound),
    1 - 2^-24 (the largest value RNG::unit returns) and 256 random draws of RNG::unit's form (k / 2^24)."""
    cdf = np.asarray(cdf, F)
    exact = cdf[np.isfinite(cdf)]
    u = np.concatenate([[F(0)], exact, np.nextafter(exact, F(-np.inf)), np.nextafter(exact, F(np.inf)), [F(1) - F(2.0 ** -24)],
                        (np.random.default_rng(700 + list(MAPS).index(name)).integers(0, 1 << 24, 256).astype(F) * F(2.0 ** -24))]).astype(F)
    return np.ascontiguousarray(u[(u >= 0) & (u < 1)])


def directions(name, sampled):
    """The directions pdf() is recorded for: every direction sample() returned, +-y, directions with dir.x = 0 and dir.z = +-0 (atan2's
    special cases), and 256 random unit directions."""
    rng = np.random.default_rng(800 + list(MAPS).index(name))
    r = rng.normal(size=(256, 3))
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)
    special = np.array([[0, 1, 0], [0, -1, 0], [0, 0.5, 0.0], [0, 0.5, -0.0], [0, -0.25, 0.0], [0.0, 0.0, 0.0], [0, 0.6, 0.8], [0, 0.6, -0.8],
                        [1, 0, 0.0], [1, 0, -0.0], [-1, 0, 0.0], [-1, 0, -0.0], [0.6, 0.8, 0], [0, 1.5, 0], [0.3, np.nan, 0.2]], F)
    return np.ascontiguousarray(np.concatenate([np.asarray(sampled, F).reshape(-1, 3), special, r]).astype(F))


def trig_tables(w, h):
    """What sample() multiplies (student/samplers.cpp:103-112), restated here on its own: theta and phi of rows 0 .. h and columns
    0 .. w - 1 in float32 as the reference computes and clamps them, then the C library's double sin / cos of them (math.sin / math.cos
    call libm).  Returns sin theta, cos theta (h + 1 each), cos phi, sin phi (w each) as float64."""
    import math

    pi = F(3.14159265358979323846264338327950288)
    two_pi = F(F(2.0) * pi)
    theta = [min(max(F(pi - F(F(pi * F(r)) / F(h))), F(0)), pi) for r in range(h + 1)]
    phi = [min(max(F(F(two_pi * F(c)) / F(w)), F(0)), two_pi) for c in range(w)]
    f64 = lambda fn, xs: np.array([fn(float(x)) for x in xs], np.float64)
    return f64(math.sin, theta), f64(math.cos, theta), f64(math.cos, phi), f64(math.sin, phi)


def _envmap():
    return pt_scene("cbox_envmap")                      # area light + map: sample_area_lights flips its coin


def _envonly_sun():
    s = pt_scene("cbox_envonly")                        # no area light (nlights == 0): every light sample is the map's
    s["env"] = {"type": 3, "image": env_map("sun16x8")}
    return s


def _deltalights_map():
    s = pt_scene("cbox_deltalights")                    # delta lights + area light + map
    s["env"] = {"type": 3, "image": env_map("3x4")}
    return s


PATH_SCENES = {"cbox_envmap": _envmap, "cbox_envonly_sun": _envonly_sun, "cbox_deltalights_map": _deltalights_map}


def path_scene(name):
    return PATH_SCENES[name]()


def sample_list():
    ys, xs, ss = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), np.asarray(SAMPLE_INDICES, np.uint32), indexing="ij")
    return np.ascontiguousarray(xs.reshape(-1)), np.ascontiguousarray(ys.reshape(-1)), np.ascontiguousarray(ss.reshape(-1))


def sin_unit_arguments():
    """Every 4096th float of [0, 1], every float within 64 ulps of a branch boundary of the restatement (2^-26, 0.126, 0.85546875, 1)
    or of a table boundary (the odd multiples of 1 / 256, where x + big rounds to the next multiple of 1 / 128), 0, denormals and 1."""
    one = int(np.float32(1).view(np.uint32))
    bits = [np.arange(0, one + 1, 4096, dtype=np.int64)]
    edges = [2.0 ** -26, float.fromhex("0x1.020c49ba5e354p-3"), 0.85546875, 1.0] + [(2 * k + 1) / 256.0 for k in range(128)]
    for e in edges:
        b = int(np.float32(e).view(np.uint32))
        bits.append(np.arange(max(b - 64, 0), min(b + 64, one) + 1, dtype=np.int64))
    bits.append(np.array([0, 1, 2, 0x7fffff, 0x800000, 0x800001, one], np.int64))
    return np.unique(np.concatenate(bits)).astype(np.uint32).view(np.float32)
