"""Inputs for the Triangle::hit verdict tests (tests/test_pt_tri_verdict_{gpu,host}.py): n sets of one triangle {p0, e1, e2},
one origin, three rays (direction, dist_bounds) - the shape of a batch of the wave kernel.  Everything is generated from a seed."""
import numpy as np

F = np.float32
EPS = F(0.00001)
INF = F(np.inf)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_sets(seed, n):
    """(a) random triangles and rays in and around the Cornell box (a cube of side 2 around the origin): the rays of a set aim at
    points of the triangle's plane spread over and around the triangle, so that about a third of them hit."""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(-1.2, 1.2, (n, 3))
    e1 = rng.uniform(-1.5, 1.5, (n, 3))
    e2 = rng.uniform(-1.5, 1.5, (n, 3))
    org = rng.uniform(-1.5, 1.5, (n, 3))
    uv = rng.uniform(-0.5, 1.2, (n, 3, 2))
    target = p0[:, None, :] + uv[:, :, :1] * e1[:, None, :] + uv[:, :, 1:] * e2[:, None, :]
    dirs = _unit(target - org[:, None, :])
    dirs[rng.random((n, 3)) < 0.1] *= -1.0                      # the triangle behind the ray: t < 0
    bounds = np.empty((n, 3, 2))
    bounds[:, :, 0] = np.where(rng.random((n, 3)) < 0.5, 0.0, EPS)
    bounds[:, :, 1] = np.where(rng.random((n, 3)) < 0.7, np.inf, rng.uniform(0.1, 3.0, (n, 3)))
    tri = np.concatenate([p0, e1, e2], axis=1)
    return tri.astype(F), org.astype(F), dirs.astype(F), bounds.astype(F)


def _step(x, k):
    """x moved by k units in the last place (x: float32 array, k: integer array), through the bit pattern; crosses zero."""
    x = np.asarray(x, F)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k               # sign-magnitude -> a monotone integer line
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(F)


def constructed_sets(seed):
    """(b) the cases around every comparison of the verdict.  Unit-square sets first: p0 = 0, e1 = x, e2 = y (scaled by a power of
    two), origin (x, y, h), direction -z, so that u = x, v = y, t = h exactly; then general triangles whose rays aim at points
    with u + v = 1 within a few units in the last place; then operands outside the fast path's window."""
    rng = np.random.default_rng(seed)
    tris, orgs, dirss = [], [], []

    def square(x, y, h, scale, d=(0.0, 0.0, -1.0)):
        n = len(x)
        s = np.asarray(scale, F).reshape(-1, 1) * np.ones((n, 1), F)
        z = np.zeros((n, 1), F)
        tris.append(np.concatenate([z, z, z, s, z, z, z, s, z], axis=1).astype(F))
        orgs.append(np.stack([np.asarray(x, F) * s[:, 0], np.asarray(y, F) * s[:, 0], np.asarray(h, F) * np.ones(n, F)], axis=1).astype(F))
        dd = np.broadcast_to(np.asarray(d, F), (n, 3, 3)).copy()
        # the three rays of a set: straight down, and two slightly tilted ones (the same triangle seen a little off)
        dd[:, 1, 0] += F(2.0 ** -12); dd[:, 2, 1] -= F(2.0 ** -11)
        dirss.append(dd)

    k = np.arange(-64, 65)
    reps = 24
    kk = np.tile(k, reps)
    n = len(kk)
    for scale in (1.0, 2.0 ** -7, 2.0 ** 9, 3.0):
        x = rng.uniform(0.05, 0.95, n).astype(F)
        square(x, _step(F(1.0) - x, kk), np.full(n, 1.0), scale)                         # u + v within 64 ulp of 1
        y = rng.uniform(0.05, 0.9, n).astype(F)
        square(_step(np.zeros(n, F), kk), y, np.full(n, 0.5), scale)                      # u within 64 ulp of 0 (denormal offsets)
        square(y, _step(np.zeros(n, F), kk), np.full(n, 0.5), scale)                      # v within 64 ulp of 0
        square(_step(np.full(n, 2.0 ** -30, F), kk) * np.sign(kk + 0.5).astype(F), y, np.full(n, 2.0), scale)   # small u of either sign, in the window
        square(_step(np.ones(n, F), kk), _step(np.zeros(n, F), np.abs(kk)), np.full(n, 1.0), scale)   # u within 64 ulp of 1, v at 0
        square(_step(np.zeros(n, F), np.abs(kk)), _step(np.ones(n, F), kk), np.full(n, 1.0), scale)   # v within 64 ulp of 1
        square(_step(np.ones(n, F), kk), np.full(n, 2.0 ** -24, F), np.full(n, 0.75), scale)          # u near 1 with a small positive v
        square(x, _step(F(1.0) - x, kk), np.zeros(n), scale)                              # nt == 0: the origin on the plane
        square(x, _step(F(1.0) - x, kk), np.full(n, -1.0), scale)                         # behind: t < 0
        square(x, y * F(0.5), np.full(n, 1.0), scale, d=(1.0, 0.0, 0.0))                  # det == 0 for ray 0: parallel to the plane
    # general triangles, targets on the edge u + v = 1 (float64 construction; the rounding of the inputs scatters the lanes
    # over both sides of the edge, a good share of them inside the ambiguous band)
    m = 40000
    p0 = rng.uniform(-1.0, 1.0, (m, 3)); e1 = rng.uniform(-1.5, 1.5, (m, 3)); e2 = rng.uniform(-1.5, 1.5, (m, 3))
    p0, e1, e2 = (a.astype(F).astype(np.float64) for a in (p0, e1, e2))
    org = rng.uniform(-1.5, 1.5, (m, 3)).astype(F).astype(np.float64)
    u = rng.uniform(0.0, 1.0, (m, 3))
    v = 1.0 - u + rng.integers(-64, 65, (m, 3)) * 2.0 ** -24
    target = p0[:, None, :] + u[..., None] * e1[:, None, :] + v[..., None] * e2[:, None, :]
    tris.append(np.concatenate([p0, e1, e2], axis=1).astype(F)); orgs.append(org.astype(F)); dirss.append(_unit(target - org[:, None, :]).astype(F))
    # operands outside the window: huge and tiny triangles, denormal, infinite and NaN coordinates, salted into ordinary sets
    t0, o0, d0, _ = random_sets(seed + 1, 16384)
    t0, o0, d0 = t0.copy(), o0.copy(), d0.copy()
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 2.0 ** -60, -(2.0 ** -60), 2.0 ** 60, -(2.0 ** 60), 2.0 ** -126, 3.4028235e38,
                        np.inf, -np.inf, np.nan], F)
    for arr, share in ((t0, 0.02), (o0, 0.01), (d0.reshape(-1, 9), 0.01)):
        hit = rng.random(arr.shape) < share
        arr[hit] = rng.choice(special, int(hit.sum()))
    with np.errstate(all="ignore"):                                                    # whole sets scaled out of the window
        t0[:2048] *= F(2.0 ** 60); o0[:2048] *= F(2.0 ** 60)
        t0[2048:4096] *= F(2.0 ** -60); o0[2048:4096] *= F(2.0 ** -60)
    tris.append(t0); orgs.append(o0); dirss.append(d0)
    tri, org, dirs = np.concatenate(tris), np.concatenate(orgs), np.concatenate(dirss)
    n = len(tri)
    bounds = np.empty((n, 3, 2), F)
    bounds[:, :, 0] = np.where(rng.random((n, 3)) < 0.5, F(0.0), EPS)
    bounds[:, :, 1] = np.where(rng.random((n, 3)) < 0.8, INF, F(3.4028235e38))
    return tri, org, dirs, bounds
