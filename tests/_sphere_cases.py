"""Inputs for the Sphere::hit tests (tests/test_pt_sphere_{gpu,host}.py, tests/golden/make_refbuild_vectors.py): n sets of one
radius, one origin and three rays (direction, dist_bounds) - the shape of a batch of the wave kernel.  Everything is generated from
a seed.  A scene holds one sphere, so what goes through scene.hit is grouped by radius (by_radius): the generators draw the radii
from short palettes - the solved radii of family B included, see there - so that the sets need a few dozen scenes, not thousands."""
import numpy as np

F = np.float32
EPS = F(0.00001)
INF = F(np.inf)

FAMILIES = ("ordinary", "tangent_exact", "tangent_near", "on_surface", "inside", "behind", "far_bound", "near_bound", "odd_bounds",
            "specials", "scaled", "twin_roots")
FAM = {name: k for k, name in enumerate(FAMILIES)}
CHAIN = ("on_surface", "inside", "behind", "far_bound", "near_bound")       # the validity chain of the two-root branch
STEPS_A = 64                                                                # family A: o.x stepped by -64 .. +64 ulps
STEPS_B = 4                                                                 # family B: the radius stepped by -4 .. +4 ulps


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _step(x, k):
    """x moved by k units in the last place (x: float32 array, k: integer array), through the bit pattern; crosses zero."""
    x = np.asarray(x, F)
    i = x.view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7FFFFFFF), i) + k               # sign-magnitude -> a monotone integer line
    i = np.where(i < 0, (-i) | 0x80000000, i)
    return i.astype(np.uint32).view(F)


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def delta_f32(radius, org, dirs):
    """delta of Sphere::hit in float32, every operation rounded on its own and in the oracle's order (oracle/pt_oracle.c,
    sphere_hit).  radius (n,), org (n, 3), dirs (n, 3, 3) -> (n, 3).  For CLASSIFYING the sets only: no test takes it for the
    expected value of anything a kernel returns."""
    radius, org, dirs = np.asarray(radius, F), np.asarray(org, F), np.asarray(dirs, F)
    with np.errstate(all="ignore"):
        o = org[:, None, :]
        a = _dot32(dirs, dirs)
        b = F(2.0) * _dot32(np.broadcast_to(o, dirs.shape), dirs)
        c = (_dot32(org, org) - radius * radius)[:, None]
        return (b * b - F(4.0) * a * c).astype(F)


def roots_f32(radius, org, dirs):
    """The two roots of the delta > 0 branch and their distances, as the oracle forms them (sum, sqrt and quotient in float64,
    narrowed): (t1, t2, d1, d2), each (n, 3); t1 is the far root.  For CONSTRUCTING bounds that meet a root's distance exactly and
    for classifying the sets."""
    radius, org, dirs = np.asarray(radius, F), np.asarray(org, F), np.asarray(dirs, F)
    with np.errstate(all="ignore"):
        delta = delta_f32(radius, org, dirs)
        m2od = (F(-2.0) * _dot32(np.broadcast_to(org[:, None, :], dirs.shape), dirs)).astype(np.float64)
        den = (F(2.0) * _dot32(dirs, dirs)).astype(np.float64)
        sq = np.sqrt(delta.astype(np.float64))
        t1, t2 = ((m2od + sq) / den).astype(F), ((m2od - sq) / den).astype(F)
        dist = lambda t: np.abs(np.sqrt(_dot32(dirs * t[..., None], dirs * t[..., None])))
        return t1, t2, dist(t1).astype(F), dist(t2).astype(F)


def root_validity(radius, org, dirs, bounds):
    """(v1, v2) of the two-root branch - far root valid, near root valid - by the reference's chain, from roots_f32."""
    t1, t2, d1, d2 = roots_f32(radius, org, dirs)
    b0, b1 = bounds[..., 0], bounds[..., 1]
    with np.errstate(all="ignore"):
        v1 = ~(t1 < 0) & ~((d1 < b0) | (d1 > b1))
        v2 = ~(t2 < 0) & ~((d2 < b0) | (d2 > b1))
    return v1, v2


def _default_bounds(rng, n):
    b = np.empty((n, 3, 2), F)
    b[:, :, 0] = np.where(rng.random((n, 3)) < 0.5, F(0.0), EPS)
    b[:, :, 1] = np.where(rng.random((n, 3)) < 0.5, INF, rng.uniform(0.1, 3.0, (n, 3)).astype(F))
    return b


def _lengths(rng, shape, share=0.25):
    """1 for a normalised direction; a quarter of them 0.2 .. 5 (what particles send)."""
    return np.where(rng.random(shape) < share, rng.uniform(0.2, 5.0, shape), 1.0)


def random_sets(seed, n):
    """(radius, org, dirs, bounds): spheres of radius 0.05 .. 1.5 (eight radii drawn from the seed) at the origin, origins in a cube
    of side 3, rays aimed at points in and around the sphere so that both verdicts occur; a quarter of the directions are not
    normalised (length 0.2 .. 5); bounds {0, EPS} x {inf, U(0.1, 3)}."""
    rng = np.random.default_rng(seed)
    radius = rng.choice(rng.uniform(0.05, 1.5, 8).astype(F), n)
    org = rng.uniform(-1.5, 1.5, (n, 3))
    target = _unit(rng.normal(size=(n, 3, 3))) * (radius[:, None, None] * rng.uniform(0.0, 1.8, (n, 3, 1)))
    dirs = _unit(target - org[:, None, :]) * _lengths(rng, (n, 3, 1))
    return radius.astype(F), org.astype(F), dirs.astype(F), _default_bounds(rng, n)


def _rotations(rng, n):
    q = _unit(rng.normal(size=(n, 4)))
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def _about(axis, v, phi):
    """v rotated about the unit vector `axis` by phi (Rodrigues)."""
    c, s = np.cos(phi)[..., None], np.sin(phi)[..., None]
    return v * c + np.cross(axis, v) * s + axis * (np.sum(axis * v, -1, keepdims=True) * (1 - c))


def _family_a(rng, reps):
    """Exact tangents: o = (r, 0, -k), d = (0, 0, s) with r, k, s small dyadic numbers, so that every product is exact and delta is
    exactly 0; o.x then stepped by -64 .. +64 ulps.  The tangent point lies at t = k / s: ahead and behind (both signs of k and s);
    a third of the rays carry bounds that exclude it."""
    kk = np.tile(np.arange(-STEPS_A, STEPS_A + 1), reps)
    n = len(kk)
    r = rng.choice(np.array([0.5, 1.0], F), n)
    k = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0], F), n) * rng.choice(np.array([-1.0, 1.0], F), n)
    s = rng.choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0], F), (n, 3)) * rng.choice(np.array([-1.0, 1.0], F), (n, 3))
    org = np.stack([_step(r, kk), np.zeros(n, F), -k], axis=1).astype(F)
    dirs = np.zeros((n, 3, 3), F)
    dirs[:, :, 2] = s
    bounds = np.empty((n, 3, 2), F)
    bounds[:, :, 0] = np.where(rng.random((n, 3)) < 0.5, F(0.0), EPS)
    bounds[:, :, 1] = INF
    dist = np.abs(k)[:, None] * np.ones((1, 3), F)                        # |d * t| = |k|: the tangent point's distance
    u = rng.random((n, 3))
    bounds[:, :, 1] = np.where(u < 1 / 6, dist * F(0.5), bounds[:, :, 1])         # ends before the tangent point
    bounds[:, :, 0] = np.where((u >= 1 / 6) & (u < 1 / 3), dist * F(2.0), bounds[:, :, 0])   # starts beyond it
    p = rng.permutation(n)                                                # every wave holds steps of every size
    return r[p], org[p], dirs[p], bounds[p], kk[p]


def _family_b(rng, nseeds, per_radius):
    """Near tangents in general position.  The radius is solved in float64 from a random origin and direction,
    r^2 = |o|^2 - (o.d)^2 / |d|^2, rounded to float32 and stepped by -4 .. +4 ulps: `nseeds` such radii.  Each radius then serves
    many sets: the solved pair is moved along its own line and turned by a random rotation (both keep the line tangent), and the
    set's three rays lie on the tangent cone of its origin (the first direction turned about the origin's axis); a quarter of the
    directions are not normalised.  Rounding the origin and the directions to float32 scatters delta about zero as the step of the
    radius does."""
    radius, org, dirs = [], [], []
    for _ in range(nseeds):
        o0 = rng.uniform(-1.2, 1.2, 3)
        d0 = _unit(rng.normal(size=3))
        r0 = F(np.sqrt(o0 @ o0 - (o0 @ d0) ** 2))
        for step in range(-STEPS_B, STEPS_B + 1):
            m = per_radius
            R = _rotations(rng, m)
            o = np.einsum("nij,nj->ni", R, o0 + rng.uniform(-2.0, 2.0, (m, 1)) * d0)
            d = np.einsum("nij,j->ni", R, d0)
            axis = _unit(o)[:, None, :]
            phi = np.concatenate([np.zeros((m, 1)), rng.uniform(0.0, 2 * np.pi, (m, 2))], axis=1)
            d3 = _about(axis, d[:, None, :], phi) * _lengths(rng, (m, 3, 1)) * rng.choice([-1.0, 1.0], (m, 3, 1))
            radius.append(np.full(m, _step(r0, step), F)); org.append(o.astype(F)); dirs.append(d3.astype(F))
    radius, org, dirs = np.concatenate(radius), np.concatenate(org), np.concatenate(dirs)
    p = rng.permutation(len(radius))
    return radius[p], org[p], dirs[p], _default_bounds(rng, len(radius))[p]


CHAIN_RADII = np.array([0.5, 0.7], F)


def _aimed(rng, radius, org, spread=0.9):
    """Three directions from org towards points inside the sphere; a quarter not normalised."""
    n = len(radius)
    target = _unit(rng.normal(size=(n, 3, 3))) * (radius[:, None, None] * rng.uniform(0.0, spread, (n, 3, 1)))
    return (_unit(target - org[:, None, :]) * _lengths(rng, (n, 3, 1))).astype(F)


def _chain(rng, m):
    """The validity chain of the two-root branch, one family per way a root loses its validity; {family: (radius, org, dirs, bounds)}."""
    out = {}
    zero_eps = lambda shape: np.where(rng.random(shape) < 0.5, F(0.0), EPS).astype(F)
    open_bounds = lambda n: np.stack([zero_eps((n, 3)), np.full((n, 3), INF, F)], axis=-1)
    pick = lambda n: rng.choice(CHAIN_RADII, n)
    # the origin on the surface, by construction and 0 .. 4 ulps off either way: the near root is +-0 or closer than EPS, the far
    # root is the chord (directions into the sphere) - or both lie behind (directions out of it)
    r = pick(m)
    o = _step((_unit(rng.normal(size=(m, 3))) * r[:, None]).astype(F), rng.integers(-4, 5, (m, 1)))
    d = _aimed(rng, r, o.astype(np.float64))
    d[rng.random((m, 3)) < 0.2] *= F(-1.0)
    out["on_surface"] = (r, o, d, open_bounds(m))
    # the origin inside: the near root is behind the ray, the far one ahead - unless dist_bounds.y ends before it
    r = pick(m)
    o = (_unit(rng.normal(size=(m, 3))) * (r * rng.uniform(0.0, 0.95, m))[:, None]).astype(F)
    d = (_unit(rng.normal(size=(m, 3, 3))) * _lengths(rng, (m, 3, 1))).astype(F)
    b = open_bounds(m)
    b[:, :, 1] = np.where(rng.random((m, 3)) < 0.3, (r[:, None] * rng.uniform(0.05, 1.0, (m, 3))).astype(F), b[:, :, 1])
    out["inside"] = (r, o, d, b)
    # the sphere behind the ray: both roots negative
    r = pick(m)
    o = (_unit(rng.normal(size=(m, 3))) * (r * rng.uniform(1.2, 3.0, m))[:, None]).astype(F)
    out["behind"] = (r, o, -_aimed(rng, r, o.astype(np.float64)), open_bounds(m))
    # dist_bounds.y below the near root, between the roots, and exactly at a root's distance (+-1 ulp: the comparisons are strict)
    for fam, side in (("far_bound", 1), ("near_bound", 0)):
        r = pick(m)
        o = (_unit(rng.normal(size=(m, 3))) * (r * rng.uniform(1.2, 3.0, m))[:, None]).astype(F)
        d = _aimed(rng, r, o.astype(np.float64))
        _, _, d1, d2 = roots_f32(r, o, d)
        with np.errstate(all="ignore"):
            mid = ((d1.astype(np.float64) + d2) / 2).astype(F)
        b = open_bounds(m)
        u = rng.random((m, 3))
        ulp = rng.integers(-1, 2, (m, 3))
        choice = np.select([u < 0.2, u < 0.45, u < 0.7, u < 0.85], [d2 * F(0.5) if side else d1 * F(2.0), mid, _step(d2, ulp), _step(d1, ulp)], mid)
        b[:, :, side] = np.where(np.isfinite(choice), choice, b[:, :, side])
        out[fam] = (r, o, d, b)
    # inverted and NaN bounds on ordinary rays
    r = pick(m)
    o = (_unit(rng.normal(size=(m, 3))) * (r * rng.uniform(0.0, 3.0, m))[:, None]).astype(F)
    d = _aimed(rng, r, o.astype(np.float64), 1.5)
    b = np.empty((m, 3, 2), F)
    b[:, :, 0] = rng.uniform(0.5, 4.0, (m, 3)); b[:, :, 1] = b[:, :, 0] * rng.uniform(0.0, 1.0, (m, 3)).astype(F)      # inverted
    u = rng.random((m, 3))
    b[:, :, 0] = np.where(u < 0.2, F(np.nan), b[:, :, 0])
    b[:, :, 1] = np.where((u > 0.1) & (u < 0.3), F(np.nan), np.where((u >= 0.3) & (u < 0.4), INF, b[:, :, 1]))
    b[:, :, 0] = np.where((u >= 0.4) & (u < 0.5), F(0.0), b[:, :, 0])
    out["odd_bounds"] = (r, o, d, b)
    return out


SPECIAL_RADII = np.array([0.0, 1e-45, 1e-39, 2.0 ** -60, 2.0 ** 60, 2.0 ** 64, np.inf, np.nan], F)
SPECIAL_VALUES = np.array([0.0, -0.0, 1e-45, -1e-39, 2.0 ** -60, -(2.0 ** 60), 2.0 ** 64, 3.4028235e38, np.inf, -np.inf, np.nan], F)


def _specials(rng, seed, m):
    """Ordinary sets salted at a few percent: zero and -0 directions (all three components: a = b = 0, delta == 0, t = 0 / 0 and a
    hit), radius 0, denormal, 2^-60, 2^60, 2^64 (r * r infinite), inf and NaN in every operand."""
    r, o, d, b = (a.copy() for a in random_sets(seed, m))
    u = rng.random(m)
    r = np.where(u < 0.08, rng.choice(SPECIAL_RADII, m), r).astype(F)
    zero = rng.random((m, 3)) < 0.04
    d[zero] = rng.choice(np.array([0.0, -0.0], F), (int(zero.sum()), 3))
    for arr, share in ((o, 0.01), (d, 0.01), (b, 0.01)):
        salt = rng.random(arr.shape) < share
        arr[salt] = rng.choice(SPECIAL_VALUES, int(salt.sum()))
    return r, o, d, b


def _scaled(seed, m):
    """Whole sets scaled by 2^+-40 (radius, origin and bounds; the directions of the first half as well)."""
    r, o, d, b = (a.copy() for a in random_sets(seed, m))
    r = np.full(m, r[0], F)                                               # one radius per scale
    h = m // 2
    with np.errstate(all="ignore"):
        for sl, s in ((slice(0, h), F(2.0 ** 40)), (slice(h, m), F(2.0 ** -40))):
            r[sl] *= s; o[sl] *= s; b[sl] *= s
        d[: h // 2] *= F(2.0 ** 40); d[h: h + h // 2] *= F(2.0 ** -40)
    return r, o, d, b


def _twins(seed, m):
    """Two roots that narrow from float64 to ONE float: a sphere and an origin on the scale of 2^-90 seen along directions of length
    2^56 .. 2^62, so that both roots are below the smallest denormal or next to it (t1 == t2 == 0, or the same few denormals) and
    a hit lies at distance exactly 0, which sqrtN's caller does not flag as zero."""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** -90
    r = np.full(m, 1.5 * scale)
    o = _unit(rng.normal(size=(m, 3))) * (r * rng.uniform(0.0, 3.0, m))[:, None]
    target = _unit(rng.normal(size=(m, 3, 3))) * (r[:, None, None] * rng.uniform(0.0, 1.5, (m, 3, 1)))
    d = _unit(target - o[:, None, :]) * 2.0 ** rng.integers(56, 63, (m, 3, 1))
    b = np.empty((m, 3, 2), F)
    b[:, :, 0] = np.where(rng.random((m, 3)) < 0.7, F(0.0), EPS)
    b[:, :, 1] = INF
    return r.astype(F), o.astype(F), d.astype(F), b


ORDINARY = 64 * 64


def constructed_sets(seed):
    """(radius, org, dirs, bounds, family, step): the sets around every decision of Sphere::hit, family[i] an index into FAMILIES,
    step[i] the ulp step of the set in the tangent families (0 elsewhere).  Layout: a run of 64 x 64 ordinary sets first (waves -
    64 consecutive sets - without a tangent lane), then the two tangent families next to each other, then the rest."""
    rng = np.random.default_rng(seed)
    parts = []

    def add(fam, r, o, d, b, step=None):
        n = len(r)
        parts.append((np.asarray(r, F), np.asarray(o, F), np.asarray(d, F), np.asarray(b, F), np.full(n, FAM[fam], np.int32),
                      np.zeros(n, np.int32) if step is None else np.asarray(step, np.int32)))

    add("ordinary", *random_sets(seed + 1, ORDINARY))
    add("tangent_exact", *_family_a(rng, 32))
    rb, ob, db, bb = _family_b(rng, 4, 128)
    add("tangent_near", rb, ob, db, bb)
    for fam, sets in _chain(rng, 1024).items():
        add(fam, *sets)
    add("specials", *_specials(rng, seed + 2, 4096))
    add("scaled", *_scaled(seed + 3, 1024))
    add("twin_roots", *_twins(seed + 4, 512))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(6))


FIXTURE_SEED, FIXTURE_PER_FAMILY = 51, 120


def fixture_sets():
    """The sets of tests/golden/refbuild_sphere_edges.npz: FIXTURE_PER_FAMILY sets of every family of constructed_sets(FIXTURE_SEED),
    evenly spaced through the family, plus every step-0 set of family A among them or not.  Returns (index into the constructed
    sets, radius, org, dirs, bounds, family, step)."""
    sets = constructed_sets(FIXTURE_SEED)
    fam, step = sets[4], sets[5]
    pick = []
    for k in range(len(FAMILIES)):
        idx = np.flatnonzero(fam == k)
        pick.append(idx[np.linspace(0, len(idx) - 1, FIXTURE_PER_FAMILY).astype(np.int64)])
    pick.append(np.flatnonzero((fam == FAM["tangent_exact"]) & (step == 0)))
    index = np.unique(np.concatenate(pick))
    return (index,) + tuple(a[index] for a in sets)


def scenes_digest(radius, kind, scene_digest):
    """One digest for the scenes a list of radii needs: the SHA-256 of their digests (tests/_cases.py: scene_digest) in by_radius order."""
    import hashlib

    return hashlib.sha256("".join(scene_digest(sphere_scene(r, kind)) for r, _ in by_radius(radius)).encode()).hexdigest()


def rays_of(radius, org, dirs, bounds):
    """The sets as single rays, set-major: (radius (3n,), org (3n, 3), dirs (3n, 3), bounds (3n, 2))."""
    return (np.repeat(np.asarray(radius, F), 3), np.repeat(np.asarray(org, F), 3, axis=0), np.ascontiguousarray(dirs, F).reshape(-1, 3),
            np.ascontiguousarray(bounds, F).reshape(-1, 2))


def by_radius(radius):
    """[(radius, indices of the rays with exactly that radius)]: by bit pattern, so that -0, denormals and NaN keep groups of their own."""
    bits = np.asarray(radius, F).view(np.uint32)
    return [(bits[idx[0:1]].view(F)[0], idx) for idx in (np.flatnonzero(bits == u) for u in np.unique(bits))]


SCENE_KINDS = ("identity", "scaled")


def sphere_scene(radius, kind):
    """One sphere of the given radius: at the origin without a transform of its own ("identity"), or at (0.3, -0.2, 0.1) scaled
    (1.5, 0.5, 2) ("scaled": translation and non-uniform scale, so that Ray::transform and Trace::transform run)."""
    T = np.eye(4, dtype=F)
    if kind == "scaled":
        T = np.array([[1.5, 0, 0, 0.3], [0, 0.5, 0, -0.2], [0, 0, 2.0, 0.1], [0, 0, 0, 1]], F)
    else:
        assert kind == "identity"
    mat = {"type": 0, "a": np.full(3, 0.5, F), "b": np.zeros(3, F), "ior": 1.0}
    cam = {"iview": np.eye(4, dtype=F).reshape(16), "vfov": 90.0, "ar": 1.0}
    return {"name": f"sphere-{kind}", "materials": [mat], "camera": cam,
            "objects": [{"kind": "sphere", "radius": float(F(radius)), "T": np.ascontiguousarray(T.T.reshape(16)), "material": 0}]}


def scene_hits(make, radius, org, dirs, bounds, kind):
    """scene.hit of single rays through one-sphere scenes, one scene per distinct radius: make(scene) returns an object with
    .hit(org, dirs, bounds) -> (n, 9) (H.OraclePT, H.RefPT, a device Pathtracer).  (n, 9) float32."""
    out = np.zeros((len(radius), 9), F)
    for r, idx in by_radius(radius):
        out[idx] = make(sphere_scene(r, kind)).hit(org[idx], dirs[idx], bounds[idx])
    return out
