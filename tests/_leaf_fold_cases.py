"""Inputs for the leaf-fold tests (tests/test_pt_leaf_fold_{gpu,host}.py): waves of 64 lanes, one leaf of 1-4 triangles or a
12-triangle list per wave, per lane one origin and three rays (direction, dist_bounds) - the shape of a batch of the wave kernel
in the mesh branch of object_testN.  A set is a dict {"tris" (W, 12, 9) = p0, e1, e2 per triangle, "ntri" (W,), "org" (W, 64, 3),
"dirs" (W, 64, 3, 3), "bounds" (W, 64, 3, 2)}.  Everything is generated from a seed.

Group F is built so that no lane can be flagged (one candidate per ray at the most, far from every edge, operands inside the
window); group M so that every lane is (a point exactly on a shared edge or vertex, or two triangles under the ray); the tests
check both claims with the CPU arithmetic (tests/host_emu/leaf_fold_host.cpp) before anything else is compared."""
import numpy as np

F = np.float32
EPS = F(0.00001)
INF = F(np.inf)
LANES = 64
MARGIN = 2.0 ** -8          # group F: barycentric distance of a target from every edge of every triangle of the leaf


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _pack(tris_list, org, dirs, bounds):
    """tris_list: per wave an (n, 9) array."""
    W = len(tris_list)
    tris = np.zeros((W, 12, 9), F)
    ntri = np.zeros(W, np.uint32)
    for w, t in enumerate(tris_list):
        t = np.asarray(t, F).reshape(-1, 9)
        assert 1 <= len(t) <= 4 or len(t) == 12
        tris[w, :len(t)] = t
        ntri[w] = len(t)
    return {"tris": tris, "ntri": ntri, "org": np.asarray(org, F).reshape(W, LANES, 3), "dirs": np.asarray(dirs, F).reshape(W, LANES, 3, 3),
            "bounds": np.asarray(bounds, F).reshape(W, LANES, 3, 2)}


def concat(*sets):
    return {k: np.concatenate([s[k] for s in sets]) for k in sets[0]}


def _wide_bounds(rng, shape):
    b = np.empty(shape + (2,), F)
    b[..., 0] = np.where(rng.random(shape) < 0.5, F(0.0), EPS)
    b[..., 1] = INF
    return b


# ------------------------------------------------------------------------------------------------
# planar grids: cells (i, j) of the lattice p0 + a E1 + b E2, each cut into the triangles {corner, E1, E2} (a - i + b - j < 1) and
# {opposite corner, -E1, -E2}: every edge of every triangle lies on a line a = integer, b = integer or a + b = integer, and the
# barycentric coordinates of a point are its distances (in a, b, a + b) from those lines.
# ------------------------------------------------------------------------------------------------
_GRIDS = {1: ((1, 1), 1), 2: ((1, 1), 2), 3: ((2, 1), 3), 4: ((2, 1), 4), 12: ((3, 2), 12)}   # ntri -> (cells, triangles kept)


def _grid_tris(p0, E1, E2, ntri):
    (ni, nj), keep = _GRIDS[ntri]
    out = []
    for j in range(nj):
        for i in range(ni):
            c = p0 + i * E1 + j * E2
            out.append(np.concatenate([c, E1, E2]))
            out.append(np.concatenate([c + E1 + E2, -E1, -E2]))
    return np.asarray(out[:keep], F)


def _lattice_points(rng, n, lo, hi):
    """n points (a, b) of [lo, hi)^2 whose a, b and a + b stay MARGIN away from every integer."""
    pts = np.empty((0, 2))
    while len(pts) < n:
        c = rng.uniform(lo, hi, (4 * n, 2))
        fr = lambda x: np.abs(x - np.round(x))
        ok = (fr(c[:, 0]) >= 2 * MARGIN) & (fr(c[:, 1]) >= 2 * MARGIN) & (fr(c[:, 0] + c[:, 1]) >= 2 * MARGIN)   # (twice: the float32 rounding of the scene)
        pts = np.concatenate([pts, c[ok]])
    return pts[:n]


def _plane(rng, axis_aligned):
    if axis_aligned:                                   # a dyadic lattice in the plane z = c: exact arithmetic
        s = 2.0 ** rng.integers(-2, 2)
        p0 = np.array([rng.integers(-8, 8) / 8.0, rng.integers(-8, 8) / 8.0, rng.integers(-8, 8) / 8.0])
        return p0, np.array([s, 0.0, 0.0]), np.array([0.0, s, 0.0])
    while True:
        E1, E2 = rng.uniform(-1.0, 1.0, 3), rng.uniform(-1.0, 1.0, 3)
        l1, l2 = np.linalg.norm(E1), np.linalg.norm(E2)
        if 0.4 < l1 < 1.5 and 0.4 < l2 < 1.5 and np.linalg.norm(np.cross(E1, E2)) > 0.5 * l1 * l2:
            return rng.uniform(-1.0, 1.0, 3), E1, E2


def group_f(seed, waves_per_kind=2):
    """Every wave takes the fast path.  Per leaf size (1, 2, 3, 4, 12 coplanar triangles) and per kind of lane: targets inside a
    triangle and in the plane outside the leaf (misses), the leaf behind the origin, dist_bounds that cut the candidate from below
    and from above, and origins on the plane (axis-aligned dyadic leaves: the numerator of t is exactly zero)."""
    rng = np.random.default_rng(seed)
    tl, orgs, dirss, bnds = [], [], [], []
    for ntri in (1, 2, 3, 4, 12):
        (ni, nj), _ = _GRIDS[ntri]
        for kind in ("mixed", "behind", "cut", "on_plane"):
            for _ in range(waves_per_kind):
                p0, E1, E2 = _plane(rng, kind == "on_plane")
                p0, E1, E2 = (a.astype(F).astype(np.float64) for a in (p0, E1, E2))
                nrm = _unit(np.cross(E1, E2))
                ab = _lattice_points(rng, LANES * 3, -1.0, max(ni, nj) + 1.0).reshape(LANES, 3, 2)
                target = p0 + ab[..., :1] * E1 + ab[..., 1:] * E2
                if kind == "on_plane":
                    oab = _lattice_points(rng, LANES, -0.5, max(ni, nj) + 0.5)
                    oab = np.round(oab * 4096.0) / 4096.0                              # dyadic; moved by 2^-13 at the most
                    org = p0 + oab[:, :1] * E1 + oab[:, 1:] * E2                       # exactly representable: z = p0.z
                    d = _unit(np.stack([rng.uniform(-1, 1, (LANES, 3)), rng.uniform(-1, 1, (LANES, 3)), rng.choice([-1.0, 1.0], (LANES, 3)) * rng.uniform(0.3, 1.0, (LANES, 3))], axis=-1))
                else:
                    # origins off the plane, rays that are not grazing (|cos| >= 0.3 by construction of the offset)
                    foot = p0 + rng.uniform(-0.5, max(ni, nj) + 0.5, (LANES, 1)) * E1 + rng.uniform(-0.5, max(ni, nj) + 0.5, (LANES, 1)) * E2
                    org = foot + nrm * (rng.choice([-1.0, 1.0], (LANES, 1)) * rng.uniform(1.5, 3.0, (LANES, 1)))
                    d = _unit(target - org[:, None, :])
                    if kind == "behind":
                        d = -d
                b = _wide_bounds(rng, (LANES, 3))
                if kind == "cut":
                    dist = np.linalg.norm(target - org[:, None, :], axis=-1)
                    low = rng.random((LANES, 3)) < 0.5
                    b[..., 0] = np.where(low, dist * 1.25, 0.0)                        # dist < b0
                    b[..., 1] = np.where(low, np.inf, dist * 0.75)                     # dist > b1
                tl.append(_grid_tris(p0, E1, E2, ntri)); orgs.append(org); dirss.append(d); bnds.append(b)
    return _pack(tl, orgs, dirss, bnds)


def _square_pair(s=1.0, z=0.0):
    p0, E1, E2 = np.array([0.0, 0.0, z]), np.array([s, 0.0, 0.0]), np.array([0.0, s, 0.0])
    return _grid_tris(p0, E1, E2, 2)


def group_m(seed):
    """Every lane is flagged, so every wave falls back.  Unit-square leaves with dyadic coordinates and rays straight down, so
    that u, v, t are exact: targets on the shared diagonal (u + v = 1 in both triangles) and on the shared vertices; two
    triangles stacked in different planes with the nearer one first, second, and both at the same distance (planes that cross
    under the ray); tetrahedra (a line through the interior crosses two faces)."""
    rng = np.random.default_rng(seed)
    tl, orgs, dirss, bnds = [], [], [], []
    down = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (LANES, 3, 3))

    def add(tris, org, d):
        tl.append(tris); orgs.append(org); dirss.append(np.array(d, np.float64)); bnds.append(_wide_bounds(rng, (LANES, 3)))

    for s in (1.0, 0.25, 4.0):
        for ntri in (2, 4):                                     # the diagonal of the first cell
            tris = _grid_tris(np.zeros(3), np.array([s, 0.0, 0.0]), np.array([0.0, s, 0.0]), ntri)
            x = rng.integers(1, 255, LANES) / 256.0
            add(tris, np.stack([x * s, (1.0 - x) * s, np.full(LANES, 1.0)], axis=1), down)
        vert = np.array([[1.0, 0.0], [0.0, 1.0]])[rng.integers(0, 2, LANES)] * s      # the two shared vertices
        add(_square_pair(s), np.concatenate([vert, np.full((LANES, 1), 2.0)], axis=1), down)
    # stacked pairs: one triangle in the plane z = 0, one in z = 0.5 (nearer for an origin above), both orders
    lo = np.array([-1.0, -1.0, 0.0, 4.0, 0.0, 0.0, 0.0, 4.0, 0.0])
    hi = np.array([-1.0, -1.0, 0.5, 4.0, 0.0, 0.0, 0.0, 4.0, 0.0])
    tilt = np.array([-1.0, -1.0, -1.0, 4.0, 0.0, 4.0, 0.0, 4.0, 0.0])                  # the plane z = x: meets z = 0 in the line x = 0
    xy = rng.integers(1, 64, (LANES, 2)) / 128.0
    above = np.concatenate([xy, np.full((LANES, 1), 2.0)], axis=1)
    add(np.stack([hi, lo]), above, down)                          # nearer first
    add(np.stack([lo, hi]), above, down)                          # nearer second
    on_line = np.concatenate([np.zeros((LANES, 1)), xy[:, 1:], np.full((LANES, 1), 2.0)], axis=1)
    add(np.stack([lo, tilt]), on_line, down)                      # equal distances: Trace::min keeps the later one
    add(np.stack([tilt, lo]), on_line, down)
    for k in range(4):                                            # tetrahedra, origins outside and (k == 3) inside
        v = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * rng.uniform(0.2, 0.6) + rng.uniform(-0.3, 0.3, 3)
        v = v.astype(F).astype(np.float64)
        faces = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
        tris = np.array([np.concatenate([v[a], v[b] - v[a], v[c] - v[a]]) for a, b, c in faces])
        w = rng.dirichlet(np.full(4, 4.0), (LANES, 3))                                 # interior points, away from the faces
        inner = w @ v
        org = _unit(rng.normal(size=(LANES, 3))) * 3.0 if k < 3 else (rng.dirichlet(np.full(4, 4.0), LANES) @ v)
        add(tris, org, _unit(inner - org[:, None, :] + 1e-3))
    return _pack(tl, orgs, dirss, bnds)


def group_a(seed):
    """Operands outside the window: sets of groups F and M scaled by 2^+-41, rays parallel to the leaf's plane (det == 0), and
    NaN / inf / zero / denormal coordinates salted into ordinary sets."""
    rng = np.random.default_rng(seed)
    sets = []
    base = concat(group_f(seed + 1, 1), group_m(seed + 2))
    for e in (41.0, -41.0):
        s = {k: v.copy() for k, v in base.items()}
        with np.errstate(all="ignore"):
            s["tris"] *= F(2.0 ** e); s["org"] *= F(2.0 ** e)
            fin = np.isfinite(s["bounds"])
            s["bounds"][fin] *= F(2.0 ** e)
        sets.append(s)
    # det == 0: unit squares in z = 0, directions in the plane z = const (ray 0) and nearly so
    W = 4
    tl = [_square_pair(2.0 ** k) for k in range(W)]
    org = np.concatenate([rng.uniform(-1, 2, (W, LANES, 2)), rng.choice([0.0, 0.5, -1.0], (W, LANES, 1))], axis=2)
    d = _unit(rng.normal(size=(W, LANES, 3, 3)))
    d[:, :, 0, 2] = 0.0
    d[:, :, 1, 2] = 1e-42
    sets.append(_pack(tl, org, d, _wide_bounds(rng, (W, LANES, 3))))
    s = {k: v.copy() for k, v in base.items()}
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, 2.0 ** -60, -(2.0 ** -60), 2.0 ** 60, 2.0 ** -126, 3.4028235e38, np.inf, -np.inf, np.nan], F)
    for key, share in (("tris", 0.01), ("org", 0.01), ("dirs", 0.01), ("bounds", 0.01)):
        hit = rng.random(s[key].shape) < share
        s[key][hit] = rng.choice(special, int(hit.sum()))
    sets.append(s)
    return concat(*sets)


def random_sets(seed, waves):
    """Random leaves in and around the Cornell box - a coplanar grid, a tetrahedron, or unrelated triangles - with origins around
    them and rays aimed at and around the leaf."""
    rng = np.random.default_rng(seed)
    tl = []
    centre = np.empty((waves, 3))
    for w in range(waves):
        kind = rng.integers(0, 3)
        ntri = int(rng.choice([1, 2, 3, 4, 12]))
        if kind == 0:
            p0, E1, E2 = _plane(rng, rng.random() < 0.3)
            tris = _grid_tris(p0, E1, E2, ntri)
        elif kind == 1:
            v = rng.uniform(-0.8, 0.8, (4, 3))
            faces = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
            tris = np.array([np.concatenate([v[a], v[b] - v[a], v[c] - v[a]]) for a, b, c in faces])
        else:
            tris = np.concatenate([rng.uniform(-1.0, 1.0, (ntri, 3)), rng.uniform(-1.2, 1.2, (ntri, 6))], axis=1)
        tl.append(tris)
        centre[w] = (tris[:, 0:3] + (tris[:, 3:6] + tris[:, 6:9]) / 3.0).mean(axis=0)
    org = centre[:, None, :] + _unit(rng.normal(size=(waves, LANES, 3))) * rng.uniform(0.2, 3.0, (waves, LANES, 1))
    pick = rng.integers(0, 12, (waves, LANES, 3))
    target = np.empty((waves, LANES, 3, 3))
    for w in range(waves):
        t = np.asarray(tl[w])
        k = pick[w] % len(t)
        uv = rng.uniform(-0.3, 0.8, (LANES, 3, 2))
        target[w] = t[k, 0:3] + uv[..., :1] * t[k, 3:6] + uv[..., 1:] * t[k, 6:9]
    d = _unit(target - org[:, :, None, :])
    d[rng.random((waves, LANES, 3)) < 0.1] *= -1.0
    b = np.empty((waves, LANES, 3, 2))
    b[..., 0] = np.where(rng.random((waves, LANES, 3)) < 0.5, 0.0, EPS)
    b[..., 1] = np.where(rng.random((waves, LANES, 3)) < 0.7, np.inf, rng.uniform(0.1, 3.0, (waves, LANES, 3)))
    return _pack(tl, org, d, b)
