"""Test-side loaders for the CHECKERS (oracle/ and oracle/_ref/) and for golden fixtures.

Nothing in here is imported by the product package."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN = os.path.join(ROOT, "tests", "golden")
REF_ROOT = "/root/reference"

PRIM_DTYPE = np.dtype(
    {
        "names": ["kind", "reserved", "v", "rgba"],
        "formats": ["<u4", "<u4", ("<f8", (3,)), ("<f4", (4,))],
        "offsets": [0, 4, 8, 32],
        "itemsize": 48,
    }
)


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def build_oracle():
    subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        build_oracle()
        _oracle = ctypes.CDLL(os.path.join(ORACLE_DIR, "_build", "liboracle.so"))
    return _oracle


def have_reference():
    return os.path.isdir(REF_ROOT)


_ref_raster = None


def ref_raster():
    """The reference's own rasterizer (oracle/_ref/libref_raster.so) or None."""
    global _ref_raster
    path = os.path.join(ORACLE_DIR, "_ref", "libref_raster.so")
    if _ref_raster is None and os.path.exists(path):
        lib = ctypes.CDLL(path)
        lib.ref_raster_svg_stream.restype = ctypes.c_long
        _ref_raster = lib
    return _ref_raster


class Textures:
    """Mip chains in the flat form the checkers take: per texture the number of levels; per level (concatenated
    over the textures) width, height and byte offset into one RGBA8 blob."""

    def __init__(self, nlevels=(), level_w=(), level_h=(), level_off=(), blob=b""):
        self.nlevels = np.ascontiguousarray(nlevels, np.uint32)
        self.level_w = np.ascontiguousarray(level_w, np.uint32)
        self.level_h = np.ascontiguousarray(level_h, np.uint32)
        self.level_off = np.ascontiguousarray(level_off, np.uint64)
        self.blob = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8) if not isinstance(blob, np.ndarray) else blob, np.uint8)

    def __len__(self):
        return len(self.nlevels)

    def texture(self, t):
        """[(w, h, texels[h, w, 4])] for texture t."""
        l0 = int(self.nlevels[:t].sum())
        out = []
        for l in range(l0, l0 + int(self.nlevels[t])):
            w, h, off = int(self.level_w[l]), int(self.level_h[l]), int(self.level_off[l])
            out.append((w, h, self.blob[off:off + 4 * w * h].reshape(h, w, 4)))
        return out

    def args(self):
        return (len(self.nlevels), P(self.nlevels) if len(self.nlevels) else None, P(self.level_w) if len(self.level_w) else None,
                P(self.level_h) if len(self.level_h) else None, P(self.level_off) if len(self.level_off) else None,
                P(self.blob) if len(self.blob) else None)

    def to_npz(self):
        return dict(tex_nlevels=self.nlevels, tex_level_w=self.level_w, tex_level_h=self.level_h, tex_level_off=self.level_off,
                    tex_blob=self.blob)

    @staticmethod
    def from_npz(g):
        if "tex_nlevels" not in g:
            return Textures()
        return Textures(g["tex_nlevels"], g["tex_level_w"], g["tex_level_h"], g["tex_level_off"], g["tex_blob"])

    @staticmethod
    def from_level0(images, mips_fn):
        """images: list of uint8 [h, w, 4]; mips_fn(level0) -> [(w, h, texels)] (oracle_generate_mips / ref_generate_mips)."""
        nl, lw, lh, lo, blob = [], [], [], [], []
        off = 0
        for im in images:
            chain = mips_fn(im)
            nl.append(len(chain))
            for w, h, tx in chain:
                lw.append(w); lh.append(h); lo.append(off)
                blob.append(np.ascontiguousarray(tx, np.uint8).reshape(-1))
                off += 4 * w * h
        return Textures(nl, lw, lh, lo, np.concatenate(blob) if blob else np.zeros(0, np.uint8))


def _mips(fn, level0):
    level0 = np.ascontiguousarray(level0, np.uint8)
    h, w = level0.shape[:2]
    lw = np.zeros(16, np.uint32)
    lh = np.zeros(16, np.uint32)
    blob = np.zeros(2 * 4 * w * h + 64, np.uint8)
    n = fn(P(level0), w, h, P(lw), P(lh), P(blob), ctypes.c_uint64(len(blob)))
    assert n > 0
    out, off = [], 0
    for k in range(n):
        out.append((int(lw[k]), int(lh[k]), blob[off:off + 4 * int(lw[k]) * int(lh[k])].reshape(int(lh[k]), int(lw[k]), 4).copy()))
        off += 4 * int(lw[k]) * int(lh[k])
    return out


def oracle_generate_mips(level0):
    """Sampler2DImp::generate_mips as restated in oracle/raster_oracle.c: [(w, h, texels[h, w, 4])]."""
    return _mips(oracle().srt_oracle_generate_mips, level0)


def ref_generate_mips(level0):
    lib = ref_raster()
    lib.ref_raster_generate_mips.restype = ctypes.c_long
    return _mips(lib.ref_raster_generate_mips, level0)


def oracle_raster_frame(prims, w, h, sr, want_samples=False, textures=None):
    """Run oracle/raster_oracle.c on an ordered stream. Returns (rgba8, samples|None, counts)."""
    prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    rgba = np.zeros((h, w, 4), np.uint8)
    ss = np.zeros((h * sr, w * sr, 4), np.float32) if want_samples else None
    counts = np.zeros(4, np.uint64)
    tex = textures or Textures()
    rc = oracle().srt_oracle_raster_frame_tex(
        P(prims), ctypes.c_size_t(len(prims)), w, h, sr, *tex.args(), P(rgba), P(ss) if want_samples else None, P(counts)
    )
    assert rc == 0
    return rgba, ss, counts


def ref_raster_prims(prims, w, h, sr, want_samples=False, textures=None):
    prims = np.ascontiguousarray(prims, dtype=PRIM_DTYPE)
    rgba = np.zeros((h, w, 4), np.uint8)
    ss = np.zeros((h * sr, w * sr, 4), np.float32) if want_samples else None
    tex = textures or Textures()
    rc = ref_raster().ref_raster_prims_tex(
        P(prims), ctypes.c_size_t(len(prims)), w, h, sr, *tex.args(), P(rgba), P(ss) if want_samples else None
    )
    assert rc == 0
    return rgba, ss


def ref_svg_textures(path, w, h, sr):
    """Textures (reference mip chains) of the <image> elements of an SVG, in stream order."""
    lib = ref_raster()
    lib.ref_raster_svg_textures.restype = ctypes.c_long
    nl = np.zeros(16, np.uint32)
    lw = np.zeros(16 * 14, np.uint32)
    lh = np.zeros(16 * 14, np.uint32)
    lo = np.zeros(16 * 14, np.uint64)
    blob = np.zeros(64 << 20, np.uint8)
    n = lib.ref_raster_svg_textures(path if isinstance(path, bytes) else path.encode(), w, h, sr, 16, P(nl), P(lw), P(lh), P(lo), P(blob),
                                    ctypes.c_uint64(len(blob)))
    assert n >= 0, n
    nlev = int(nl[:n].sum())
    size = int(lo[nlev - 1] + 4 * int(lw[nlev - 1]) * int(lh[nlev - 1])) if nlev else 0
    return Textures(nl[:n], lw[:nlev], lh[:nlev], lo[:nlev], blob[:size].copy())


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_blas_against_golden(g, k, dump):
    """BVH<Triangle> of object slot k: `dump(k)` -> (boxes, links, order) compared with the fixture, which holds either the
    arrays or (meshes of more than 4096 nodes) their SHA-256 digests.  Returns True when the fixture has that mesh."""
    if f"blas{k}_boxes" in g:
        bb, bl, bo = dump(k)
        want_b, want_l, want_o = g[f"blas{k}_boxes"], g[f"blas{k}_links"], g[f"blas{k}_order"]
        assert np.array_equal(np.ascontiguousarray(bb, np.float32).view(np.uint32), np.ascontiguousarray(want_b, np.float32).view(np.uint32))
        assert np.array_equal(bl, want_l) and np.array_equal(bo[: len(want_o)], want_o)
        return True
    if f"blas{k}_sha256" in g:
        bb, bl, bo = dump(k)
        nodes, ntri = (int(v) for v in g[f"blas{k}_nodes"])
        assert len(bb) == nodes
        assert [sha(bb), sha(bl), sha(bo[:ntri])] == [str(v) for v in g[f"blas{k}_sha256"]], "BVH<Triangle> arrays differ from the reference"
        return True
    return False


def load_fullsize():
    """tests/golden/pt_fullsize.json: SHA-256 (+ a crop) of full-size epoch images from the reference build."""
    import json
    with open(os.path.join(GOLDEN, "pt_fullsize.json")) as f:
        return json.load(f)


def golden_rays(g, scene, seed, n=2048):
    """The scene.hit rays a pt_*.npz fixture was made with: random_rays, or - where the fixture says so - the same rays carried
    into the scene's world (tests/_scale_cases.py:scaled_rays)."""
    from _cases import random_rays

    if "rays" not in g:
        return random_rays(seed, n)
    assert str(g["rays"]) == "scaled_rays", str(g["rays"])
    from _scale_cases import scaled_rays

    return scaled_rays("random_rays", seed, n, scene)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# ------------------------------------------------------------------------------------------------
# Path tracer checkers
# ------------------------------------------------------------------------------------------------
_ref_pt = None


def ref_pt_lib():
    """The reference's own path tracer (oracle/_ref/libref_pt.so) or None."""
    global _ref_pt
    path = os.path.join(ORACLE_DIR, "_ref", "libref_pt.so")
    if _ref_pt is None and os.path.exists(path):
        lib = ctypes.CDLL(path)
        lib.ref_pt_create.restype = ctypes.c_void_p
        lib.ref_pt_dump_bvh.restype = ctypes.c_long
        _ref_pt = lib
    return _ref_pt


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class _SceneFeeder:
    """Feeds a scenes.py dict through an add_material/add_mesh/add_sphere/commit/set_camera API."""

    def feed(self, scene):
        for m in scene["materials"]:
            self._add_material(int(m["type"]), _f32(m["a"]), _f32(m["b"]), float(m["ior"]))
        for o in scene["objects"]:
            if o["kind"] == "mesh":
                self._add_mesh(_f32(o["pos"]), _f32(o["nrm"]), np.ascontiguousarray(o["idx"], np.uint32), _f32(o["T"]),
                               int(o["material"]), bool(o["is_light"]))
            elif o.get("light_mesh") is not None:     # emissive sphere: analytic shape + its triangle approximation as the light
                lm = o["light_mesh"]
                self._add_sphere_light(float(o["radius"]), _f32(o["T"]), int(o["material"]), _f32(lm["pos"]), _f32(lm["nrm"]),
                                       np.ascontiguousarray(lm["idx"], np.uint32))
            else:
                self._add_sphere(float(o["radius"]), _f32(o["T"]), int(o["material"]))
        if scene.get("env"):                  # {"type": 1 sphere | 2 hemisphere, "radiance"} or {"type": 3, "image": float32 [h, w, 3]}
            if int(scene["env"]["type"]) == 3:
                self._set_env_map(_f32(scene["env"]["image"]))
            else:
                self._set_env(int(scene["env"]["type"]), _f32(scene["env"]["radiance"]))
        for l in scene.get("lights", []):   # delta lights: {"type": 0 directional | 1 point | 2 spot, "radiance", "angle_bounds", "T"}
            self._add_light(int(l["type"]), _f32(l["radiance"]), _f32(l.get("angle_bounds", (0.0, 0.0))), _f32(l["T"]))
        self._commit()
        c = scene["camera"]
        self._set_camera(_f32(c["iview"]), float(c["vfov"]), float(c["ar"]))


class RefPT(_SceneFeeder):
    """PT::Pathtracer of the reference, driven through oracle/ref_harness/pt_ref.cpp."""

    def __init__(self, scene, w, h, max_depth=8, use_bvh=True):
        self.lib = ref_pt_lib()
        assert self.lib is not None
        self.w, self.h = w, h
        self.h_ = ctypes.c_void_p(self.lib.ref_pt_create(w, h, max_depth, int(use_bvh)))
        self.feed(scene)

    def _add_material(self, t, a, b, ior):
        assert self.lib.ref_pt_add_material(self.h_, t, P(a), P(b), ctypes.c_float(ior)) >= 0

    def _add_mesh(self, pos, nrm, idx, T, material, is_light):
        assert self.lib.ref_pt_add_mesh(self.h_, P(pos), P(nrm), len(pos), P(idx), len(idx), P(T), material, int(is_light)) == 0

    def _add_sphere(self, radius, T, material):
        assert self.lib.ref_pt_add_sphere(self.h_, ctypes.c_float(radius), P(T), material) == 0

    def _add_sphere_light(self, radius, T, material, pos, nrm, idx):
        assert self.lib.ref_pt_add_sphere_light(self.h_, ctypes.c_float(radius), P(T), material, P(pos), P(nrm), len(pos), P(idx), len(idx)) == 0

    def _add_light(self, type_, radiance, angle_bounds, T):
        assert self.lib.ref_pt_add_light(self.h_, type_, P(radiance), P(angle_bounds), P(T)) == 0

    def _set_env(self, type_, radiance):
        assert self.lib.ref_pt_set_env_light(self.h_, type_, P(radiance)) == 0

    def _set_env_map(self, image):
        assert self.lib.ref_pt_set_env_map(self.h_, image.shape[1], image.shape[0], P(image)) == 0

    def _commit(self):
        assert self.lib.ref_pt_commit(self.h_) == 0

    def _set_camera(self, iview, vfov, ar):
        assert self.lib.ref_pt_set_camera(self.h_, P(iview), ctypes.c_float(vfov), ctypes.c_float(ar)) == 0

    def trace_samples(self, seed, xs, ys, ss):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        out = np.zeros((len(xs), 3), np.float32)
        draws = np.zeros(len(xs), np.uint32)
        assert self.lib.ref_pt_trace_samples(self.h_, ctypes.c_uint64(seed), P(xs), P(ys), P(ss), ctypes.c_size_t(len(xs)), P(out), P(draws)) == 0
        return out, draws

    def epoch(self, seed, sample_base, samples):
        img = np.zeros((self.h, self.w, 3), np.float32)
        assert self.lib.ref_pt_epoch(self.h_, ctypes.c_uint64(seed), sample_base, samples, P(img)) == 0
        return img

    def epoch_rows(self, seed, sample_base, samples, row0, row1, img):
        """Rows [row0, row1) of one epoch into img (h, w, 3); safe to call from several threads at once."""
        assert self.lib.ref_pt_epoch_rows(self.h_, ctypes.c_uint64(seed), sample_base, samples, row0, row1, P(img)) == 0

    def epoch_log(self, seed, sample_base, samples, cap=1 << 16):
        """One epoch with the harness's sink behind Gui::Widget_Render::log_ray: (image, log) where log is [n, 13] =
        {ray.point, ray.dir, t, pixel, sample, ordinal of the call within its sample, color} per log_ray call, in call order."""
        img = np.zeros((self.h, self.w, 3), np.float32)
        log = np.zeros((cap, 13), np.float32)
        n = ctypes.c_size_t()
        assert self.lib.ref_pt_epoch_rows_log(self.h_, ctypes.c_uint64(seed), sample_base, samples, 0, self.h, P(img), P(log),
                                              ctypes.c_size_t(cap), ctypes.byref(n)) == 0
        assert n.value <= cap, "ray log overflow: raise cap"
        return img, log[: n.value].copy()

    def hit(self, org, dirs, bounds):
        org, dirs, bounds = _f32(org), _f32(dirs), _f32(bounds)
        out = np.zeros((len(org), 9), np.float32)
        assert self.lib.ref_pt_hit(self.h_, P(org), P(dirs), P(bounds), ctypes.c_size_t(len(org)), P(out)) == 0
        return out

    def particles_update(self, pos, vel, age, dt, radius):
        """Scene_Particles::Particle::update of the reference for every particle: (pos, vel, age, alive)."""
        pos, vel, age = _f32(pos).copy(), _f32(vel).copy(), _f32(age).copy()
        alive = np.zeros(len(age), np.uint8)
        assert self.lib.ref_pt_particles_update(self.h_, P(pos), P(vel), P(age), ctypes.c_size_t(len(age)), ctypes.c_float(dt),
                                                ctypes.c_float(radius), P(alive)) == 0
        return pos, vel, age, alive

    def dump_bvh(self, which, cap=1 << 22):
        boxes = np.zeros((cap, 6), np.float32)
        links = np.zeros((cap, 4), np.uint32)
        order = np.zeros(cap * 4, np.uint32)
        n = self.lib.ref_pt_dump_bvh(self.h_, which, P(boxes), P(links), ctypes.c_size_t(cap), P(order))
        if n < 0:
            return None
        return boxes[:n].copy(), links[:n].copy(), order


class OraclePT(_SceneFeeder):
    """oracle/pt_oracle.c driven through ctypes. math_mode 0 = libm (pins against the reference
    build), 1 = SRT-MATH v1 (what the HIP kernel computes)."""

    def __init__(self, scene, w, h, max_depth=8, use_bvh=True, math_mode=1):
        self.lib = oracle()
        self.lib.srt_oracle_pt_create.restype = ctypes.c_void_p
        self.lib.srt_oracle_pt_dump_bvh.restype = ctypes.c_long
        self.w, self.h = w, h
        self.h_ = ctypes.c_void_p(self.lib.srt_oracle_pt_create())
        self._use_bvh = use_bvh
        assert self.lib.srt_oracle_pt_set_params(self.h_, w, h, max_depth) == 0
        self.lib.srt_oracle_pt_set_math(self.h_, math_mode)
        self.feed(scene)

    def _add_material(self, t, a, b, ior):
        assert self.lib.srt_oracle_pt_add_material(self.h_, t, P(a), P(b), ctypes.c_float(ior)) >= 0

    def _add_mesh(self, pos, nrm, idx, T, material, is_light):
        assert self.lib.srt_oracle_pt_add_mesh(self.h_, P(pos), P(nrm), len(pos), P(idx), len(idx), P(T), material, int(is_light)) == 0

    def _add_sphere(self, radius, T, material):
        assert self.lib.srt_oracle_pt_add_sphere(self.h_, ctypes.c_float(radius), P(T), material) == 0

    def _add_sphere_light(self, radius, T, material, pos, nrm, idx):
        assert self.lib.srt_oracle_pt_add_sphere_light(self.h_, ctypes.c_float(radius), P(T), material, P(pos), P(nrm), len(pos), P(idx), len(idx)) == 0

    def _add_light(self, type_, radiance, angle_bounds, T):
        assert self.lib.srt_oracle_pt_add_light(self.h_, type_, P(radiance), P(angle_bounds), P(T)) == 0

    def _set_env(self, type_, radiance):
        assert self.lib.srt_oracle_pt_set_env_light(self.h_, type_, P(radiance)) == 0

    def _set_env_map(self, image):
        assert self.lib.srt_oracle_pt_set_env_map(self.h_, image.shape[1], image.shape[0], P(image)) == 0

    def _commit(self):
        rc = self.lib.srt_oracle_pt_commit(self.h_, int(self._use_bvh))
        assert rc == 0, f"oracle commit failed ({rc})"

    def _set_camera(self, iview, vfov, ar):
        assert self.lib.srt_oracle_pt_set_camera(self.h_, P(iview), ctypes.c_float(vfov), ctypes.c_float(ar)) == 0

    def set_math(self, mode):
        self.lib.srt_oracle_pt_set_math(self.h_, mode)

    def trace_samples(self, seed, xs, ys, ss, counters=None):
        xs, ys, ss = (np.ascontiguousarray(a, np.uint32) for a in (xs, ys, ss))
        out = np.zeros((len(xs), 3), np.float32)
        draws = np.zeros(len(xs), np.uint32)
        rays = np.zeros(len(xs), np.uint32)
        rc = self.lib.srt_oracle_pt_trace_samples(self.h_, ctypes.c_uint64(seed), P(xs), P(ys), P(ss), ctypes.c_size_t(len(xs)),
                                                  P(out), P(draws), P(rays), P(counters) if counters is not None else None)
        assert rc == 0
        return out, draws, rays

    def epoch(self, seed, sample_base, samples, y0=0, y1=None, img=None, counters=None):
        if img is None:
            img = np.zeros((self.h, self.w, 3), np.float32)
        y1 = self.h if y1 is None else y1
        rc = self.lib.srt_oracle_pt_epoch_rows(self.h_, ctypes.c_uint64(seed), sample_base, samples, y0, y1, P(img),
                                               P(counters) if counters is not None else None)
        assert rc == 0
        return img

    def epoch_log(self, seed, sample_base, samples, cap=1 << 16):
        """One epoch and the rays it hands to Pathtracer::log_ray: (image, log [n, 10] = {point, dir, t, pixel, sample, bounce})."""
        img = np.zeros((self.h, self.w, 3), np.float32)
        log = np.zeros((cap, 10), np.float32)
        n = ctypes.c_size_t()
        assert self.lib.srt_oracle_pt_epoch_rows_log(self.h_, ctypes.c_uint64(seed), sample_base, samples, 0, self.h, P(img), P(log),
                                                     ctypes.c_size_t(cap), ctypes.byref(n)) == 0
        assert n.value <= cap, "ray log overflow: raise cap"
        return img, log[: n.value].copy()

    def hit(self, org, dirs, bounds):
        org, dirs, bounds = _f32(org), _f32(dirs), _f32(bounds)
        out = np.zeros((len(org), 9), np.float32)
        assert self.lib.srt_oracle_pt_hit(self.h_, P(org), P(dirs), P(bounds), ctypes.c_size_t(len(org)), P(out)) == 0
        return out

    def particles_update(self, pos, vel, age, dt, radius, max_iter=4096):
        pos, vel, age = _f32(pos).copy(), _f32(vel).copy(), _f32(age).copy()
        alive = np.zeros(len(age), np.uint8)
        assert self.lib.srt_oracle_pt_particles_update(self.h_, P(pos), P(vel), P(age), ctypes.c_size_t(len(age)), ctypes.c_float(dt),
                                                       ctypes.c_float(radius), P(alive), ctypes.c_uint32(max_iter)) == 0
        return pos, vel, age, alive

    def dump_bvh(self, which, cap=1 << 22):
        boxes = np.zeros((cap, 6), np.float32)
        links = np.zeros((cap, 4), np.uint32)
        order = np.zeros(cap * 4, np.uint32)
        n = self.lib.srt_oracle_pt_dump_bvh(self.h_, which, P(boxes), P(links), ctypes.c_size_t(cap), P(order))
        if n < 0:
            return None
        return boxes[:n].copy(), links[:n].copy(), order


COUNTER_NAMES = ("rays", "box_tests", "objects_entered", "tri_tests", "sphere_tests", "tlas_nodes", "blas_nodes", "light_tri_tests")


def oracle_accumulate(acc, epoch, k):
    oracle().srt_oracle_pt_accumulate(P(acc), P(epoch), ctypes.c_size_t(acc.size), k)
    return acc


def oracle_epoch_mt(o, seed, base, n, rows=None, threads=16):
    """OraclePT.epoch split by rows over at most `threads` host threads (srt_oracle_pt_epoch_rows is safe for disjoint rows);
    rows = (y0, y1) computes only those rows, the others stay zero."""
    from concurrent.futures import ThreadPoolExecutor

    y0, y1 = rows or (0, o.h)
    img = np.zeros((o.h, o.w, 3), np.float32)
    step = max(1, -(-(y1 - y0) // threads))
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(lambda a: o.epoch(seed, base, n, a, min(a + step, y1), img), range(y0, y1, step)))
    return img


def oracle_running_means(epoch_of, total, spe, first_k=0, acc=None, shape=None):
    """The reference's running mean (rays/pathtracer.cpp:195-231) of a render of `total` samples in epochs of `spe`:
    [accumulator after 0, 1, 2, ... completed epochs], the epochs given by epoch_of(offset, count)."""
    acc = np.zeros(shape, np.float32) if acc is None else acc.copy()
    out = [acc.copy()]
    k = first_k
    for s in range(0, total, spe):
        k += 1
        oracle_accumulate(acc, epoch_of(s, min(spe, total - s)), k)
        out.append(acc.copy())
    return out


def epochs_through(through, total, spe):
    """Epochs of a render completed once `through` of its `total` samples are folded (the last one may be short)."""
    return -(-total // spe) if through == total else through // spe


# ------------------------------------------------------------------------------------------------
# Host emulation of the device traversal headers (tests/host_emu): pt_device.h / pt_trace.h / pt_flat.h compiled
# with g++ (same -ffp-contract=off) and run one lane at a time.  Checks the traversal LOGIC on the CPU; the HIP
# build of the same source is what the GPU tests check.
# ------------------------------------------------------------------------------------------------
CSRC = os.path.join(ROOT, "soft-rendering-toolsets_amd", "csrc")
HOST_EMU = os.path.join(ROOT, "tests", "host_emu")
BUILD_DIR = os.path.join(ORACLE_DIR, "_build")
# The scene layer (host-only C++ of the product): the one place in tests/ and tools/ that names its files.
SCENE_LAYER_SRCS = [os.path.join(CSRC, f) for f in ("pt_scene.cpp",)]
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _compile(out, srcs, flags, *, scene_layer, extra, device_headers, keep):
    """The one compiler line of the tests.  srcs: paths, or names under tests/host_emu.  `extra` stands in front of the common include
    directories (so a site's own -I wins) except its -l items, which go behind the sources.  keep: build only if `out` is missing or
    older than a file the compiler read last time (its list, and the command, are kept in out + ".d")."""
    srcs = [os.path.join(HOST_EMU, s) for s in srcs] + (SCENE_LAYER_SRCS if scene_layer else [])
    incs = ["-I" + HOST_EMU, "-I" + CSRC] if device_headers else []
    cmd = ["g++", *flags, "-std=c++17", "-ffp-contract=off", *(e for e in extra if not e.startswith("-l")), *incs,
           "-I" + os.path.join(ROOT, "include"), *srcs, *(e for e in extra if e.startswith("-l"))]
    if not keep:
        subprocess.run(cmd + ["-o", out], check=True)
        return out
    import json

    record = out + ".d"
    rel = lambda p: os.path.relpath(p, ROOT)          # (the tree may be copied elsewhere together with what was built in it)
    try:
        with open(record) as f:
            old = json.load(f)
        fresh = old["cmd"] == [c.replace(ROOT, "@") for c in cmd] and \
            all(os.path.getmtime(os.path.join(ROOT, d)) <= os.path.getmtime(out) for d in old["deps"])
    except (OSError, ValueError, KeyError):
        fresh = False
    if not fresh:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(cmd + ["-o", out], check=True)
        rules = subprocess.run([c for c in cmd if c != "-shared"] + ["-MM"], check=True, capture_output=True, text=True).stdout
        deps = sorted({rel(t) for t in rules.replace("\\\n", " ").split() if not t.endswith(":")})
        with open(record, "w") as f:
            json.dump({"cmd": [c.replace(ROOT, "@") for c in cmd], "deps": deps}, f)
    return out


def build_host_lib(name, srcs, *, scene_layer=False, extra=(), device_headers=True, program=False):
    """oracle/_build/lib<name>.so (program: oracle/_build/<name>, a program with its own main) from srcs, built if missing or stale:
    -O2 -ffp-contract=off as the product build, tests/host_emu (the stand-in for the HIP runtime) and csrc/ (the device headers) on
    the include path unless device_headers is off, the scene layer linked in where scene_layer is set."""
    out = os.path.join(BUILD_DIR, name if program else f"lib{name}.so")
    return _compile(out, srcs, ("-O2",) if program else ("-O2", "-fPIC", "-shared"), scene_layer=scene_layer, extra=extra,
                    device_headers=device_headers, keep=True)


def run_sanitized_main(tmp_path, main_cpp, *, scene_layer=True, extra_srcs=(), args=(), expect=None, extra=(), flags=SANITIZE,
                       device_headers=True):
    """A stand-alone program (its own main, nothing loaded into Python) built into tmp_path with AddressSanitizer and
    UndefinedBehaviorSanitizer and run once as its own process: exit status 0 and the line `expect` ("<name>: ok" by default, <name>
    being main_cpp without "_main.cpp").  Returns what it printed."""
    name = os.path.basename(main_cpp)[: -len(".cpp")]
    name = name[: -len("_main")] if name.endswith("_main") else name
    exe = os.path.join(str(tmp_path), name)
    if not os.path.exists(exe):                       # (a test that runs its program on several inputs builds it once)
        _compile(exe, [main_cpp, *extra_srcs], flags, scene_layer=scene_layer, extra=extra, device_headers=device_headers, keep=False)
    r = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert (expect or name + ": ok") in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


_emu = None


def host_emu():
    global _emu
    if _emu is None:
        _emu = ctypes.CDLL(build_host_lib("flat_host", ["flat_host.cpp"], scene_layer=True))
        _emu.emu_create.restype = ctypes.c_void_p
    return _emu


class EmuPT(_SceneFeeder):
    """scene.hit of the device headers on the CPU: nested form (scene_hit) and flattened walk (flat_trace3)."""

    def __init__(self, scene, use_bvh=True):
        self.lib = host_emu()
        self.h_ = ctypes.c_void_p(self.lib.emu_create())
        self.use_bvh = use_bvh
        self.feed(scene)

    def _add_material(self, t, a, b, ior):
        assert self.lib.emu_add_material(self.h_, t, P(a), P(b), ctypes.c_float(ior)) >= 0

    def _add_mesh(self, pos, nrm, idx, T, material, is_light):
        assert self.lib.emu_add_mesh(self.h_, P(pos), P(nrm), len(pos), P(idx), len(idx), P(T), material, int(is_light)) == 0

    def _add_sphere(self, radius, T, material):
        assert self.lib.emu_add_sphere(self.h_, ctypes.c_float(radius), P(T), material) == 0

    def _add_sphere_light(self, radius, T, material, pos, nrm, idx):
        self._add_sphere(radius, T, material)

    def _add_light(self, type_, radiance, angle_bounds, T):
        pass   # scene.hit only

    def _set_env(self, type_, radiance):
        pass

    def _set_env_map(self, image):
        pass

    def _commit(self):
        assert self.lib.emu_commit(self.h_, int(self.use_bvh)) == 0

    def _set_camera(self, iview, vfov, ar):
        pass

    def hit(self, org, dirs, bounds, slot=0):
        """(nested, flat): uint32 arrays [n, 4] = {hit, distance bits, object slot, triangle}."""
        org, dirs, bounds = _f32(org), _f32(dirs), _f32(bounds)
        a = np.zeros((len(org), 4), np.uint32)
        b = np.zeros((len(org), 4), np.uint32)
        assert self.lib.emu_hit(self.h_, P(org), P(dirs), P(bounds), ctypes.c_size_t(len(org)), slot, P(a), P(b)) == 0
        return a, b

    def hit3(self, org, dirs3, bounds):
        """Three rays per batch sharing an origin; [n, 3, 4]."""
        org, dirs3, bounds = _f32(org), _f32(dirs3), _f32(bounds)
        out = np.zeros((len(org), 3, 4), np.uint32)
        assert self.lib.emu_hit3(self.h_, P(org), P(dirs3), P(bounds), ctypes.c_size_t(len(org)), P(out)) == 0
        return out

    def hit_depth(self, org, dirs, bounds):
        """The flattened walk over a stack that counts: (deepest frame index each ray touched, -1 for none; its result as `hit`
        reports it; (max_tlas_depth, max_blas_depth) of the host build)."""
        org, dirs, bounds = _f32(org), _f32(dirs), _f32(bounds)
        deepest = np.zeros(len(org), np.int32)
        flat = np.zeros((len(org), 4), np.uint32)
        tree = np.zeros(2, np.uint32)
        assert self.lib.emu_hit_depth(self.h_, P(org), P(dirs), P(bounds), ctypes.c_size_t(len(org)), P(deepest), P(flat), P(tree)) == 0
        return deepest, flat, (int(tree[0]), int(tree[1]))

    def close(self):
        self.lib.emu_destroy(self.h_)


_core_driver = None


def pt_core_driver():
    """C surface over srt_host::RenderCore (the Scene-independent part of the drop-in PT::Pathtracer), linked to the product
    library: tests/host_emu/pt_core_driver.cpp + soft-rendering-toolsets_amd/host/pathtracer_core.cpp, built with g++."""
    global _core_driver
    if _core_driver is None:
        host = os.path.join(ROOT, "soft-rendering-toolsets_amd", "host")
        lib = os.path.join(ROOT, "soft-rendering-toolsets_amd", "lib")
        out = build_host_lib("pt_core_driver", ["pt_core_driver.cpp", os.path.join(host, "pathtracer_core.cpp")], device_headers=False,
                             extra=("-D__HIP_PLATFORM_AMD__", "-I" + host, "-I/opt/rocm/include", "-L" + lib, "-lsrt_hip", "-L/opt/rocm/lib",
                                    "-lamdhip64", "-lpthread", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"))
        _core_driver = ctypes.CDLL(out)
        _core_driver.core_create.restype = ctypes.c_void_p
        _core_driver.core_context.restype = ctypes.c_void_p
        _core_driver.core_progress.restype = ctypes.c_float
        _core_driver.core_epochs_accumulated.restype = ctypes.c_size_t
    return _core_driver


def oracle_tonemap(rgb, exposure):
    """HDR_Image::tonemap_to as restated by oracle/pt_oracle.c: (h, w, 3) float32 -> (h, w, 4) uint8."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    out = np.zeros((h, w, 4), np.uint8)
    oracle().srt_oracle_tonemap(ctypes.c_uint32(w), ctypes.c_uint32(h), P(rgb), ctypes.c_float(exposure), P(out))
    return out


def ref_tonemap(rgb, exposure):
    """The reference's HDR_Image::tonemap_to (oracle/_ref/libref_pt.so); None when the reference build is absent."""
    lib = ref_pt_lib()
    if lib is None:
        return None
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    out = np.zeros((h, w, 4), np.uint8)
    lib.ref_pt_tonemap(ctypes.c_uint32(w), ctypes.c_uint32(h), P(rgb), ctypes.c_float(exposure), P(out))
    return out


def parse_scene_dump(blob):
    """oracle/integration/harness/pt_full.cpp:dump_scene -> the scene description dict of soft-rendering-toolsets_amd/scenes.py."""
    import struct

    at = [0]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, blob, at[0])
        at[0] += struct.calcsize("<" + fmt)
        return v

    def mesh():
        nv, ni = take("II")
        v = np.frombuffer(blob, np.float32, nv * 6, at[0]).reshape(nv, 6).copy(); at[0] += nv * 24
        i = np.frombuffer(blob, np.uint32, ni, at[0]).copy(); at[0] += ni * 4
        return {"pos": v[:, :3].copy(), "nrm": v[:, 3:].copy(), "idx": i}

    mats, objs, lights, env = [], [], [], None
    while True:
        (kind,) = take("I")
        if kind == 0:
            break
        if kind in (1, 2, 5):
            (mtype,) = take("I"); a = take("3f"); b = take("3f"); (ior,) = take("f"); (is_light,) = take("I")
            T = np.array(take("16f"), np.float32)
            mats.append({"type": mtype, "a": np.array(a, np.float32), "b": np.array(b, np.float32), "ior": ior})
            if kind == 2:
                (radius,) = take("f")
                o = {"kind": "sphere", "radius": radius, "T": T, "material": len(mats) - 1}
                if is_light:
                    o["light_mesh"] = mesh()
                objs.append(o)
            else:
                m = mesh()
                objs.append({"kind": "mesh", "pos": m["pos"], "nrm": m["nrm"], "idx": m["idx"], "T": T, "material": len(mats) - 1, "is_light": bool(is_light)})
        elif kind == 3:
            (ltype,) = take("I"); rad = take("3f"); ab = take("2f"); T = np.array(take("16f"), np.float32)
            lights.append({"type": ltype, "radiance": np.array(rad, np.float32), "angle_bounds": np.array(ab, np.float32), "T": T})
        elif kind == 4:
            (etype,) = take("I"); rad = take("3f")
            env = {"type": etype, "radiance": np.array(rad, np.float32)}
        else:
            raise AssertionError(f"unknown record {kind}")
    d = {"name": "pt_full", "materials": mats, "objects": objs, "lights": lights}
    if env:
        d["env"] = env
    return d
