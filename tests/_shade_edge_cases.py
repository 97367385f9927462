"""Scenes that put ONE shading parameter at the edge of its range: glass iors around and far from 1, spot cones that are empty,
inverted or wider than a circle, delta-light counts around the wave kernel's batches of three, black / negative / huge albedos
and emissions, environment maps of one texel row or column, and materials on both sides of the elision gate's 1e15 bound.

Every case is a copy of a named scene of _cases.pt_scene with one parameter changed; same name -> same arrays.  CASES lists them,
BASE names the scene each one was cut from, FAMILIES groups them as the GPU tests run them.  ORACLE_ONLY are the cases the
reference build aborts on (bsdf.h:102, "You scattered an emissive BSDF!": a light material whose emission has no positive luma
is shaded as a BSDF): they are compared with the oracle alone and are not in tests/golden/refbuild_shade_edges.npz."""
import numpy as np

from _cases import pt_sample_list, pt_scene

F = np.float32
W, H, DEPTH, SEED, NSAMPLES = 24, 16, 8, 5, 600           # what the fixture and the host tests trace
MAX_SAMPLE = 1 << 12

GLASS, SPHERE_OBJECT, LIGHT_MATERIAL = 6, 6, 7            # material / object slots of scenes.cornell_box
SPOT = 1                                                  # index of the spot light in cbox_deltalights
NEXT_ABOVE_1E15 = float(np.nextafter(F(1e15), F(np.inf)))


def _albedo_pair_at_the_gate():
    """The elision gate (elision_provable, csrc/pt.hip) reads the records the kernels read, and a Lambertian's holds albedo / PI_F
    (BSDF_Lambertian's constructor, rays/bsdf.h:26; build_scene and srt_pt_update_materials divide in float32).  So an albedo of
    1e15 is far inside the gate; the pair that straddles it is the largest float32 albedo whose record is still <= 1e15 and the
    next float above it."""
    pi = F(3.14159265358979323846264338327950288)
    x = F(1e15) * pi
    while F(x / pi) <= F(1e15):
        x = np.nextafter(x, F(np.inf))
    while F(x / pi) > F(1e15):
        x = np.nextafter(x, F(0))
    above = np.nextafter(x, F(np.inf))
    assert F(x / pi) <= F(1e15) < F(above / pi)
    return float(x), float(above)


GATE_ALBEDO_AT, GATE_ALBEDO_ABOVE = _albedo_pair_at_the_gate()


def sample_list():
    return pt_sample_list(77, W, H, NSAMPLES, max_sample=MAX_SAMPLE)


def _f(v):
    return np.asarray(v, F)


def _glass(base, **change):
    def make():
        s = pt_scene(base)
        s["materials"][GLASS] = dict(s["materials"][GLASS], **{k: (float(v) if k == "ior" else _f(v)) for k, v in change.items()})
        return s
    return base, make


def _camera_in_glass(off_centre=0.0, base="cbox", **change):
    """The camera inside the glass object of `base`, `off_centre` radii from its centre along +x.  From the centre of the sphere
    every ray meets it along its normal (cos_i = -1: no total internal reflection, whatever the ior); from 0.8 radii most of
    them meet it beyond the critical angle of ior 1.5 (sin > 1 / 1.5)."""
    def make():
        s = _glass(base, **change)[1]()
        ball = s["objects"][SPHERE_OBJECT]
        iview = _f(s["camera"]["iview"]).copy()
        iview[12:15] = _f(ball["T"])[12:15]                              # column-major: the translation column
        iview[12] += F(off_centre * ball.get("radius", 0.0))
        s["camera"] = dict(s["camera"], iview=iview)
        return s
    return make


def _spot(bounds=None):
    """cbox_deltalights with its spot light turned over.  Spot_Light::sample measures the angle from the light's +y axis, and the
    scene's spot, 0.1 below the ceiling, has that axis pointing up: its 35 / 70 degree cone lights a patch of the ceiling no
    sample of the list sees, so no narrower cone would change a sample.  Negating the y and z columns of its pose (a half turn
    about x, exact in float32) points the cone into the box; the spot cases and their base scene both use this pose and differ in
    angle_bounds alone."""
    def make():
        s = pt_scene("cbox_deltalights")
        T = _f(s["lights"][SPOT]["T"]).copy()
        T[4:12] *= F(-1.0)
        s["lights"][SPOT] = dict(s["lights"][SPOT], T=T, **({} if bounds is None else {"angle_bounds": _f(bounds)}))
        return s
    return "spot_down", make


def _light_count(n):
    def make():
        s = pt_scene("cbox_deltalights")
        four, lights = s["lights"], []
        for i in range(n):
            l = dict(four[i % 4])
            if i >= 4:                                                   # an extra light: a copy moved by (0.07 k, 0, -0.05 k)
                k = i - 3
                T = _f(l["T"]).copy()
                T[12:15] += _f([0.07 * k, 0.0, -0.05 * k])
                l["T"] = T
            lights.append(l)
        if n == 6:                                                       # one in each batch of three
            lights[3] = dict(lights[3], radiance=_f([0.0, 0.0, 0.0]))
            lights[5] = dict(lights[5], radiance=_f([-0.3, 0.2, -0.1]))
        s["lights"] = lights
        return s
    return "cbox_deltalights", make


def _albedo(value):
    def make():
        s = pt_scene("cbox_deltalights")
        s["materials"] = [dict(m, a=_f(value)) if int(m["type"]) == 0 else m for m in s["materials"]]
        return s
    return "cbox_deltalights", make


def _emission(value):
    def make():
        s = pt_scene("cbox")
        s["materials"][LIGHT_MATERIAL] = dict(s["materials"][LIGHT_MATERIAL], a=_f(value))
        return s
    return "cbox", make


def _env_map(h, w, seed, scale=1.0, negative=False):
    def make():
        s = pt_scene("cbox_envmap")
        img = (np.random.default_rng(seed).uniform(0.0, 1.5, (h, w, 3)).astype(F) * F(scale)).astype(F)
        if negative:
            img[1, 2] = _f([-2.0, -1.0, -0.5])
        s["env"] = {"type": 3, "image": np.ascontiguousarray(img, F)}
        return s
    return "cbox_envmap", make


def _env_radiance(base, value):
    def make():
        s = pt_scene(base)
        s["env"] = dict(s["env"], radiance=_f(value))
        return s
    return base, make


def _gate(material, channel, value):
    def make():
        s = pt_scene("cbox_lambertian")
        a = _f(s["materials"][material]["a"]).copy()
        a[channel] = F(value)
        s["materials"][material] = dict(s["materials"][material], a=a)
        return s
    return "cbox_lambertian", make


GATE_WALL, GATE_CHANNEL = 4, 1        # the floor's green channel; the light's red channel
_TABLE = {}
FAMILIES = {}


def _add(family, name, entry):
    assert name not in _TABLE
    _TABLE[name] = entry
    FAMILIES.setdefault(family, []).append(name)


# (the NaN parameters - this ior, and albedo_nan below - are here because the reference build and the oracle agree on them)
for _ior in ("1.0", "1.0000001", "0.5", "1e-3", "0.0", "-1.5", "1e6", "3e38", "nan"):
    _add("glass", f"glass_ior_{_ior}", _glass("cbox", ior=float(_ior)))
_add("glass", "glass_transmittance_0", _glass("cbox", a=(0, 0, 0)))
_add("glass", "glass_camera_inside", ("cbox", _camera_in_glass()))
_add("glass", "glass_camera_tir", ("cbox", _camera_in_glass(0.8)))
for _ior in ("0.5", "1.0"):
    _add("glass_mesh", f"glass_mesh_ior_{_ior}", _glass("cbox_blob512_glass", ior=float(_ior)))
# on the sphere the reflectance reaches 1 % of the samples: only the Fresnel coin (4 % at ior 1.5) reflects on the way in, and a
# ray reflected inside a sphere meets it at the same angle for ever.  The blob's facets let internally reflected rays out again,
# and with the camera inside the blob every first hit is one that can reflect internally.
_add("glass_mesh", "glass_reflectance_0", ("blob_camera_inside", _camera_in_glass(base="cbox_blob512_glass", b=(0, 0, 0))))
for _b in ((40, 40), (70, 35), (0, 0), (0, 360), (400, 500), (-10, 20), (0, 1e-30), (179.99, 180), (360, 360)):
    _add("spot", f"spot_{_b[0]:g}_{_b[1]:g}", _spot(_b))
for _n in (1, 2, 3, 6, 7):
    _add("light_count", f"lights_{_n}", _light_count(_n))
# (negative_luma: point_lighting skips a light when luma(att) == 0, not when it is negative - (-0.5, 0.2, 0.1) has a positive luma)
for _name, _a in (("0", (0, 0, 0)), ("green", (0, 0.5, 0)), ("negative", (-0.5, 0.2, 0.1)), ("negative_luma", (-0.5, 0.1, 0.1)),
                  ("1e20", (1e20, 1e20, 1e20)), ("nan", (float("nan"), 0.5, 0.5))):
    _add("albedo", f"albedo_{_name}", _albedo(_a))
for _name, _e in (("2e38", (2e38, 2e38, 2e38)), ("denormal", (1e-40, 0, 0)), ("mixed_sign", (-5, 10, -5)), ("0", (0, 0, 0)),
                  ("negative", (-1, -1, -1))):
    _add("emission", f"emission_{_name}", _emission(_e))
for _k, (_h, _w) in enumerate(((1, 1), (1, 5), (5, 1), (1, 2), (2, 1), (2, 2))):
    _add("env_map", f"envmap_{_h}x{_w}", _env_map(_h, _w, 40 + _k))
_add("env_map", "envmap_3x4_1e38", _env_map(3, 4, 50, scale=1e38))
_add("env_map", "envmap_3x4_negative", _env_map(3, 4, 51, negative=True))
for _base in ("cbox_envsphere", "cbox_envhemi"):
    _add("env_uniform", f"{_base[5:]}_0", _env_radiance(_base, (0, 0, 0)))
    _add("env_uniform", f"{_base[5:]}_1e30", _env_radiance(_base, (1e30, 0, 1e-30)))
_add("gate", "gate_albedo_1e15", _gate(GATE_WALL, GATE_CHANNEL, GATE_ALBEDO_AT))          # (the RECORD is at 1e15: albedo / PI_F)
_add("gate", "gate_albedo_above", _gate(GATE_WALL, GATE_CHANNEL, GATE_ALBEDO_ABOVE))
_add("gate", "gate_emission_1e15", _gate(LIGHT_MATERIAL, 0, 1e15))
_add("gate", "gate_emission_above", _gate(LIGHT_MATERIAL, 0, NEXT_ABOVE_1E15))

CASES = list(_TABLE)
BASE = {name: entry[0] for name, entry in _TABLE.items()}
# a base that is no named scene of pt_scene: the scene a case was cut from after the change that lets its parameter matter
_DERIVED_BASES = {"spot_down": _spot()[1], "blob_camera_inside": _camera_in_glass(base="cbox_blob512_glass")}
ORACLE_ONLY = ("emission_0", "emission_negative")
REFERENCE_SET = [c for c in CASES if c not in ORACLE_ONLY]
GATE_NEIGHBOURS = (("gate_albedo_1e15", "gate_albedo_above"), ("gate_emission_1e15", "gate_emission_above"))
# what elision_provable (csrc/pt.hip) decides per case with srt_pt_set_elision on: only a scene without delta and environment
# lights, with an emitting light and every Lambertian / light channel within 1e15, takes the two-ray build
ELIDING = [c for c in CASES if BASE[c] in ("cbox", "cbox_lambertian", "cbox_blob512_glass", "blob_camera_inside")
           and c not in ORACLE_ONLY + ("gate_albedo_above", "gate_emission_above", "emission_2e38")]


def shade_edge_scene(name):
    return _TABLE[name][1]()


def base_scene(name):
    """The scene case `name` differs from in one parameter."""
    b = BASE[name]
    return _DERIVED_BASES[b]() if b in _DERIVED_BASES else pt_scene(b)


def family_of(name):
    return next(f for f, names in FAMILIES.items() if name in names)
