"""Writes tests/golden/env_image_components.npz and env_image_paths.npz from the REFERENCE (authoring container only):
  * the component fixture from integration/_build/libref_env_sampler.so - Samplers::Sphere::Image itself with a settable RNG::unit
    (integration/harness/env_sampler_ref.cpp): _pdf, _cdf, total, sample() for chosen draws, pdf() for chosen directions;
  * the path fixture from integration/_build/libref_pt_envimage.so - the reference's path tracer with Env_Map::sample / pdf
    answered by the map's image sampler (integration/harness/env_image_ref.cpp).
Data only.  The script asserts, on the recorded values, what the tests rely on.   python tests/golden/make_env_image_golden.py"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the package (srt_amd), for the scenes
import _harness as H  # noqa: E402
import _env_image_cases as E  # noqa: E402

BUILD = os.path.join(H.ROOT, "integration", "_build")


def components():
    lib = ctypes.CDLL(os.path.join(BUILD, "libref_env_sampler.so"))
    lib.ref_env_sampler_create.restype = ctypes.c_void_p
    out = {}
    saw_end = saw_nonfinite = False
    for name in E.MAPS:
        img = E.env_map(name)
        h, w = img.shape[:2]
        s = ctypes.c_void_p(lib.ref_env_sampler_create(w, h, H.P(img)))
        pdf, cdf, total = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32), ctypes.c_float(0)
        lib.ref_env_sampler_tables(s, H.P(pdf), H.P(cdf), ctypes.byref(total))
        u = E.draws(name, cdf)
        dirs, index = np.zeros((len(u), 3), np.float32), np.zeros(len(u), np.uint32)
        lib.ref_env_sampler_sample(s, H.P(u), ctypes.c_size_t(len(u)), H.P(dirs), H.P(index))
        d = E.directions(name, dirs)
        p = np.zeros(len(d), np.float32)
        lib.ref_env_sampler_pdf(s, H.P(d), ctypes.c_size_t(len(d)), H.P(p))
        lib.ref_env_sampler_destroy(s)
        out.update({f"{name}.pdf": pdf, f"{name}.cdf": cdf, f"{name}.total": np.float32(total.value), f"{name}.u": u, f"{name}.index": index,
                    f"{name}.sample": dirs, f"{name}.dirs": d, f"{name}.pdf_of": p})
        saw_end |= bool((index == w * h).any())
        saw_nonfinite |= bool((~np.isfinite(p)).any())
        print(f"{name}: {w}x{h} total {total.value:g}, {len(u)} draws (max index {index.max()} of {w * h}), {len(d)} directions "
              f"({int((~np.isfinite(p)).sum())} pdfs not finite)")
    assert saw_end, "no recorded draw reaches the index w * h"
    assert saw_nonfinite, "no recorded pdf is inf or NaN"
    assert np.isnan(out["black.cdf"]).all() and (out["black.index"] == 12).all(), "a black map: NaN tables, every draw at w * h"
    # on the negative map the CDF is not sorted: the bisection's result is not the first element greater than u
    cdf, u, index = out["negative.cdf"], out["negative.u"], out["negative.index"]
    assert (np.diff(cdf) < 0).any()
    linear = np.array([next((i for i, c in enumerate(cdf) if c > x), len(cdf)) for x in u], np.uint32)
    assert (linear != index).any(), "the bisection and a linear scan agree on every recorded draw of the negative map"
    eq = out["zero_runs.cdf"]
    assert (np.diff(eq) == 0).any(), "the zero-run map has no equal CDF neighbours"
    np.savez_compressed(os.path.join(HERE, "env_image_components.npz"), **out)


def _ref(lib, scene):
    r = object.__new__(H.RefPT)
    r.lib, r.w, r.h = lib, E.W, E.H
    r.h_ = ctypes.c_void_p(lib.ref_pt_create(E.W, E.H, E.DEPTH, 1))
    r.feed(scene)
    return r


def paths():
    lib = ctypes.CDLL(os.path.join(BUILD, "libref_pt_envimage.so"))
    lib.ref_pt_create.restype = ctypes.c_void_p
    stock = H.ref_pt_lib()
    assert stock is not None, "oracle/_ref/libref_pt.so is missing"
    xs, ys, ss = E.sample_list()
    out = {"meta": np.array([E.W, E.H, E.DEPTH, E.EPOCH_SPP, E.EPOCH_BASE], np.int64), "seed": np.uint64(E.SEED)}
    calls = np.zeros(2, np.uint64)
    for name in E.PATH_SCENES:
        scene = E.path_scene(name)
        lib.ref_env_image_calls(H.P(calls), 1)
        r = _ref(lib, scene)
        rgb, draws = r.trace_samples(E.SEED, xs, ys, ss)
        lib.ref_env_image_calls(H.P(calls), 1)
        nsample, npdf = int(calls[0]), int(calls[1])
        epoch = r.epoch(E.SEED, E.EPOCH_BASE, E.EPOCH_SPP)
        u_rgb, u_draws = _ref(stock, scene).trace_samples(E.SEED, xs, ys, ss)
        assert nsample > 0 and npdf > 0, "the wrappers were not called"
        assert not np.array_equal(rgb.view(np.uint32), u_rgb.view(np.uint32)) and not np.array_equal(draws, u_draws), \
            f"{name}: the image sampler changes nothing against the stock build"
        if scene["env"] and any(o.get("is_light") for o in scene["objects"]):
            assert 0 < nsample < npdf, f"{name}: the coin of sample_area_lights never fell on one side ({nsample} of {npdf})"
        else:
            assert nsample == npdf, f"{name}: without area lights every light sample is the map's"
        assert np.isfinite(epoch).all()
        print(f"{name}: {nsample} sample() / {npdf} pdf() calls, {int((draws != u_draws).sum())} of {len(draws)} draw counts differ from the uniform build, "
              f"{int((~np.isfinite(rgb)).any(axis=1).sum())} samples not finite")
        out.update({f"{name}.rgb": rgb, f"{name}.draws": draws, f"{name}.epoch": epoch})
    np.savez_compressed(os.path.join(HERE, "env_image_paths.npz"), **out)


if __name__ == "__main__":
    components()
    paths()
