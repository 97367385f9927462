"""GPU: new shading values for a committed scene on the device - the shading timelines' kernel (srt_pt_shading_timeline_apply) against
what the reference recorded (tests/golden/anim_shading.npz) through dump_shading, and apply / update / update_materials /
update_lights followed by a render against a fresh commit built from the recorded values: image and ray count, under the automatic
kernel form and every forced form that takes the scene, with and without BVHs.  Then the enqueue-only loop on one stream, the upload
figures, the elision proof while the host's record lags, and a two-rank group.  Every comparison is bit for bit."""
import numpy as np
import pytest

import _anim_cases as AC
import _cases
import _shading_cases as SH

pytestmark = pytest.mark.gpu

F = np.float32
UNSUPPORTED = -4
W, HT, DEPTH, SPP, SEED = 32, 24, 4, 4, 11


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def g():
    return SH.load()


def make_pt(srt, scene, device=0, use_bvh=True, depth=DEPTH):
    pt = srt.Pathtracer(device)
    pt.set_params(W, HT, 1, depth, use_bvh)
    pt.build_scene(scene)
    if device >= 0:
        pt.set_camera(scene["camera"])
    return pt


def render_case(g, name):
    """(scene, material indices, light indices, tracks) of a rendered scene: the delta-light box takes the whole "render" group, the
    blob-mesh box its three materials."""
    scene = _cases.pt_scene(name)
    if name == "cbox_deltalights":
        return scene, np.array(SH.RENDER_MATERIALS, np.uint32), np.array(SH.RENDER_LIGHTS, np.uint32), SH.tracks(g, "render")
    return scene, np.array(SH.RENDER_MATERIALS, np.uint32), np.zeros(0, np.uint32), SH.sub_tracks(g, "render", range(18))


def values_at(g, scene, lights, ti):
    mats = SH.material_values(g, "render", ti)
    l21 = SH.light_values(g, "render", ti, scene.get("lights", [])[:3])[:len(lights)]
    return mats, l21


def renders(srt, pt, modes):
    """{mode: (image, rays)} for the modes that take the scene."""
    out = {}
    for mode in modes:
        pt.set_kernel(mode)
        try:
            pt.ray_count(reset=True)
            img = pt.render_epoch(SEED, 0, SPP)
            out[mode] = (img, pt.ray_count()[0])
        except srt.SrtError as e:
            assert e.status == UNSUPPORTED, (mode, e)
        pt.set_kernel(0)
    return out


def same_renders(got, want):
    assert got.keys() == want.keys()
    for mode in want:
        assert AC.bits_equal(got[mode][0], want[mode][0]) and got[mode][1] == want[mode][1], f"kernel mode {mode}: rays {got[mode][1]} / {want[mode][1]}"


def test_apply_equals_the_reference(srt, g):
    """apply(t) then dump_shading(device) at every recorded time: 20 materials, 300 lights (320 lanes: six blocks, the material / light
    boundary inside the first wave) equal the recorded values, and the whole dump - itrans, has_trans - equals the host form's."""
    scene, mats, lights = SH.record_scene(g)
    pt, host = make_pt(srt, scene), make_pt(srt, scene, device=-1)
    tl, tl_host = (p.create_shading_timeline(mats, lights, True, SH.tracks(g, "record")) for p in (pt, host))
    bad = {}
    for i, t in enumerate(g["times"]):
        tl.apply(float(t))
        tl_host.update(float(t))
        d, want = pt.dump_shading(from_device=True), host.dump_shading()
        want_m, want_l = SH.stored(SH.material_values(g, "record", i)), SH.light_values(g, "record", i, scene["lights"])
        bad[float(t)] = (sum(AC.mismatches(d["materials"][f][mats], want_m[f]) for f in ("a", "b", "ior")), AC.mismatches(d["lights"][:, :21], want_l),
                         AC.mismatches(d["env_radiance"], g["record_env_out"][i]), int(not SH.dumps_equal(d, want)), int(not SH.dumps_equal(pt.dump_shading(), want)))
    tl.close(); tl_host.close()
    pt.close(); host.close()
    assert not any(any(b) for b in bad.values()), bad


@pytest.mark.parametrize("use_bvh", [True, False])
@pytest.mark.parametrize("name", ["cbox_deltalights", "cbox_blob512_glass"])
def test_renders_equal_a_fresh_commit(srt, g, name, use_bvh):
    """apply(t), the host form update(t), and update_materials / update_lights with explicit values, each followed by a render under
    every kernel form that takes the scene: image and ray count of a fresh commit built from the recorded values.  Then the time at
    which the area light's keyed emission is exactly 0."""
    scene, mats, lights, tracks = render_case(g, name)
    modes = range(8)
    for ti, sweep in ((SH.T_BETWEEN, modes), (SH.T_ZERO_EMISSION, (0,))):
        t = float(g["times"][ti])
        want_m, want_l = values_at(g, scene, lights, ti)
        fresh = make_pt(srt, SH.with_values(scene, mats, want_m, lights, want_l), use_bvh=use_bvh)
        want, want_dump = renders(srt, fresh, sweep), fresh.dump_shading(from_device=True)
        fresh.close()
        assert 0 in want and (len(want) >= 4 or len(sweep) == 1), want.keys()
        for how in ("apply", "update", "explicit"):
            pt = make_pt(srt, scene, use_bvh=use_bvh)
            tl = pt.create_shading_timeline(mats, lights, False, tracks)
            if how == "explicit":
                pt.update_materials(mats, want_m)
                if len(lights):
                    pt.update_lights(lights, want_l[:, :3], want_l[:, 3:5], want_l[:, 5:])
            else:
                getattr(tl, how)(t)
            same_renders(renders(srt, pt, sweep), want)
            assert SH.dumps_equal(pt.dump_shading(from_device=True), want_dump) and SH.dumps_equal(pt.dump_shading(), want_dump), how
            tl.close()
            pt.close()
    assert np.all(want_m["a"][2] == 0)                                                # (the last time: a black area light)


def test_enqueue_only_on_one_stream(srt, torch, g):
    """render_epoch_device A, apply(t), render_epoch_device B on one stream with no host wait in between: A is the committed scene's
    image, B the fresh commit's at t."""
    scene, mats, lights, tracks = render_case(g, "cbox_deltalights")
    ti = SH.T_BETWEEN
    want_m, want_l = values_at(g, scene, lights, ti)
    pt = make_pt(srt, scene)
    tl = pt.create_shading_timeline(mats, lights, False, tracks)
    local_tiles, _, floats_per_tile = pt.tile_info()
    tiles = [torch.zeros(local_tiles * floats_per_tile, device="cuda:0") for _ in range(2)]
    images = [torch.zeros(HT * W * 3, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    pt.render_epoch_device(s, SEED, 0, SPP, tiles[0].data_ptr())
    pt.untile_device(s, tiles[0].data_ptr(), images[0].data_ptr())
    tl.apply(float(g["times"][ti]), s)
    pt.render_epoch_device(s, SEED, 0, SPP, tiles[1].data_ptr())
    pt.untile_device(s, tiles[1].data_ptr(), images[1].data_ptr())
    st.synchronize()
    a, b = (im.cpu().numpy().reshape(HT, W, 3) for im in images)
    tl.close(); pt.close()
    committed, fresh = make_pt(srt, scene), make_pt(srt, SH.with_values(scene, mats, want_m, lights, want_l))
    want_a, want_b = committed.render_epoch(SEED, 0, SPP), fresh.render_epoch(SEED, 0, SPP)
    committed.close(); fresh.close()
    assert AC.bits_equal(a, want_a) and AC.bits_equal(b, want_b) and not AC.bits_equal(want_a, want_b)


def test_upload_figures(srt, g):
    """The steady state uploads nothing: after the first apply the upload figure does not move over ten further calls.  The host forms
    move it by exactly 32 B per listed material and 160 B per listed light."""
    scene, mats, lights, tracks = render_case(g, "cbox_deltalights")
    pt = make_pt(srt, scene)
    tl = pt.create_shading_timeline(mats, lights, False, tracks)
    T = g["times"]
    tl.apply(float(T[2]))
    c0 = pt.scene_counts()
    for k in range(10):
        tl.apply(float(T[k % len(T)]))
    c1 = pt.scene_counts()
    assert c1["uploaded_bytes"] == c0["uploaded_bytes"] and c1["device_bytes"] == c0["device_bytes"] and c1["objects"] == c0["objects"]
    want_m, want_l = values_at(g, scene, lights, SH.T_BETWEEN)
    pt.update_materials(mats[:2], want_m[:2])
    c2 = pt.scene_counts()
    pt.update_lights(lights, want_l[:, :3], want_l[:, 3:5], want_l[:, 5:])
    c3 = pt.scene_counts()
    tl.update(float(T[5]))
    c4 = pt.scene_counts()
    assert c2["uploaded_bytes"] - c1["uploaded_bytes"] == 32 * 2 and c3["uploaded_bytes"] - c2["uploaded_bytes"] == 160 * len(lights)
    assert c4["uploaded_bytes"] - c3["uploaded_bytes"] == 32 * len(mats) + 160 * len(lights)
    assert c4["uploaded_triangle_bytes"] == c0["uploaded_triangle_bytes"] and c4["blas_builds"] == c0["blas_builds"]
    tl.close(); pt.close()


def test_elision_while_the_record_lags(srt, torch, g):
    """set_elision on an all-Lambertian box with a keyed albedo: an epoch launched while the host's record lags elides nothing, one
    launched after srt_pt_sync elides again, and both images equal the un-elided context's."""
    scene = _cases.pt_scene("cbox_lambertian")
    mats, tracks = np.array([0], np.uint32), SH.sub_tracks(g, "render", range(6))
    t = float(g["times"][SH.T_BETWEEN])
    got = {}
    for elide in (True, False):
        pt = make_pt(srt, scene)
        pt.set_elision(elide)
        pt.set_kernel(2)                                      # the persistent sweeps: the form whose two-ray batches the proof switches on
        tl = pt.create_shading_timeline(mats, [], False, tracks)
        local_tiles, _, floats_per_tile = pt.tile_info()
        tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
        before = pt.render_epoch(SEED, 0, SPP)
        elided_before = pt.rays_elided(reset=True)
        torch.cuda.synchronize()
        st = torch.cuda.Stream(device="cuda:0")
        tl.apply(t, st.cuda_stream)
        pt.render_epoch_device(st.cuda_stream, SEED, 0, SPP, tiles.data_ptr())
        pt.untile_device(st.cuda_stream, tiles.data_ptr(), image.data_ptr())
        st.synchronize()
        lagging, elided_lagging = image.cpu().numpy().reshape(HT, W, 3), pt.rays_elided(reset=True)
        pt.sync()
        settled = pt.render_epoch(SEED, 0, SPP)
        got[elide] = (before, lagging, settled, elided_before, elided_lagging, pt.rays_elided())
        tl.close(); pt.close()
    on, off = got[True], got[False]
    assert on[3] > 0 and on[4] == 0 and on[5] > 0 and off[3:] == (0, 0, 0), (on[3:], off[3:])
    for k in range(3):
        assert AC.bits_equal(on[k], off[k]), k
    assert AC.bits_equal(on[1], on[2]) and not AC.bits_equal(on[0], on[1])
    want_m = SH.material_values(g, "render", SH.T_BETWEEN)[:1]
    fresh = make_pt(srt, SH.with_values(scene, mats, want_m, [], []))
    assert AC.bits_equal(fresh.render_epoch(SEED, 0, SPP), on[2])
    fresh.close()


def test_group(srt, g):
    """Two ranks on one device: ShadingTimelineGroup gives every rank the same t, and the image is the single context's."""
    scene, mats, lights, tracks = render_case(g, "cbox_deltalights")
    ti = SH.T_BETWEEN
    want_m, want_l = values_at(g, scene, lights, ti)
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(scene)
    grp.set_camera(scene["camera"])
    tl = grp.create_shading_timeline(mats, lights, False, tracks)
    assert len(tl.timelines) == 2 and AC.bits_equal(tl.values(float(g["times"][ti]))["lights"], want_l)
    tl.apply(float(g["times"][ti]))
    applied = grp.render_epoch(SEED, 0, SPP)
    dumps = grp.dump_shading(from_device=True)
    tl.update(float(g["times"][SH.T_ZERO_EMISSION]))
    updated = grp.render_epoch(SEED, 0, SPP)
    tl.close(); grp.close()
    single = make_pt(srt, SH.with_values(scene, mats, want_m, lights, want_l))
    want_applied, want_dump = single.render_epoch(SEED, 0, SPP), single.dump_shading(from_device=True)
    single.close()
    single = make_pt(srt, SH.with_values(scene, mats, *values_at(g, scene, lights, SH.T_ZERO_EMISSION)[:1], lights, values_at(g, scene, lights, SH.T_ZERO_EMISSION)[1]))
    want_updated = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert AC.bits_equal(applied, want_applied) and AC.bits_equal(updated, want_updated) and all(SH.dumps_equal(d, want_dump) for d in dumps)
