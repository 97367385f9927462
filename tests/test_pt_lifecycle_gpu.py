"""GPU: who owns what.  Every HIP allocation, event and stream of the library lives in an owner (csrc/hip_owned.h) that counts
itself, and srt_pt_live_resources reads the four counts: a context that has been through every entry point that allocates, then
destroyed with its skins and timelines, leaves the four counts where they were - nothing leaks, nothing is freed twice (a second
free of a block would take a count below its start).  The same drive repeated on a live context holds the counts still, handles of
an older commit stay destroyable, and the images along the way are the oracle's, bit for bit: moving ownership moved no data.  The
multi-device group (csrc/pt_group.cpp) gets the same three checks, and one of a create that fails half-way.  Smallest sizes
throughout: 32x24 pixels, depth 3, 2 samples per epoch."""
import os

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _instance_cases as IC
import _skin_cases as SC
import _update_cases as UC
from _cases import pt_scene

pytestmark = pytest.mark.gpu

F = np.float32
W, HT, DEPTH, SPP, SEED = 32, 24, 3, 2, 11
UNSUPPORTED = -4
MODES = (0, 4, 6, 7)
# (scene, committed with BVHs): the Cornell box as a list and as trees, a real BVH<Triangle>, the delta lights
SCENES = [("cbox", False), ("cbox", True), ("cbox_blob512_glass", True), ("cbox_deltalights", True)]
IDS = [f"{n}-{'bvh' if b else 'list'}" for n, b in SCENES]
GOLDEN = os.path.join(H.GOLDEN, "lifecycle_epochs.npz")


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def live(srt):
    import gc

    from soft_rendering_toolsets_amd._pt_bindings import live_resources

    def read():
        gc.collect()                                        # (a context an earlier test left to the collector goes now, not between two readings)
        return live_resources()

    return read


@pytest.fixture(scope="module")
def goldens():
    """The committed epoch images (tests/golden/make_lifecycle_golden.py wrote them from the oracle), checked against the oracle once."""
    g = np.load(GOLDEN)
    out = {}
    for (name, use_bvh), key in zip(SCENES, IDS):
        want = H.OraclePT(pt_scene(name), W, HT, DEPTH, use_bvh).epoch(SEED, 0, SPP)
        assert AC.bits_equal(g[key], want), f"{key}: the committed golden is not the oracle's epoch"
        out[key] = g[key]
    return out


def light_index(scene):
    return next(i for i, o in enumerate(scene["objects"]) if o.get("is_light"))


def sphere_index(scene):
    return next(i for i, o in enumerate(scene["objects"]) if o["kind"] == "sphere")


def mesh_index(scene):
    """A mesh srt_pt_update_mesh takes: the blob where the scene has one, else the first wall."""
    if len(scene["objects"]) > UC.BLOB_OBJECT and scene["objects"][UC.BLOB_OBJECT]["kind"] == "mesh" and not scene["objects"][UC.BLOB_OBJECT].get("is_light"):
        return UC.BLOB_OBJECT
    return next(i for i, o in enumerate(scene["objects"]) if o["kind"] == "mesh" and not o.get("is_light"))


def committed_T(scene, i):
    return np.ascontiguousarray(scene["objects"][i]["T"], F).reshape(16)


def commit(pt, scene, use_bvh):
    pt.set_params(W, HT, 1, DEPTH, use_bvh)
    pt.set_dynamic_lights(True)
    pt.set_bvh_builder(True, 8)                             # the device builder for every tree of 8 primitives and more
    pt.build_scene(scene)
    pt.set_camera(scene["camera"])


def render_modes(srt, pt, name, use_bvh):
    """One epoch under every mode the scene takes; the images (all equal).  Mode 7 needs a real BVH<Triangle>, 6 a scene it can pack."""
    images = {}
    for mode in MODES:
        pt.set_kernel(mode)
        try:
            images[mode] = pt.render_epoch(SEED, 0, SPP)
        except srt.SrtError as e:
            assert e.status == UNSUPPORTED and mode in (6, 7), (mode, str(e))
    pt.set_kernel(0)
    assert 0 in images and 4 in images
    if name == "cbox_blob512_glass":
        assert 6 in images and 7 in images
    return images


def drive(srt, torch, pt, scene, name, use_bvh, read_timers):
    """Every owner of the context once, on the scene just committed.  Returns the epoch images (rendered before anything moves) and the
    handles that are still open."""
    keep = []

    def dev(a):
        keep.append(torch.from_numpy(np.ascontiguousarray(a, F)).to("cuda:0"))
        return keep[-1].data_ptr()

    images = render_modes(srt, pt, name, use_bvh)
    # timing brackets: the dominant kernel's, and the streamed form's four (the probe kernel's is the fourth)
    pt.kernel_time(True); pt.stream_times(True)
    for mode in images:
        pt.set_kernel(mode)
        pt.render_epoch(SEED, 0, SPP)
    pt.set_kernel(0)
    if read_timers:
        pt.kernel_time(False); pt.stream_times(False)       # (read: the pairs go to the spares)
    pt.set_ray_log(16)
    pt.render_epoch(SEED, 0, SPP)
    pt.read_ray_log()
    pt.set_ray_log(0)
    x = np.linspace(0.1, 2.0, 70, dtype=F)
    assert np.isfinite(pt.math_hypot(x, x[::-1].copy())).all() and np.isfinite(pt.math_exp(x)).all()   # a debug round trip of each kind
    # new vertices for a mesh: rebuilt (the device builder: threshold 8), then refitted
    m = mesh_index(scene)
    pos, nrm = UC.original(scene, m)
    pt.update_mesh(m, pos, nrm)
    pt.refit_mesh(m, pos, nrm)
    handles = []
    if name == "cbox_blob512_glass":                        # a skin with a rig on the blob, posed at a time of its keys
        g, joints = SC.load_fixture("blob_chain3")
        rig = AC.load_rig("blob_chain3")
        skin = pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints)
        skin.set_rig(*[rig[k] for k in ("parent", "base", "rest_pose", "knot_offsets", "knot_times", "knot_quats")])
        skin.pose_refit_at(float(rig["times"][2]))
        handles.append(skin)
    # an object timeline on a sphere: two position keys around where it stands
    s = sphere_index(scene)
    at = committed_T(scene, s)[12:15]
    tl = pt.create_timeline([s], [((np.array([0.0, 1.0], F), np.stack([at, at + F(0.01)])), None, None)])
    tl.repose_refit(0.5)
    handles.append(tl)
    # a shading timeline: the albedo of material 0, and a delta light's radiance where the scene has one
    albedo = (np.array([0.0, 1.0], F), np.array([[0.2, 0.3, 0.4], [0.5, 0.5, 0.5]], F))
    nl = 1 if scene.get("lights") else 0
    tracks = [albedo] + [None] * 5 + ([(np.array([0.0, 1.0], F), np.array([[0.3, 0.3, 0.3], [0.6, 0.5, 0.4]], F))] + [None] * 5) * nl
    sh = pt.create_shading_timeline([0], [0] * nl, False, tracks)
    sh.apply(0.5)
    handles.append(sh)
    # device-form reposes with the area light in the list, under srt_pt_set_dynamic_lights
    li = light_index(scene)
    listed = [s, li]
    moved = np.stack([IC.translate(committed_T(scene, s), (0.01, 0.0, 0.0)), IC.translate(committed_T(scene, li), (0.0, -0.01, 0.0))])
    pt.repose_device(listed, dev(moved))
    pt.repose_refit_device(listed, dev(moved))
    pt.repose_refit_device(listed, dev(np.stack([committed_T(scene, s), committed_T(scene, li)])))
    pt.render_epoch(SEED, 0, SPP)                           # (settles what is pending)
    return images, handles


@pytest.mark.parametrize("name,use_bvh", SCENES, ids=IDS)
def test_balance_and_pixels(srt, torch, live, goldens, name, use_bvh):
    """1 and 4: create, drive every owner, destroy - the four counts are back where they started; and the images rendered on the
    way are the committed goldens.  The timing brackets of the last renders are left unread: destroy owns them too (all four slots
    of the streamed form's)."""
    scene = pt_scene(name)
    before = live()
    pt = srt.Pathtracer(0)
    commit(pt, scene, use_bvh)
    images, handles = drive(srt, torch, pt, scene, name, use_bvh, read_timers=False)
    during = live()
    assert during[0] > before[0] and during[1] > before[1] and during[2] > before[2] and during[3] > before[3], (before, during)
    for h in handles:
        h.close()
    pt.close()
    assert live() == before, (before, during, live())
    key = IDS[SCENES.index((name, use_bvh))]
    for mode, img in images.items():
        assert AC.bits_equal(img, goldens[key]), f"{key}, kernel mode {mode}: the epoch differs from the golden"


def test_steady_state(srt, torch, live):
    """2: commit and drive the same scene three times on one context: what a commit and a growing array replace is freed, so the
    second and the third round end on the same counts."""
    name, use_bvh = "cbox_blob512_glass", True
    scene = pt_scene(name)
    before = live()
    pt = srt.Pathtracer(0)
    after = []
    for _ in range(3):
        commit(pt, scene, use_bvh)
        _, handles = drive(srt, torch, pt, scene, name, use_bvh, read_timers=True)
        for h in handles:
            h.close()
        after.append(live())
    assert after[1] == after[2], after
    pt.close()
    assert live() == before, (before, after, live())


def test_stale_handles(srt, torch, live):
    """3: a skin, a timeline and a shading timeline made before a second commit are refused afterwards, and still destroyable."""
    name, use_bvh = "cbox_blob512_glass", True
    scene = pt_scene(name)
    before = live()
    pt = srt.Pathtracer(0)
    commit(pt, scene, use_bvh)
    _, handles = drive(srt, torch, pt, scene, name, use_bvh, read_timers=True)
    assert len(handles) == 3
    commit(pt, scene, use_bvh)
    skin, tl, sh = handles
    for call in (lambda: skin.pose_refit_at(0.5), lambda: tl.repose_refit(0.5), lambda: sh.apply(0.5)):
        with pytest.raises(srt.SrtError) as e:
            call()
        assert e.value.status == -5                         # SRT_ERR_STATE: stale
    pt.render_epoch(SEED, 0, SPP)
    for h in handles:
        h.close()
    pt.close()
    assert live() == before, (before, live())


# ---- the multi-device group (srt_pt_create_multi): what the drop-in class and the benchmark render through -------------------------
# cbox with BVHs.  32x24 is less than one 32x32 tile: ranks 1 and 2 of a three-rank group own nothing, the smallest case in which a
# per-rank loop can go wrong.  72x40 has padding tiles, and going there replaces every lane buffer and accumulator.
GROUP_SCENE, GROUP_KEY, W2, HT2 = "cbox", "cbox-bvh", 72, 40


def commit_group(g, scene, w, h):
    g.set_params(w, h, 1, DEPTH, True)
    g.build_scene(scene)
    g.set_camera(scene["camera"])


@pytest.mark.parametrize("devices", [[0], [0, 0, 0]], ids=["1rank", "3ranks"])
def test_group_balance(srt, live, goldens, devices):
    """5: a group through every entry point of its own that allocates - lanes 0, 1 and the display lane, both kinds of timing pair
    (read and left unread), the accumulators, the ray log, a change of image size, handle groups - then closed: the four counts
    are back where they started, and the first epoch is the committed golden."""
    scene = pt_scene(GROUP_SCENE)
    before = live()
    g = srt.PathtracerGroup(devices)
    commit_group(g, scene, W, HT)
    assert AC.bits_equal(g.render_epoch(SEED, 0, SPP), goldens[GROUP_KEY]), f"devices {devices}: the epoch differs from the golden"
    g.render_epoch_lane(1, SEED, 0, SPP)
    g.gather_time(True)
    g.render_epoch(SEED, 0, SPP)
    ms, epochs = g.gather_time(False)                       # (read: the pair goes to the spares)
    assert epochs == 1 and ms >= 0.0
    g.gather_time(True)
    g.render_epoch(SEED, 0, SPP)                            # (left unread: destroy owns the pair)
    # two launches in flight on lanes 0 and 1, folded in launch order; one epoch folded is that epoch
    g.render_samples(0, SEED, 0, SPP)
    g.render_samples(1, SEED, SPP, SPP)
    g.wait_lane(0)
    g.fold(0, SPP, 0, 2 * SPP, 0)
    assert AC.bits_equal(g.accumulator_image(), goldens[GROUP_KEY]), f"devices {devices}: the folded epoch differs from the golden"
    g.wait_lane(1)
    g.fold(1, SPP, SPP, 2 * SPP, 0)
    assert np.isfinite(g.accumulator_image()).all()
    g.set_ray_log(16)
    g.render_epoch(SEED, 0, SPP)
    g.read_ray_log()
    g.set_ray_log(0)
    commit_group(g, scene, W2, HT2)
    assert g.render_epoch(SEED, 0, SPP).shape == (HT2, W2, 3)
    s = sphere_index(scene)
    at = committed_T(scene, s)[12:15]
    tl = g.create_timeline([s], [((np.array([0.0, 1.0], F), np.stack([at, at + F(0.01)])), None, None)])
    tl.repose_refit(0.5)
    sh = g.create_shading_timeline([0], [], False, [(np.array([0.0, 1.0], F), np.array([[0.2, 0.3, 0.4], [0.5, 0.5, 0.5]], F))] + [None] * 5)
    sh.apply(0.5)
    tl.close()
    sh.close()
    during = live()
    assert all(d > b for d, b in zip(during, before)) and len(during) == 4, (before, during)
    g.close()
    assert live() == before, (before, during, live())


def test_group_steady_state(srt, live):
    """6: one two-rank group between two image sizes, three times: the lane buffers and accumulators a new size replaces are freed, so
    the second and the third round end on the same counts."""
    scene = pt_scene(GROUP_SCENE)
    before = live()
    g = srt.PathtracerGroup([0, 0])
    commit_group(g, scene, W, HT)
    after = []
    for _ in range(3):
        for w, h in ((W, HT), (W2, HT2)):
            g.set_params(w, h, 1, DEPTH, True)
            g.reset_accumulator()
            g.render_epoch(SEED, 0, SPP)
        after.append(live())
    assert after[1] == after[2], after
    g.close()
    assert live() == before, (before, after, live())


def test_group_create_fails_half_way(srt, live):
    """7: rank 1's device does not exist (srt_pt_create refuses it before it touches a device): rank 0's context, events and stream go
    away with the partly built group."""
    before = live()
    with pytest.raises(srt.SrtError) as e:
        srt.PathtracerGroup([0, 10_000])
    assert e.value.status == -1                             # SRT_ERR_INVALID
    assert live() == before, (before, live())
