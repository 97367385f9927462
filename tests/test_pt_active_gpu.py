"""GPU: srt_pt_set_active / srt_pt_set_active_device - objects of a committed scene switched off and on without a commit.  A scene
with hidden objects keeps the tree of the commit (the oracle would walk another), so the expectation is the host definition walked
by the device headers on the CPU (tests/_active_cases.py: EmuActive), produced here at test time; where hiding and leaving out must
agree the other side is a fresh commit without the objects.  Everything is compared bit for bit.  Device arrays are torch tensors
passed by data_ptr()."""
import numpy as np
import pytest

import _active_cases as A
import _instance_cases as IC
import _light_cases as LC
import _repose_device_cases as RDC
import _repose_refit_cases as C
import _skin_cases as SC
import _update_cases as UC
from _active_cases import DEPTH, HT, SEED, SPP, W, bits_equal
from _cases import random_rays

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -5, -4


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def make_pt(srt, scene, device=0, use_bvh=True, dynamic=False):
    pt = srt.Pathtracer(device)
    pt.set_params(W, HT, 1, DEPTH, use_bvh)
    if dynamic:
        pt.set_dynamic_lights(True)
    pt.build_scene(scene)
    if device >= 0:
        pt.set_camera(scene["camera"])
    return pt


def flags_on_device(torch, flags):
    d = torch.from_numpy(np.ascontiguousarray(flags, np.uint8)).to("cuda:0")
    torch.cuda.synchronize()
    return d


def top_dump(pt, nobj):
    boxes, links, order = pt.dump_bvh(-1, cap=2 * nobj + 2)
    return boxes, links, order[:nobj]


def top_equal(a, b):
    return bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def check_against(pt, want, modes, hit_modes=(0,)):
    """Every sample with its RNG draw and ray ledgers, the hit records of the walks, and per kernel mode the epoch image - the fold
    of those samples."""
    rgb, draws, rays = pt.trace_samples(SEED, *A.every_sample(W, HT, SPP))
    assert np.array_equal(draws, want["samples"][1]) and np.array_equal(rays, want["samples"][2])
    assert bits_equal(rgb, want["samples"][0])
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    for mode in hit_modes:
        pt.set_kernel(mode)
        got = pt.hit(org, d, b)
        pt.set_kernel(0)
        assert bits_equal(got, want["hits"][1 if mode == 5 else 0]), f"hit under kernel mode {mode}"
    for mode in modes:
        pt.set_kernel(mode)
        got = pt.render_epoch(SEED, 0, SPP)
        pt.set_kernel(0)
        assert bits_equal(got, want["epoch"]), f"kernel mode {mode}"


def case(which):
    """(scene, hidden objects, kernel modes, hit modes): the 74-object particle scene with a third of its particles off (the streamed
    form and the lane-per-pixel kernel), or IC.sweeps_scene() with the blob - whose instance stays - and a wall off (the sweeps, the
    inline walks, the flattened walk and the streamed sweeps)."""
    if which == "particles":
        return IC.particles_shared()[0], A.hidden(), (0, 1, 6), (0,)
    return IC.sweeps_scene(), np.array([UC.BLOB_OBJECT, 2], np.uint32), (0, 2, 5, 7), (0, 5)


@pytest.fixture(scope="module")
def wanted():
    """The emulated expectation of each case, computed once."""
    out = {}
    for which in ("particles", "sweeps"):
        S, off, _, _ = case(which)
        out[which] = A.expectation(S, [("active", off, np.zeros(len(off), np.uint8))])
    return out


@pytest.mark.parametrize("which", ["particles", "sweeps"])
def test_host_form_on_the_device(srt, wanted, which):
    """The dumps are the host-only context's, every sample of 32x24xSPP equals the emulation with its ledgers, and the epoch image of
    every kernel form is the fold of those samples."""
    S, off, modes, hit_modes = case(which)
    nobj, want = len(S["objects"]), wanted[which]
    only = make_pt(srt, S, device=-1)
    only.set_active(off, np.zeros(len(off), np.uint8))
    want_dumps, want_cost = IC.all_dumps(only, nobj), only.scene_tree_cost()
    only.close()
    pt = make_pt(srt, S)
    before = pt.render_epoch(SEED, 0, SPP)
    pt.set_active(off, np.zeros(len(off), np.uint8))
    check_against(pt, want, modes, hit_modes)
    assert not bits_equal(before, want["epoch"])
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), want_dumps) and top_equal(top_dump(pt, nobj), want["dump"])
    assert np.array_equal(pt.active(), want["active"]) and pt.scene_tree_cost() == want_cost == want["cost"]
    pt.close()


@pytest.mark.parametrize("which", ["particles", "sweeps"])
def test_hidden_is_left_out(srt, wanted, which):
    """The GPU's closest hits with the objects hidden against a fresh commit without them on a second context: at most A.TIES_CAP = 0
    of the 2048 rays differ."""
    S, off, _, _ = case(which)
    pt, fresh = make_pt(srt, S), make_pt(srt, A.without(S, off))
    pt.set_active(off, np.zeros(len(off), np.uint8))
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    a, f = pt.hit(org, d, b), fresh.hit(org, d, b)
    pt.close(); fresh.close()
    differ = A.mismatches(a, f)
    print(f"{which}: {differ} of {A.RAYS} rays differ between the hidden and the absent objects")
    assert bits_equal(a, wanted[which]["hits"][0]) and differ <= A.TIES_CAP == 0 and np.count_nonzero(f[:, 0]) > 500


def test_device_form(srt, torch, wanted):
    """The flags come from a device buffer.  The call only enqueues: right after it one call is pending and nothing was settled;
    after sync the dumps and the table are the host form's.  Uploads: 4 B per listed object for a new list, nothing for a repeated one."""
    S, off, modes, _ = case("particles")
    nobj, want = len(S["objects"]), wanted["particles"]
    pidx = A.particle_indices()
    flags = A.flags_of(nobj, off)[pidx]                     # d_alive's layout: one byte per particle
    d_flags = flags_on_device(torch, flags)
    host, pt = make_pt(srt, S), make_pt(srt, S)
    host.set_active(off, np.zeros(len(off), np.uint8))
    assert pt.top_refit_pending() == (0, 0)
    pt.set_active_device(pidx, d_flags.data_ptr())
    assert pt.top_refit_pending() == (1, 0)                 # enqueued, not settled: the host's record lags
    pt.sync()
    assert pt.top_refit_pending() == (0, 0) and pt.top_refit_count() == 0
    assert np.array_equal(pt.active(), host.active()) and np.array_equal(pt.active(), want["active"])
    assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(host, nobj)) and pt.scene_tree_cost() == host.scene_tree_cost()
    check_against(pt, want, modes)
    # the upload figure in the steady state
    c0 = pt.scene_counts()["uploaded_bytes"]
    pt.set_active_device(pidx, d_flags.data_ptr())          # the list the device holds
    c1 = pt.scene_counts()["uploaded_bytes"]
    other = np.ascontiguousarray(pidx[::-1][:9])
    d_other = flags_on_device(torch, flags[::-1][:9].copy())
    pt.set_active_device(other, d_other.data_ptr())
    c2 = pt.scene_counts()["uploaded_bytes"]
    pt.set_active_device(other, d_other.data_ptr())
    assert pt.top_refit_pending() == (1, 0)
    c3 = pt.scene_counts()["uploaded_bytes"]
    assert c1 - c0 == 0 and c2 - c1 == 4 * len(other) and c3 - c2 == 0
    assert np.array_equal(pt.active(), want["active"])
    # and back on, from the device: the committed scene as values, the untouched context's image bit for bit
    d_ones = flags_on_device(torch, np.ones(len(pidx), np.uint8))
    pt.set_active_device(pidx, d_ones.data_ptr())
    untouched = make_pt(srt, S)
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), untouched.render_epoch(SEED, 0, SPP)) and np.all(pt.active() == 1)
    first = IC.all_dumps(untouched, nobj)
    back = IC.all_dumps(pt, nobj)
    assert A.values_equal(back[0][0], first[0][0]) and np.array_equal(back[0][1], first[0][1]) and IC.dumps_equal(back[1:], first[1:])
    for p in (host, pt, untouched):
        p.close()


def test_device_form_on_the_sweeps_scene(srt, torch, wanted):
    """At most 16 objects: the kernels that read the sweep records and their leaf counts, after the device form."""
    S, off, modes, hit_modes = case("sweeps")
    nobj = len(S["objects"])
    d_flags = flags_on_device(torch, np.zeros(len(off), np.uint8))
    pt = make_pt(srt, S)
    pt.set_active_device(off, d_flags.data_ptr())
    check_against(pt, wanted["sweeps"], modes, hit_modes)
    assert top_equal(top_dump(pt, nobj), wanted["sweeps"]["dump"])
    pt.close()


def test_pool_loop(srt, torch):
    """particles_step_device -> particle_transforms_device -> set_active_device(d_alive) -> repose_refit_device ->
    render_epoch_device, three frames on one stream with no host wait in between.  A third of the particles die in frame 2; one dead
    slot is respawned by a torch write before frame 3.  The final epoch, table and dumps equal a second context driven through the
    host forms with the same numbers."""
    S = IC.particles_shared()[0]
    nobj = len(S["objects"])
    pidx = A.particle_indices()
    n = len(pidx)
    pos0 = RDC.particle_positions(S)
    rng = np.random.default_rng(8)
    vel0 = ((rng.random((n, 3)) - 0.5) * 2.0).astype(np.float32)
    dt, radius = 0.01, 0.015
    age0 = np.full(n, 10.0, np.float32)
    dying = np.arange(1, n, 3)
    age0[dying] = np.float32(0.015)                         # alive after frame 1, dead from frame 2 on
    slot = int(dying[2])
    spawn_pos, spawn_vel = np.array([0.1, 0.6, 0.05], np.float32), np.array([0.3, -0.2, 0.1], np.float32)
    # the device loop
    pt = make_pt(srt, S)
    local_tiles, _, floats_per_tile = pt.tile_info()
    d_pos, d_vel = torch.from_numpy(pos0.copy()).to("cuda:0"), torch.from_numpy(vel0.copy()).to("cuda:0")
    d_age, d_alive = torch.from_numpy(age0.copy()).to("cuda:0"), torch.ones(n, dtype=torch.uint8, device="cuda:0")
    d_T = torch.zeros((n, 16), device="cuda:0")
    d_spawn_pos, d_spawn_vel = torch.from_numpy(spawn_pos).to("cuda:0"), torch.from_numpy(spawn_vel).to("cuda:0")
    tiles, image = torch.zeros(local_tiles * floats_per_tile, device="cuda:0"), torch.zeros(HT * W * 3, device="cuda:0")
    torch.cuda.synchronize()
    st = torch.cuda.Stream(device="cuda:0")
    s = st.cuda_stream
    with torch.cuda.stream(st):
        for frame in range(3):
            if frame == 2:                                  # the spawn: pos, vel, age and the alive byte of a dead slot
                d_pos[slot] = d_spawn_pos
                d_vel[slot] = d_spawn_vel
                d_age[slot] = 5.0
                d_alive[slot] = 1
            pt.particles_step_device(d_pos.data_ptr(), d_vel.data_ptr(), d_age.data_ptr(), n, dt, radius, d_alive.data_ptr(), s)
            pt.particle_transforms_device(d_pos.data_ptr(), n, RDC.PARTICLE_SCALE, d_T.data_ptr(), s)
            pt.set_active_device(pidx, d_alive.data_ptr(), s)
            pt.repose_refit_device(pidx, d_T.data_ptr(), s)
            pt.render_epoch_device(s, SEED, frame, 1, tiles.data_ptr())
        pt.untile_device(s, tiles.data_ptr(), image.data_ptr())
    assert pt.top_refit_pending()[0] == 6                   # six enqueue-only calls, none settled on the way
    st.synchronize()
    got = {"image": image.cpu().numpy().reshape(HT, W, 3), "alive": d_alive.cpu().numpy(), "pos": d_pos.cpu().numpy(), "active": pt.active(),
           "dumps": IC.all_dumps(pt, nobj), "refits": pt.top_refit_count()}
    pt.close()
    # the same frames through the host forms
    ref = make_pt(srt, S)
    pos, vel, age = pos0.copy(), vel0.copy(), age0.copy()
    alive_by_frame = []
    for frame in range(3):
        if frame == 2:
            pos[slot], vel[slot], age[slot] = spawn_pos, spawn_vel, np.float32(5.0)
        pos, vel, age, alive = ref.particles_step(pos, vel, age, dt, radius)
        ref.set_active(pidx, alive)
        ref.repose_refit(pidx, RDC.translate_scale_product(pos, RDC.PARTICLE_SCALE))
        ref_image = ref.render_epoch(SEED, frame, 1)
        alive_by_frame.append(alive.copy())
    want_active, want_dumps = ref.active(), IC.all_dumps(ref, nobj)
    ref.close()
    dead = np.setdiff1d(dying, [slot])
    assert np.all(alive_by_frame[0] == 1) and np.all(alive_by_frame[1][dying] == 0) and int(alive_by_frame[1].sum()) == n - len(dying)
    assert alive_by_frame[2][slot] == 1 and np.all(alive_by_frame[2][dead] == 0)
    assert np.array_equal(got["alive"], alive_by_frame[2]) and bits_equal(got["pos"], pos) and got["refits"] == 3
    assert np.array_equal(got["active"], want_active) and np.array_equal(got["active"][pidx], alive_by_frame[2])
    assert IC.dumps_equal(got["dumps"], want_dumps)
    assert bits_equal(got["image"], ref_image)


def test_pool_of_1200_half_masked(srt, torch):
    """1200 instances of a 12-triangle mesh, every second one off through the device form: levels of more than 256 interior nodes
    (and as many leaves and records for the count kernels).  The boxes are the numpy restatement's, the hits the emulation's."""
    S = A.pool_scene(1200)
    nobj = len(S["objects"])
    off = np.arange(0, nobj, 2, dtype=np.uint32)            # (object 0, the source mesh of every instance, among them)
    want = A.expectation(S, [("active", off, np.zeros(len(off), np.uint8))], samples=False)
    assert C.widest_level(want["dump"][1]) > 256
    d_flags = flags_on_device(torch, np.zeros(len(off), np.uint8))
    pt = make_pt(srt, S)
    first = top_dump(pt, nobj)
    pt.set_active_device(off, d_flags.data_ptr())
    org, d, b = random_rays(A.RAY_SEED, A.RAYS)
    hits = pt.hit(org, d, b)
    got, table = top_dump(pt, nobj), pt.active()
    pt.close()
    assert np.array_equal(got[1], first[1]) and np.array_equal(got[2], first[2]) and not bits_equal(got[0], first[0])
    assert np.array_equal(table, A.flags_of(nobj, off))
    assert bits_equal(got[0], A.expected_boxes(S, table, got[1], got[2])) and top_equal(got, want["dump"])
    assert bits_equal(hits, want["hits"][0]) and np.count_nonzero(hits[:, 0]) > 100


def test_particle_passes_through_an_inactive_object(srt):
    """srt_pt_particles_step: a particle aimed at the blob of IC.sweeps_scene() bounces while the blob is active; with the blob off it
    ends where it ends in a scene committed without the blob - it passes through."""
    S = IC.sweeps_scene()
    box = A.posed_of(S)[UC.BLOB_OBJECT]
    centre = (box[:3] + box[3:]) * np.float32(0.5)
    pos = np.array([[centre[0], centre[1], 0.49]], np.float32)
    vel = np.array([[0.0, 0.0, -2.0]], np.float32)
    age = np.array([1.0], np.float32)
    dt, radius = 0.1, 0.015
    assert 0.49 - 2.0 * dt < box[5] - 0.05                  # the leg ends well inside the blob's box
    pt, absent = make_pt(srt, S), make_pt(srt, A.without(S, [UC.BLOB_OBJECT]))
    bounced = pt.particles_step(pos, vel, age, dt, radius)
    pt.set_active([UC.BLOB_OBJECT], [0])
    through = pt.particles_step(pos, vel, age, dt, radius)
    want = absent.particles_step(pos, vel, age, dt, radius)
    pt.set_active([UC.BLOB_OBJECT], [1])
    again = pt.particles_step(pos, vel, age, dt, radius)
    pt.close(); absent.close()
    assert bits_equal(through[0], want[0]) and bits_equal(through[1], want[1])
    assert bits_equal(through[0], (pos + vel * np.float32(dt)).astype(np.float32))           # one free leg
    assert not bits_equal(bounced[0], through[0]) and bounced[0][0, 2] > through[0][0, 2]    # it did not get as far: the blob was in the way
    assert bits_equal(again[0], bounced[0]) and bits_equal(again[1], bounced[1])


def test_group(srt, torch, wanted):
    """PathtracerGroup.set_active[_device] on a 1-rank group: the single context's image."""
    S, off, _, _ = case("particles")
    want = wanted["particles"]
    grp = srt.PathtracerGroup([0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    grp.set_active(off, np.zeros(len(off), np.uint8))
    hidden = grp.render_epoch(SEED, 0, SPP)
    tables = [m.active() for m in grp.members]
    d_ones = flags_on_device(torch, np.ones(len(off), np.uint8))
    grp.set_active_device(off, [d_ones.data_ptr()])
    back = grp.render_epoch(SEED, 0, SPP)
    d_zeros = flags_on_device(torch, np.zeros(len(off), np.uint8))
    grp.set_active_device(off, [d_zeros.data_ptr()])
    hidden_again = grp.render_epoch(SEED, 0, SPP)
    with pytest.raises(ValueError):
        grp.set_active_device(off, [])
    grp.close()
    single = make_pt(srt, S)
    first = single.render_epoch(SEED, 0, SPP)
    single.close()
    assert bits_equal(hidden, want["epoch"]) and bits_equal(hidden_again, want["epoch"]) and bits_equal(back, first)
    assert all(np.array_equal(t, want["active"]) for t in tables)


PERSIST = ("repose_device", "repose_device of the hidden one", "repose_refit_device of the hidden one", "skin pose of the hidden one",
           "skin pose_refit of the hidden one")


@pytest.mark.parametrize("name", PERSIST)
def test_flags_persist_on_the_device(srt, torch, name):
    """repose_device, repose_refit_device, a skin pose and a skin pose_refit with the blob and a wall hidden, on other objects and on
    the hidden blob: the flags persist, the topology is what the same call gives with every object active, the boxes are the masked
    fold, hiding before the call or after it gives the same scene and the same image, and reactivated the scene is the all-active one."""
    S = IC.sweeps_scene()
    nobj = len(S["objects"])
    off = np.array([UC.BLOB_OBJECT, 2], np.uint32)
    zeros, ones = np.zeros(2, np.uint8), np.ones(2, np.uint8)
    table = A.flags_of(nobj, off)
    idx, Ts = C.sweeps_case(S)
    d_T = torch.from_numpy(np.ascontiguousarray(Ts, np.float32)).to("cuda:0")
    blob_T = np.array([IC.translate(S["objects"][UC.BLOB_OBJECT]["T"], (0.05, 0.1, -0.05))], np.float32)
    d_blob_T = torch.from_numpy(blob_T).to("cuda:0")
    torch.cuda.synchronize()
    g, joints = SC.load_fixture("blob_chain3")
    skins = []

    def call(pt):
        if name == "repose_device":
            pt.repose_device(idx, d_T.data_ptr())
        elif name == "repose_device of the hidden one":
            pt.repose_device([UC.BLOB_OBJECT], d_blob_T.data_ptr())
        elif name == "repose_refit_device of the hidden one":
            pt.repose_refit_device([UC.BLOB_OBJECT], d_blob_T.data_ptr())
        else:
            skins.append(pt.create_skin(UC.BLOB_OBJECT, g["pos"], g["nrm"], joints))
            (skins[-1].pose_refit if "refit" in name else skins[-1].pose)(g["posed"][0])

    a, b, c = make_pt(srt, S), make_pt(srt, S), make_pt(srt, S)
    a.set_active(off, zeros)
    call(a)
    call(b)
    call(c)
    c.set_active(off, zeros)
    da, db, dc = IC.all_dumps(a, nobj), IC.all_dumps(b, nobj), IC.all_dumps(c, nobj)
    assert np.array_equal(a.active(), table)
    assert np.array_equal(da[0][1], db[0][1]) and np.array_equal(da[0][2][:nobj], db[0][2][:nobj]) and IC.dumps_equal(da[1:], db[1:])
    posed = A.posed_from_leaves(db[0][0], db[0][1], db[0][2], nobj)
    assert bits_equal(da[0][0], C.top_boxes_numpy(da[0][1], da[0][2], A.masked(posed, table)))
    assert IC.dumps_equal(da, dc)
    assert bits_equal(a.render_epoch(SEED, 0, SPP), c.render_epoch(SEED, 0, SPP))
    a.set_active(off, ones)
    assert bits_equal(a.render_epoch(SEED, 0, SPP), b.render_epoch(SEED, 0, SPP))
    for s in skins:
        s.close()
    for p in (a, b, c):
        p.close()


def test_no_change_on_success_none_on_refusal(srt, torch):
    """Off and on again through the host form: the epoch equals an untouched context's bit for bit.  Refusals - an emissive mesh and a
    sphere light with dynamic lights on, a duplicate, an index out of range, a NULL pointer - leave the device scene as it was: the
    epoch, the dumps and the upload counter before equal those after, and nothing is pending."""
    L = LC.three_light_scene()
    nl = len(L["objects"])
    pt, untouched = make_pt(srt, L, dynamic=True), make_pt(srt, L, dynamic=True)
    pt.set_active([2, UC.BLOB_OBJECT], [0, 0])
    hidden = pt.render_epoch(SEED, 0, SPP)
    pt.set_active([2, UC.BLOB_OBJECT], [1, 1])
    first = untouched.render_epoch(SEED, 0, SPP)
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), first) and not bits_equal(hidden, first)
    pt.set_active([2], [0])
    image, dumps, counts, table = pt.render_epoch(SEED, 0, SPP), IC.all_dumps(pt, nl), pt.scene_counts(), pt.active()
    d = flags_on_device(torch, np.zeros(2, np.uint8))
    for match, bad in (("area light", [3, LC.CBOX_LIGHT]), ("area light", [9, 3]), ("listed twice", [3, 3]), ("out of range", [nl, 3])):
        for call, name in ((lambda: pt.set_active(bad, [0, 0]), "srt_pt_set_active"), (lambda: pt.set_active_device(bad, d.data_ptr()), "srt_pt_set_active_device")):
            with pytest.raises(srt.SrtError, match=match) as e:
                call()
            assert e.value.status == INVALID and name + ":" in str(e.value)
    with pytest.raises(srt.SrtError, match="NULL argument") as e:
        pt.set_active_device([3, 4], 0)
    assert e.value.status == INVALID
    assert pt.top_refit_pending() == (0, 0) and pt.scene_counts() == counts and np.array_equal(pt.active(), table)
    assert IC.dumps_equal(IC.all_dumps(pt, nl), dumps) and bits_equal(pt.render_epoch(SEED, 0, SPP), image)
    pt.close(); untouched.close()
    one = make_pt(srt, A.one_object_scene())
    image = one.render_epoch(SEED, 0, SPP)
    with pytest.raises(srt.SrtError, match="root of the BVH<Object> is a leaf") as e:
        one.set_active_device([0], d.data_ptr())
    assert e.value.status == UNSUPPORTED and bits_equal(one.render_epoch(SEED, 0, SPP), image)
    one.close()
    lst = make_pt(srt, IC.sweeps_scene(), use_bvh=False)
    with pytest.raises(srt.SrtError, match="without BVHs") as e:
        lst.set_active_device([3], d.data_ptr())
    assert e.value.status == UNSUPPORTED
    lst.close()
    empty = srt.Pathtracer(0)
    with pytest.raises(srt.SrtError, match="before srt_pt_scene_commit") as e:
        empty.set_active_device([3], d.data_ptr())
    assert e.value.status == STATE
    empty.close()
