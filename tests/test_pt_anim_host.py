"""CPU: the Animate mode's timeline on the host side - srt_pt_timeline_transforms through the ABI on a host-only context and the rig
evaluation srt_pt_skin_posed runs (srt_pt_rig_posed_host: a host-only context has no skins) against what the reference recorded
(tests/golden/anim_*.npz), bit for bit; the intermediate poses through the host emulation of pt_anim.h
(tests/host_emu/anim_host.cpp); joint_to_posed for the Euler angles of the committed skin fixtures; srt_hypotf against this host's
libm; every refusal, each with the scene left as it was; and a sanitized stand-alone program over the check, the packing and the
evaluation.  Every comparison is on float32 viewed as uint32, NaN matching NaN; there are no tolerances."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _anim_cases as AC
import _harness as H
import _instance_cases as IC
import _skin_cases as SC

F = np.float32
INVALID, UNSUPPORTED, STATE = -1, -4, -5


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def objects():
    return AC.load_objects()


@pytest.fixture(scope="module")
def scene():
    return IC.particles_shared()[0]


def last_error(srt):
    return srt.load_library().srt_last_error().decode("utf-8", "replace")


def host_pt(srt, scene):
    pt = srt.Pathtracer(device=-1)
    pt.set_params(8, 8, 1, 8, True)
    pt.build_scene(scene)
    return pt


def particle_list(n):
    """n objects of the particle scene a timeline may list: particles first, then the two spheres behind them."""
    return np.arange(IC.PARTICLE_FIRST, IC.PARTICLE_FIRST + n, dtype=np.uint32)


def test_abi_and_bindings(srt):
    lib = srt.load_library()
    names = ("srt_pt_timeline_create", "srt_pt_timeline_destroy", "srt_pt_timeline_transforms", "srt_pt_timeline_transforms_device", "srt_pt_timeline_repose_refit",
             "srt_pt_timeline_repose", "srt_pt_skin_set_rig", "srt_pt_skin_posed", "srt_pt_skin_posed_device", "srt_pt_skin_vertices_at_device", "srt_pt_skin_pose_at",
             "srt_pt_skin_pose_refit_at")
    text = open(os.path.join(H.ROOT, "include", "srt_pt.h")).read()
    for name in names:
        assert getattr(lib, name) is not None and name + "(" in text, name
    for cls, methods in ((srt.Pathtracer, ("create_timeline",)), (srt.Timeline, ("transforms", "transforms_device", "repose_refit", "repose", "close")),
                         (srt.Skin, ("set_rig", "posed_at", "pose_at", "pose_refit_at")), (srt.PathtracerGroup, ("create_timeline",)),
                         (srt.SkinGroup, ("set_rig", "pose_at", "pose_refit_at")), (srt.TimelineGroup, ("repose_refit", "repose"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)


def test_fixture_holds_the_cases(objects):
    """What make_anim_golden.py asserted when it recorded, checked again on the committed file."""
    off = objects["track_offsets"]
    counts = np.diff(off).reshape(-1, 3)
    assert len(counts) == AC.NOBJECTS == 70 and np.array_equal(objects["times"], AC.TIMES)
    assert all(set(counts[:, i]) >= {0, 1, 2, 3, 6} for i in range(3)) and {1, 2, 3} <= set((counts > 0).sum(axis=1))
    rebuilt = AC.object_tracks()
    assert np.array_equal(rebuilt[0], off) and AC.bits_equal(rebuilt[1], objects["knot_times"]) and AC.bits_equal(rebuilt[2], objects["knot_values"])
    pose = objects["pose"]
    assert np.all(pose[:, AC.PITCH_UP, 5] == 0) and np.all(np.abs(pose[:, AC.PITCH_DOWN, 4] + 90) < 0.05) and np.all(np.abs(pose[:, AC.SECOND_SOLUTION, 4]) > 90)
    assert np.isnan(objects["trans"][:, AC.ZERO]).any() and np.all(pose[:, counts[:, 2] == 0, 6:9] == 0)
    for name in AC.RIGS:
        g = AC.load_rig(name)
        keyed = np.diff(g["knot_offsets"]) > 0
        assert keyed.any() and (~keyed).any() and np.array_equal(g["times"], AC.TIMES)


def test_timeline_transforms_equal_the_reference(srt, objects, scene):
    """All 70 recorded objects at every time, through srt_pt_timeline_transforms on a host-only context."""
    pt = host_pt(srt, scene)
    idx = np.array([k for k, o in enumerate(scene["objects"]) if not o.get("is_light")][:AC.NOBJECTS], np.uint32)   # walls, spheres, particles: any 70 that are no light
    assert len(idx) == AC.NOBJECTS
    tl = pt.create_timeline(idx, (objects["track_offsets"], objects["knot_times"], objects["knot_values"]))
    bad = {float(t): AC.mismatches(tl.transforms(t), objects["trans"][i]) for i, t in enumerate(objects["times"])}
    tl.close()
    pt.close()
    assert not any(bad.values()), bad


def test_intermediate_poses_equal_the_reference(objects):
    """Position, Euler angles (degrees) and scale of Anim_Pose::at, and the matrices, from the host emulation of pt_anim.h."""
    bad = {}
    for i, t in enumerate(objects["times"]):
        pose, trans = AC.emu_objects(objects["track_offsets"], objects["knot_times"], objects["knot_values"], t)
        bad[float(t)] = (AC.mismatches(pose, objects["pose"][i]), AC.mismatches(trans, objects["trans"][i]))
    assert not any(a or b for a, b in bad.values()), bad


@pytest.mark.parametrize("name", AC.RIGS)
def test_rig_posed_equals_the_reference(srt, name):
    """Skeleton::set_time + joint_to_posed: the library's host form (what srt_pt_skin_posed runs) and the emulation, Euler angles included."""
    lib, g = srt.load_library(), AC.load_rig(name)
    parent, extent, base, rest, koff, ktimes, kquats = AC.rig_arrays(g)
    nj, bad = len(parent), {}
    for i, t in enumerate(g["times"]):
        euler, posed = np.zeros((nj, 3), F), np.zeros((nj, 16), F)
        assert lib.srt_pt_rig_posed_host(nj, H.P(parent), H.P(extent), H.P(base), H.P(rest), H.P(koff), H.P(ktimes), H.P(kquats), float(t), H.P(euler), H.P(posed)) == 0
        e_euler, e_posed = AC.emu_rig(parent, extent, base, rest, koff, ktimes, kquats, t)
        bad[float(t)] = (AC.mismatches(euler, g["euler"][i]), AC.mismatches(posed, g["posed"][i]), AC.mismatches(e_euler, g["euler"][i]), AC.mismatches(e_posed, g["posed"][i]))
    assert not any(any(v) for v in bad.values()), bad


@pytest.mark.parametrize("name", AC.RIGS)
def test_joint_to_posed_of_the_committed_skin_fixtures(name):
    """The `posed` arrays of tests/golden/skin_*.npz are joint_to_posed for known Euler angles: a check that needs no new fixture."""
    rig, g = SC.rigs()[name], np.load(os.path.join(H.GOLDEN, f"skin_{name}.npz"))
    order = g["order"]
    inv = np.zeros(len(order), np.int64)
    inv[order] = np.arange(len(order))
    parent = np.array([-1 if rig["parent"][j] < 0 else inv[rig["parent"][j]] for j in order], np.int32)
    extent, base = np.ascontiguousarray(g["extent"], F), np.array(rig["base"], F)
    for p, angles in enumerate(rig["poses"]):
        euler = np.ascontiguousarray(np.array(angles, F)[order])
        posed = np.zeros((len(order), 16), F)
        AC.anim_emu().anim_emu_posed_of_euler(H.P(parent), H.P(extent), H.P(base), H.P(euler), len(order), H.P(posed))
        assert AC.mismatches(posed, g["posed"][p]) == 0, (name, p)


def test_hypotf_equals_libm():
    """srt_hypotf restates glibc 2.35's __hypotf: bit-identical to this host's libm on 1.2e7 arguments - random bit patterns (NaNs,
    infinities, denormals) and the renderer's range (matrix entries) - and on the corners."""
    emu = AC.anim_emu()
    first = np.zeros(2, np.uint32)
    for mode, count in ((0, 8_000_000), (1, 4_000_000)):
        bad = emu.anim_emu_hypot_sweep(0x9E3779B97F4A7C15 + mode, count, mode, H.P(first))
        assert bad == 0, (mode, bad, [hex(v) for v in first])
    corners = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, 1.17549435e-38, 2.0 ** -75, 2.0 ** 64], F)
    snan = np.array([0x7fa00000], np.uint32).view(F)
    x, y = (np.ascontiguousarray(a.reshape(-1)) for a in np.meshgrid(np.concatenate([corners, snan]), np.concatenate([corners, snan])))
    out = np.zeros(len(x), F)
    emu.anim_emu_hypot(H.P(x), H.P(y), ctypes.c_uint64(len(x)), H.P(out))
    want = np.zeros(len(x), F)
    emu.anim_emu_hypot_libm(H.P(x), H.P(y), ctypes.c_uint64(len(x)), H.P(want))
    assert np.isinf(want[(np.isinf(x) | np.isinf(y)) & ~(x.view(np.uint32) == 0x7fa00000) & ~(y.view(np.uint32) == 0x7fa00000)]).all()
    assert AC.bits_equal(out, want)


def _scene_state(pt, nobj):
    return IC.all_dumps(pt, nobj), pt.scene_tree_cost(), pt.scene_counts()


def test_refusals_leave_the_scene_alone(srt, objects, scene):
    """Every refusal of srt_pt_timeline_create, the stale timeline, the device forms on a host-only context."""
    lib = srt.load_library()
    nobj = len(scene["objects"])
    pt = host_pt(srt, scene)
    before = _scene_state(pt, nobj)
    two = particle_list(2)
    off = np.array([0, 2, 3, 4, 4, 6, 6], np.uint32)
    times, values = np.array([0.0, 1.0, 0.0, 0.5, 0.0, 2.0], F), np.ones((6, 4), F)
    h = ctypes.c_void_p()

    def create(idx=two, n=2, off=off, times=times, values=values, ctx=None, out=h):
        return lib.srt_pt_timeline_create(pt._ctx if ctx is None else ctx, None if idx is None else H.P(idx), n, None if off is None else H.P(off),
                                          None if times is None else H.P(times), None if values is None else H.P(values), None if out is None else ctypes.byref(out))

    assert create(ctx=ctypes.c_void_p()) == INVALID and create(idx=None) == INVALID and create(off=None) == INVALID
    assert create(times=None) == INVALID and create(values=None) == INVALID and create(out=None) == INVALID
    assert create(idx=np.array([IC.PARTICLE_FIRST, nobj], np.uint32)) == INVALID                          # out of range
    assert create(idx=np.array([IC.PARTICLE_FIRST, IC.PARTICLE_FIRST], np.uint32)) == INVALID             # listed twice
    light = [k for k, o in enumerate(scene["objects"]) if o.get("is_light")][0]
    assert create(idx=np.array([IC.PARTICLE_FIRST, light], np.uint32)) == INVALID                         # an area light, srt_pt_repose's rule
    assert "light" in last_error(srt).lower()
    for bad_times in ([0.0, 0.0, 0.0, 0.5, 0.0, 2.0], [1.0, 0.0, 0.0, 0.5, 0.0, 2.0], [0.0, np.nan, 0.0, 0.5, 0.0, 2.0], [0.0, np.inf, 0.0, 0.5, 0.0, 2.0]):
        assert create(times=np.array(bad_times, F)) == INVALID, bad_times
    assert create(off=np.array([0, 2, 3, 4, 4, 4, 4], np.uint32)) == INVALID                              # object 1 has no key at all
    assert "any()" in last_error(srt)
    assert create(off=np.array([1, 2, 3, 4, 4, 6, 6], np.uint32)) == INVALID and create(off=np.array([0, 3, 2, 4, 4, 6, 6], np.uint32)) == INVALID
    assert not h.value
    with pytest.raises(srt.SrtError) as e:
        pt.create_timeline(two, [(((0.0, 1.0), np.zeros((2, 3))), None, None), (None, None, None)])      # the bindings' per-object form
    assert e.value.status == INVALID
    assert IC.dumps_equal(_scene_state(pt, nobj)[0], before[0]) and _scene_state(pt, nobj)[1:] == before[1:]
    # a valid one: the device forms are refused after validation, the host form works, NaN and infinite knot VALUES are not checked
    values[1] = np.nan
    assert create() == 0 and h.value
    tl = srt.Timeline(pt, h, two)
    d = ctypes.c_void_p(64)                                 # (never dereferenced: the call is refused before anything is enqueued)
    assert lib.srt_pt_timeline_transforms_device(tl._h, None, 0.5, d) == UNSUPPORTED and "host-only" in last_error(srt)
    assert lib.srt_pt_timeline_repose_refit(tl._h, None, 0.5) == UNSUPPORTED and lib.srt_pt_timeline_repose(tl._h, None, 0.5) == UNSUPPORTED
    assert lib.srt_pt_timeline_transforms_device(None, None, 0.5, d) == INVALID and lib.srt_pt_timeline_transforms_device(tl._h, None, 0.5, None) == INVALID
    assert lib.srt_pt_timeline_transforms(tl._h, 0.5, None) == INVALID and lib.srt_pt_timeline_transforms(None, 0.5, d) == INVALID
    assert lib.srt_pt_timeline_repose_refit(None, None, 0.5) == INVALID and lib.srt_pt_timeline_repose(None, None, 0.5) == INVALID
    assert tl.transforms(0.5).shape == (2, 16)
    assert IC.dumps_equal(_scene_state(pt, nobj)[0], before[0]) and _scene_state(pt, nobj)[1:] == before[1:]
    # stale: the scene was committed again
    pt.build_scene(scene)
    out = np.zeros((2, 16), F)
    assert lib.srt_pt_timeline_transforms(tl._h, 0.5, H.P(out)) == STATE and "stale" in last_error(srt)
    assert lib.srt_pt_timeline_transforms_device(tl._h, None, 0.5, d) == STATE and lib.srt_pt_timeline_repose_refit(tl._h, None, 0.5) == STATE
    assert lib.srt_pt_timeline_repose(tl._h, None, 0.5) == STATE
    tl.close()
    assert lib.srt_pt_timeline_destroy(None) == 0
    # no committed scene at all
    fresh = srt.Pathtracer(device=-1)
    assert create(ctx=fresh._ctx) == STATE
    fresh.close()
    pt.close()


def test_closing_the_context_closes_its_timelines(srt, objects, scene):
    """Pathtracer.close() destroys the timelines it created before the context goes; a close() after it does nothing."""
    pt = host_pt(srt, scene)
    two = particle_list(2)
    tracks = [(((0.0, 1.0), np.zeros((2, 3))), None, None), (None, ((0.5,), np.array([[0, 0, 0, 1]], F)), None)]
    a, b = pt.create_timeline(two, tracks), pt.create_timeline(two, tracks)
    a.close()
    assert not a._h and b._h and len(pt._timelines) == 2
    pt.close()
    assert not b._h
    b.close(); a.close()


def test_rig_refusals(srt):
    """What srt_pt_skin_set_rig refuses (through srt_pt_rig_posed_host: the same check), and the NULL skin of every skin entry point."""
    lib, g = srt.load_library(), AC.load_rig("blob128_tree5")
    parent, extent, base, rest, koff, ktimes, kquats = AC.rig_arrays(g)
    nj = len(parent)
    posed = np.zeros((nj, 16), F)

    def run(parent=parent, koff=koff, ktimes=ktimes, rest=rest, out=posed):
        return lib.srt_pt_rig_posed_host(nj, None if parent is None else H.P(parent), H.P(extent), H.P(base), None if rest is None else H.P(rest), H.P(koff), H.P(ktimes),
                                         H.P(kquats), 0.5, None, None if out is None else H.P(out))

    assert run() == 0
    assert run(parent=None) == INVALID and run(rest=None) == INVALID and run(out=None) == INVALID
    for j, p in ((0, 0), (1, 1), (1, 3), (2, -2)):                                                        # itself, behind it, below -1
        bad = parent.copy()
        bad[j] = p
        assert run(parent=bad) == INVALID and "parent" in last_error(srt), (j, p)
    down = koff.copy()
    down[1], down[2] = down[2] + 1, down[1]
    assert run(koff=np.ascontiguousarray(down)) == INVALID
    late = koff.copy()
    late[0] = 1
    assert run(koff=late) == INVALID
    keyed = int(np.nonzero(np.diff(koff) >= 2)[0][0])
    for v in (np.nan, np.inf, ktimes[koff[keyed]]):
        t = ktimes.copy()
        t[koff[keyed] + 1] = v
        assert run(ktimes=t) == INVALID, v
    d = ctypes.c_void_p(64)
    assert lib.srt_pt_skin_set_rig(None, H.P(parent), H.P(base), H.P(rest), H.P(koff), H.P(ktimes), H.P(kquats)) == INVALID
    assert lib.srt_pt_skin_posed(None, 0.5, H.P(posed)) == INVALID and lib.srt_pt_skin_posed_device(None, None, 0.5, d) == INVALID
    assert lib.srt_pt_skin_vertices_at_device(None, None, 0.5, 0, d, d) == INVALID
    assert lib.srt_pt_skin_pose_at(None, None, 0.5, 0) == INVALID and lib.srt_pt_skin_pose_refit_at(None, None, 0.5, 0) == INVALID


def _flat_file(path, objects):
    with open(path, "wb") as f:
        n, nt, nk = AC.NOBJECTS, len(objects["times"]), len(objects["knot_times"])
        np.array([n, nt, nk], np.uint32).tofile(f)
        for a, t in ((objects["track_offsets"], np.uint32), (objects["knot_times"], F), (objects["knot_values"], F), (objects["times"], F), (objects["trans"], F)):
            np.ascontiguousarray(a, t).tofile(f)
        np.array([len(AC.RIGS)], np.uint32).tofile(f)
        for name in AC.RIGS:
            g = AC.load_rig(name)
            parent, extent, base, rest, koff, ktimes, kquats = AC.rig_arrays(g)
            np.array([len(parent), len(ktimes)], np.uint32).tofile(f)
            for a in (parent, extent, base, rest, koff, ktimes, kquats, np.ascontiguousarray(g["posed"], F)):
                a.tofile(f)


def test_sanitized_program(objects, tmp_path):
    """-fsanitize=address,undefined over the table check, the packing and the host evaluation: the fixtures, NaN and infinite times,
    malformed offset arrays, a hierarchy that does not end.  A program of its own, run as its own process."""
    exe = AC.sanitized_program()
    path = str(tmp_path / "anim.bin")
    _flat_file(path, objects)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "anim_sanitized: ok" in run.stdout and "ACCEPTED" not in run.stdout, run.stdout[-3000:] + run.stderr[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
