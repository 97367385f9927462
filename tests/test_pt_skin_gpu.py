"""GPU: srt_pt_skin_* - Skeleton::find_joints once and Skeleton::skin per frame on the device, feeding srt_pt_update_mesh_device.
Everything is bit-exact (outputs compared as uint32 views; where the expected value is NaN, NaN-ness per component - the sign
of a default NaN differs between x86 and the GPU): against results recorded from the reference (tests/golden/skin_*.npz), and,
for cases the recordings do not hold, against the numpy restatement tests/_skin_expected.py, which test_pt_skin_host.py pins to
those recordings."""
import numpy as np
import pytest

import _harness as H
import _instance_cases as IC
import _skin_cases as SC
import _skin_expected as E
import _update_cases as UC
from test_pt_update_gpu import DEPTH, HT, SEED, SPP, W, bits_equal, check_against, make_pt, reference

pytestmark = pytest.mark.gpu

STATE = -5
INVALID = -1


def same(got, want):
    """Bit equality; where `want` is NaN, `got` has to be NaN (any sign, any payload)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


@pytest.fixture(scope="module")
def srt():
    import srt_amd

    return srt_amd


@pytest.fixture(scope="module")
def scenes():
    return IC.scenes_module()


def skin_on_single_mesh(srt, pos, nrm, idx, joints, committed_pos=None):
    """A context whose one object is the mesh, and a skin on it.  committed_pos: other vertices for the commit (the bind arrays are
    create_skin's own arguments; the committed ones may be any frame).  Committed without a BVH: the reference's BVH<Triangle> build
    does not terminate on some of these meshes, and a skin does not read it."""
    S = SC.single_mesh_scene(pos if committed_pos is None else committed_pos, nrm, idx)
    pt = srt.Pathtracer(0)
    pt.set_params(8, 8, 1, 4, False)
    pt.build_scene(S)
    return pt, pt.create_skin(0, pos, nrm, joints)


@pytest.mark.parametrize("name", sorted(SC.rigs()))
def test_fixtures(srt, name):
    """The map and vertices() for both flat_normals settings equal what the reference computed."""
    g, joints = SC.load_fixture(name)
    pt, skin = skin_on_single_mesh(srt, g["pos"], g["nrm"], g["idx"], joints)
    off, jidx, w = skin.map()
    ex = E.find_joints(g["pos"], joints)
    assert skin.counts() == {"vertices": len(g["pos"]), "joints": len(joints), "influences": len(g["jidx"]), "triangles": len(g["idx"]) // 3}
    assert np.array_equal(off, g["off"]) and np.array_equal(jidx, g["jidx"])
    assert bits_equal(w, ex[2])                       # (the reference keeps no weights: the restatement's, pinned through the positions)
    for k, posed in enumerate(g["posed"]):
        p, n = skin.vertices(posed)
        assert bits_equal(p, g["smooth_pos"][k]) and bits_equal(n, g["smooth_nrm"][k]), (name, k, "smooth")
        p, n = skin.vertices(posed, flat_normals=True)
        assert bits_equal(p, g["flat_pos"][k]) and bits_equal(n, g["flat_nrm"][k]), (name, k, "flat")
    skin.close(); pt.close()


# vertex counts 1, 63, 64, 65, 257, 600 (beyond two 256-count blocks of the scan) and 66000 (beyond 256 blocks: the second trip of the
# kernel over the block sums); joint counts 1, 3, 33 and 70 (beyond a wavefront)
EDGE = [(1, 1), (63, 3), (64, 33), (65, 70), (257, 1), (600, 33), (66000, 3)]


@pytest.mark.parametrize("nverts,njoints", EDGE)
def test_edge_meshes(srt, nverts, njoints):
    """_skin_cases.edge_mesh: a vertex with no joint, one at exactly `radius` and one an ulp outside, the three returns of
    closest_on_line_segment, a zero-extent joint, lists of three and more influences, a vertex no triangle names, shared vertices
    and a degenerate triangle."""
    pos, nrm, idx, joints, posed = SC.edge_mesh(nverts, njoints)
    ex = E.expected(pos, nrm, idx, joints, [posed])
    counts = np.diff(ex["off"].astype(np.int64))
    if nverts >= 63:
        assert counts[0] >= 1 and ex["jidx"][ex["off"][0]] == 0                      # at exactly radius: bone 0 is in vertex 0's list
        assert not (ex["jidx"][ex["off"][1]:ex["off"][2]] == 0).any()                # one ulp outside: it is not in vertex 1's
        assert all((ex["jidx"][ex["off"][v]:ex["off"][v + 1]] == 0).any() for v in (2, 3))
        assert counts[5] == 0
        if njoints >= 3:
            assert counts.max() >= 3
            assert (ex["jidx"] == njoints - 1).any()                                    # the zero-extent joint has vertices
        assert np.isnan(ex["frames"][0][1][2]).all()                                    # vertex 2's last triangle is the degenerate one
    committed = np.random.default_rng(5).uniform(-0.5, 0.5, pos.shape).astype(np.float32)
    pt, skin = skin_on_single_mesh(srt, pos, nrm, idx, joints, committed_pos=committed)
    off, jidx, w = skin.map()
    assert np.array_equal(off, ex["off"]) and np.array_equal(jidx, ex["jidx"]) and same(w, ex["w"])
    want_p, want_n = ex["frames"][0]
    assert not np.isnan(want_p).any()
    p, n = skin.vertices(posed)
    assert bits_equal(p, want_p) and bits_equal(n, nrm)
    p, n = skin.vertices(posed, flat_normals=True)
    assert bits_equal(p, want_p) and same(n, want_n)
    assert bits_equal(p[counts == 0], pos[counts == 0])                                # no joint: the bind position
    assert bits_equal(n[-1], nrm[-1]) or nverts < 4                                    # named by no triangle: the bind normal
    skin.close(); pt.close()


def test_vertex_on_a_bone_is_nan(srt):
    """Distance 0: weight inf / inf.  The reference yields NaN positions there and so does vertices().  (Never through pose().)"""
    pos, nrm, idx, joints, posed = SC.edge_mesh(65, 3)
    pos[7] = [0, 0.5, 0]                                                                # ON bone 0
    ex = E.expected(pos, nrm, idx, joints, [posed])
    assert np.isnan(ex["frames"][0][0][7]).all() and not np.isnan(np.delete(ex["frames"][0][0], 7, axis=0)).any()
    committed = np.random.default_rng(5).uniform(-0.5, 0.5, pos.shape).astype(np.float32)
    pt, skin = skin_on_single_mesh(srt, pos, nrm, idx, joints, committed_pos=committed)
    off, jidx, w = skin.map()
    assert np.array_equal(off, ex["off"]) and np.array_equal(jidx, ex["jidx"]) and same(w, ex["w"])
    p, n = skin.vertices(posed, flat_normals=True)
    assert same(p, ex["frames"][0][0]) and same(n, ex["frames"][0][1])
    skin.close(); pt.close()


@pytest.fixture(scope="module")
def blob(scenes):
    """cbox+blob512 and the three-joint chain through the blob: per pose the restatement's arrays (flat normals for the second
    pose) and the oracle's results on scenes.with_vertices of them.  Computed once, left unchanged."""
    S = UC.blob_scene()
    pos, nrm = UC.original(S, UC.BLOB_OBJECT)
    idx = np.ascontiguousarray(S["objects"][UC.BLOB_OBJECT]["idx"], np.uint32)
    joints, poses = SC.blob_chain()
    ex = E.expected(pos, nrm, idx, joints, poses)
    assert np.diff(ex["off"].astype(np.int64)).max() == 3
    arrays = [(ex["frames"][0][0], nrm), (ex["frames"][1][0], ex["frames"][1][1])]
    assert not any(np.isnan(a).any() for pair in arrays for a in pair)
    return {"S": S, "pos": pos, "nrm": nrm, "joints": joints, "poses": poses, "flat": [False, True], "arrays": arrays,
            "refs": [reference(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n)) for p, n in arrays]}


@pytest.mark.parametrize("use_bvh,builder", [(True, (False,)), (True, (True, 1)), (False, None)])
def test_pose_equals_update_mesh_and_the_oracle(srt, scenes, blob, use_bvh, builder):
    """Two poses in turn.  After each, the context equals one that was given update_mesh(index, *skin.vertices(posed)) - samples,
    epoch image, hits, BVH dumps - and the oracle on the restatement's arrays.  builder (True, 1): the device builder takes the mesh."""
    S, nobj = blob["S"], len(blob["S"]["objects"])
    pt = make_pt(srt, S, use_bvh=use_bvh, builder=builder)
    other = make_pt(srt, S, use_bvh=use_bvh, builder=builder)
    skin = pt.create_skin(UC.BLOB_OBJECT, blob["pos"], blob["nrm"], blob["joints"])
    refs = blob["refs"] if use_bvh else [reference(scenes.with_vertices(S, UC.BLOB_OBJECT, p, n), use_bvh=False) for p, n in blob["arrays"]]
    for k, posed in enumerate(blob["poses"]):
        flat = blob["flat"][k]
        p, n = skin.vertices(posed, flat_normals=flat)
        assert bits_equal(p, blob["arrays"][k][0]) and bits_equal(n, blob["arrays"][k][1])
        before = pt.scene_counts()
        skin.pose(posed, flat_normals=flat)
        after = pt.scene_counts()
        assert after["blas_builds"] == before["blas_builds"] + (1 if use_bvh else 0)
        other.update_mesh(UC.BLOB_OBJECT, p, n)
        # (without a BVH only the default kernel form takes the scene: the others walk a BVH<Triangle>)
        check_against(pt, refs[k], (0, 2, 5, 6, 7) if use_bvh else (0,), hit_modes=(0, 5) if use_bvh else (0,))
        rgb, draws, rays = (np.asarray(a) for a in pt.trace_samples(SEED, *_every(W, HT, SPP)))
        rgb2, draws2, rays2 = (np.asarray(a) for a in other.trace_samples(SEED, *_every(W, HT, SPP)))
        assert bits_equal(rgb, rgb2) and np.array_equal(draws, draws2) and np.array_equal(rays, rays2)
        assert bits_equal(pt.render_epoch(SEED, 0, SPP), other.render_epoch(SEED, 0, SPP))
        if use_bvh:                                    # (a scene committed without BVHs has none to dump)
            assert IC.dumps_equal(IC.all_dumps(pt, nobj), IC.all_dumps(other, nobj)), k
    skin.close(); pt.close(); other.close()


def _every(w, h, spp):
    from test_pt_update_gpu import every_sample

    return every_sample(w, h, spp)


def test_an_instance_follows_the_skinned_source(srt, scenes, blob):
    """_instance_cases.sweeps_scene(): object 6 is the blob, the last object an instance of it."""
    S = IC.sweeps_scene()
    pos, nrm = UC.original(S, 6)
    assert bits_equal(pos, blob["pos"])
    pt = make_pt(srt, S)
    skin = pt.create_skin(6, pos, nrm, blob["joints"])
    with pytest.raises(srt.SrtError, match="object 6"):
        pt.create_skin(len(S["objects"]) - 1, pos, nrm, blob["joints"])                  # the instance itself is refused
    skin.pose(blob["poses"][0])
    check_against(pt, reference(scenes.with_vertices(S, 6, *blob["arrays"][0])), (0, 2, 5, 6, 7))
    skin.close(); pt.close()


def test_group(srt, blob):
    S = blob["S"]
    grp = srt.PathtracerGroup([0, 0])
    grp.set_params(W, HT, 1, DEPTH, True)
    grp.build_scene(S)
    grp.set_camera(S["camera"])
    skins = grp.create_skin(UC.BLOB_OBJECT, blob["pos"], blob["nrm"], blob["joints"])
    assert len(skins.skins) == 2
    images = []
    for k, posed in enumerate(blob["poses"]):
        skins.pose(posed, flat_normals=blob["flat"][k])
        images.append(grp.render_epoch(SEED, 0, SPP))
    counts = grp.scene_counts()
    skins.close(); grp.close()
    assert all(bits_equal(images[k], blob["refs"][k]["epoch"]) for k in range(2)) and counts[0] == counts[1]


def test_failures_leave_the_committed_scene_as_it_was(srt, blob):
    """A skin on an area light is refused at creation; a stale skin (its context committed again) is refused by every call; renders
    of the committed scene are bit-identical to before in both cases."""
    S = blob["S"]
    light = [k for k, o in enumerate(S["objects"]) if o["kind"] == "mesh" and o.get("is_light")][0]
    pt = make_pt(srt, S)
    first = pt.render_epoch(SEED, 0, SPP)
    with pytest.raises(srt.SrtError, match="area light") as e:
        pt.create_skin(light, *UC.original(S, light), blob["joints"])
    assert e.value.status == INVALID
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), first)
    skin = pt.create_skin(UC.BLOB_OBJECT, blob["pos"], blob["nrm"], blob["joints"])
    pt.build_scene(S)                                                                   # the scene is committed again: the skin is stale
    for call in (lambda: skin.pose(blob["poses"][0]), lambda: skin.vertices(blob["poses"][0]), skin.map):
        with pytest.raises(srt.SrtError, match="stale") as e:
            call()
        assert e.value.status == STATE
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), first)
    fresh = pt.create_skin(UC.BLOB_OBJECT, blob["pos"], blob["nrm"], blob["joints"])       # a new skin on the new commit works
    fresh.pose(blob["poses"][0])
    assert bits_equal(pt.render_epoch(SEED, 0, SPP), blob["refs"][0]["epoch"])
    skin.close(); fresh.close(); pt.close()
