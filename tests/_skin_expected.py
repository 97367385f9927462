"""float32 numpy restatement of the reference's skinning, for the tests that have no reference at hand (the GPU machine):
Skeleton::find_joints (student/skeleton.cpp:219-256) with closest_on_line_segment (:195-217), Skeleton::skin (:258-307), the
flat-normal loop of Scene_Object::sync_anim_mesh (scene/object.cpp:114-126), and the two matrix routines they go through,
Mat4::inverse (lib/mat4.h:299-351) and Mat4::operator* (:136-147).  In the style of _normals_expected.py: every operator is one
numpy float32 operation - one rounding each, nothing fused - and sums associate as the reference's expressions do.
test_pt_skin_host.py pins it bit for bit to results recorded from the reference (tests/golden/skin_*.npz).

Matrices are Mat4::data: 16 floats, column-major (m[c][r] below is cols[c][r]).  Joints are SKIN_JOINT_DTYPE records in
Skeleton::for_joints order."""
import numpy as np

F = np.float32
JOINT_DTYPE = np.dtype([("bind", np.float32, 16), ("extent", np.float32, 3), ("radius", np.float32)])


def mat4_inverse(m16):
    """Mat4::inverse: the sixteen cofactor sums, then sixteen divisions by det()."""
    m = [[F(m16[4 * c + k]) for k in range(4)] for c in range(4)]
    r = [[F(0)] * 4 for _ in range(4)]
    with np.errstate(all="ignore"):
        r[0][0] = m[1][2] * m[2][3] * m[3][1] - m[1][3] * m[2][2] * m[3][1] + m[1][3] * m[2][1] * m[3][2] - m[1][1] * m[2][3] * m[3][2] - m[1][2] * m[2][1] * m[3][3] + m[1][1] * m[2][2] * m[3][3]
        r[0][1] = m[0][3] * m[2][2] * m[3][1] - m[0][2] * m[2][3] * m[3][1] - m[0][3] * m[2][1] * m[3][2] + m[0][1] * m[2][3] * m[3][2] + m[0][2] * m[2][1] * m[3][3] - m[0][1] * m[2][2] * m[3][3]
        r[0][2] = m[0][2] * m[1][3] * m[3][1] - m[0][3] * m[1][2] * m[3][1] + m[0][3] * m[1][1] * m[3][2] - m[0][1] * m[1][3] * m[3][2] - m[0][2] * m[1][1] * m[3][3] + m[0][1] * m[1][2] * m[3][3]
        r[0][3] = m[0][3] * m[1][2] * m[2][1] - m[0][2] * m[1][3] * m[2][1] - m[0][3] * m[1][1] * m[2][2] + m[0][1] * m[1][3] * m[2][2] + m[0][2] * m[1][1] * m[2][3] - m[0][1] * m[1][2] * m[2][3]
        r[1][0] = m[1][3] * m[2][2] * m[3][0] - m[1][2] * m[2][3] * m[3][0] - m[1][3] * m[2][0] * m[3][2] + m[1][0] * m[2][3] * m[3][2] + m[1][2] * m[2][0] * m[3][3] - m[1][0] * m[2][2] * m[3][3]
        r[1][1] = m[0][2] * m[2][3] * m[3][0] - m[0][3] * m[2][2] * m[3][0] + m[0][3] * m[2][0] * m[3][2] - m[0][0] * m[2][3] * m[3][2] - m[0][2] * m[2][0] * m[3][3] + m[0][0] * m[2][2] * m[3][3]
        r[1][2] = m[0][3] * m[1][2] * m[3][0] - m[0][2] * m[1][3] * m[3][0] - m[0][3] * m[1][0] * m[3][2] + m[0][0] * m[1][3] * m[3][2] + m[0][2] * m[1][0] * m[3][3] - m[0][0] * m[1][2] * m[3][3]
        r[1][3] = m[0][2] * m[1][3] * m[2][0] - m[0][3] * m[1][2] * m[2][0] + m[0][3] * m[1][0] * m[2][2] - m[0][0] * m[1][3] * m[2][2] - m[0][2] * m[1][0] * m[2][3] + m[0][0] * m[1][2] * m[2][3]
        r[2][0] = m[1][1] * m[2][3] * m[3][0] - m[1][3] * m[2][1] * m[3][0] + m[1][3] * m[2][0] * m[3][1] - m[1][0] * m[2][3] * m[3][1] - m[1][1] * m[2][0] * m[3][3] + m[1][0] * m[2][1] * m[3][3]
        r[2][1] = m[0][3] * m[2][1] * m[3][0] - m[0][1] * m[2][3] * m[3][0] - m[0][3] * m[2][0] * m[3][1] + m[0][0] * m[2][3] * m[3][1] + m[0][1] * m[2][0] * m[3][3] - m[0][0] * m[2][1] * m[3][3]
        r[2][2] = m[0][1] * m[1][3] * m[3][0] - m[0][3] * m[1][1] * m[3][0] + m[0][3] * m[1][0] * m[3][1] - m[0][0] * m[1][3] * m[3][1] - m[0][1] * m[1][0] * m[3][3] + m[0][0] * m[1][1] * m[3][3]
        r[2][3] = m[0][3] * m[1][1] * m[2][0] - m[0][1] * m[1][3] * m[2][0] - m[0][3] * m[1][0] * m[2][1] + m[0][0] * m[1][3] * m[2][1] + m[0][1] * m[1][0] * m[2][3] - m[0][0] * m[1][1] * m[2][3]
        r[3][0] = m[1][2] * m[2][1] * m[3][0] - m[1][1] * m[2][2] * m[3][0] - m[1][2] * m[2][0] * m[3][1] + m[1][0] * m[2][2] * m[3][1] + m[1][1] * m[2][0] * m[3][2] - m[1][0] * m[2][1] * m[3][2]
        r[3][1] = m[0][1] * m[2][2] * m[3][0] - m[0][2] * m[2][1] * m[3][0] + m[0][2] * m[2][0] * m[3][1] - m[0][0] * m[2][2] * m[3][1] - m[0][1] * m[2][0] * m[3][2] + m[0][0] * m[2][1] * m[3][2]
        r[3][2] = m[0][2] * m[1][1] * m[3][0] - m[0][1] * m[1][2] * m[3][0] - m[0][2] * m[1][0] * m[3][1] + m[0][0] * m[1][2] * m[3][1] + m[0][1] * m[1][0] * m[3][2] - m[0][0] * m[1][1] * m[3][2]
        r[3][3] = m[0][1] * m[1][2] * m[2][0] - m[0][2] * m[1][1] * m[2][0] + m[0][2] * m[1][0] * m[2][1] - m[0][0] * m[1][2] * m[2][1] - m[0][1] * m[1][0] * m[2][2] + m[0][0] * m[1][1] * m[2][2]
        det = (m[0][3] * m[1][2] * m[2][1] * m[3][0]
               - m[0][2] * m[1][3] * m[2][1] * m[3][0] - m[0][3] * m[1][1] * m[2][2] * m[3][0]
               + m[0][1] * m[1][3] * m[2][2] * m[3][0] + m[0][2] * m[1][1] * m[2][3] * m[3][0]
               - m[0][1] * m[1][2] * m[2][3] * m[3][0] - m[0][3] * m[1][2] * m[2][0] * m[3][1]
               + m[0][2] * m[1][3] * m[2][0] * m[3][1] + m[0][3] * m[1][0] * m[2][2] * m[3][1]
               - m[0][0] * m[1][3] * m[2][2] * m[3][1] - m[0][2] * m[1][0] * m[2][3] * m[3][1]
               + m[0][0] * m[1][2] * m[2][3] * m[3][1] + m[0][3] * m[1][1] * m[2][0] * m[3][2]
               - m[0][1] * m[1][3] * m[2][0] * m[3][2] - m[0][3] * m[1][0] * m[2][1] * m[3][2]
               + m[0][0] * m[1][3] * m[2][1] * m[3][2] + m[0][1] * m[1][0] * m[2][3] * m[3][2]
               - m[0][0] * m[1][1] * m[2][3] * m[3][2] - m[0][2] * m[1][1] * m[2][0] * m[3][3]
               + m[0][1] * m[1][2] * m[2][0] * m[3][3] + m[0][2] * m[1][0] * m[2][1] * m[3][3]
               - m[0][0] * m[1][2] * m[2][1] * m[3][3] - m[0][1] * m[1][0] * m[2][2] * m[3][3]
               + m[0][0] * m[1][1] * m[2][2] * m[3][3])
        return np.array([r[c][k] / det for c in range(4) for k in range(4)], F)


def mat4_mul(a16, b16):
    """Mat4::operator*, a * b: ret[i][j] = sum over k, from 0.0f, of b[i][k] * a[k][j]."""
    out = np.zeros(16, F)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                s = F(0)
                for k in range(4):
                    s = F(s + F(F(b16[4 * i + k]) * F(a16[4 * k + j])))
                out[4 * i + j] = s
    return out


def mat_point(m16, P):
    """Mat4 * Vec3 for every row of P: v0 col0 + v1 col1 + v2 col2 + 1.0f col3, then Vec4::project."""
    m = np.asarray(m16, F)
    r = [((P[:, 0] * m[a] + P[:, 1] * m[4 + a]) + P[:, 2] * m[8 + a]) + F(1) * m[12 + a] for a in range(4)]
    return np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def closest_on_line_segment(start, end, P):
    """closest_on_line_segment as written: `<= 0` gives start, the projection is ((dot / norm) * v) / norm, the end test is on squared
    norms, and the last return is proj (not start + proj)."""
    start, end = np.asarray(start, F), np.asarray(end, F)
    start_p = (P - start).astype(F)
    start_end = (end - start).astype(F)
    d = _dot(start_p, start_end[None, :])
    n = np.sqrt(_dot(start_end, start_end))
    s = d / n
    proj = ((start_end[None, :] * s[:, None]) / n).astype(F)
    out = np.where((_dot(proj, proj) > _dot(start_end, start_end))[:, None], end[None, :], proj)
    return np.where((d <= 0)[:, None], start[None, :], out).astype(F)


def bone_distances(pos, joints):
    """[nverts, njoints]: the distance find_joints compares with Joint::radius and skin inverts."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    out = np.zeros((len(pos), len(joints)), F)
    with np.errstate(all="ignore"):
        for j, J in enumerate(joints):
            p = mat_point(mat4_inverse(J["bind"]), pos)
            end = (F(0) + np.asarray(J["extent"], F)).astype(F)
            diff = (p - closest_on_line_segment(np.zeros(3, F), end, p)).astype(F)
            out[:, j] = np.sqrt(_dot(diff, diff))
    return out


def find_joints(pos, joints):
    """(offsets[nverts + 1], joints[n], weights[n], inside[nverts, njoints], weight matrix): the CSR map with skin's weights
    (1.0f / distance) / sum_of_inv_dis, the sum taken from 0.0f in list order."""
    dist = bone_distances(pos, joints)
    radius = np.array([J["radius"] for J in joints], F)
    with np.errstate(all="ignore"):
        inside = dist <= radius[None, :]
        inv_dist = (F(1) / dist).astype(F)
        total = np.zeros(len(dist), F)
        for j in range(len(joints)):
            total = np.where(inside[:, j], total + inv_dist[:, j], total).astype(F)
        W = (inv_dist / total[:, None]).astype(F)
    off = np.zeros(len(dist) + 1, np.uint32)
    off[1:] = np.cumsum(inside.sum(axis=1))
    v, j = np.nonzero(inside)                      # row-major: vertex by vertex, joints ascending
    return off, j.astype(np.uint32), W[v, j].astype(F), inside, W


def skin(pos, joints, posed, inside=None, W=None):
    """Skeleton::skin: sum, from Vec3{0} in list order, of w_ij * ((posed_j * inverse(bind_j)) * pos); no joint: the bind position."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    posed = np.ascontiguousarray(posed, F).reshape(-1, 16)
    if inside is None:
        _, _, _, inside, W = find_joints(pos, joints)
    out = np.zeros_like(pos)
    with np.errstate(all="ignore"):
        for j, J in enumerate(joints):
            p = mat_point(mat4_mul(posed[j], mat4_inverse(J["bind"])), pos)
            out = np.where(inside[:, j][:, None], out + p * W[:, j][:, None], out).astype(F)
    return np.where(inside.any(axis=1)[:, None], out, pos).astype(F)


def flat_normals(pos, bind_nrm, idx):
    """sync_anim_mesh without smooth normals: every triangle in index order writes cross(v1 - v0, v2 - v0).unit() to its three
    vertices - a vertex ends with the normal of the last triangle that names it, its bind normal when none does."""
    pos, bind_nrm = np.ascontiguousarray(pos, F).reshape(-1, 3), np.ascontiguousarray(bind_nrm, F).reshape(-1, 3)
    tri = np.ascontiguousarray(idx, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        l = (pos[tri[:, 1]] - pos[tri[:, 0]]).astype(F)
        r = (pos[tri[:, 2]] - pos[tri[:, 0]]).astype(F)
        c = np.stack([l[:, 1] * r[:, 2] - l[:, 2] * r[:, 1], l[:, 2] * r[:, 0] - l[:, 0] * r[:, 2], l[:, 0] * r[:, 1] - l[:, 1] * r[:, 0]], axis=1).astype(F)
        n = (c / np.sqrt(_dot(c, c))[:, None]).astype(F)
    last = np.full(len(pos), -1, np.int64)
    np.maximum.at(last, tri.reshape(-1), np.repeat(np.arange(len(tri)), 3))
    return np.where((last >= 0)[:, None], n[np.maximum(last, 0)] if len(tri) else bind_nrm, bind_nrm).astype(F)


def expected(pos, nrm, idx, joints, posed_list):
    """Everything the GPU tests compare with: the map, and per pose the skinned positions and the flat normals."""
    off, jidx, w, inside, W = find_joints(pos, joints)
    frames = []
    for posed in posed_list:
        p = skin(pos, joints, posed, inside, W)
        frames.append((p, flat_normals(p, nrm, idx)))
    return {"off": off, "jidx": jidx, "w": w, "frames": frames}
