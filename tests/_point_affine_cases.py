"""Matrices and points for the leaf section's point transform (mat_point_affine, csrc/pt_device.h), shared by
tests/test_pt_point_affine_host.py and tests/test_pt_point_affine_gpu.py: one matrix per wave of 64 lanes, one point per lane."""
import numpy as np

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
KINDS = ("affine", "affine_negative_zeros", "w2", "perspective", "one_lane_inf", "one_lane_nan", "row0_overflows", "affine_infinite_entry")


def cases(seed, waves):
    """-> dict(mats (W, 16) as Mat4::data (column-major), points (W * 64, 3), kind (W,) index into KINDS, skips (W,) bool: the waves
    that may leave w out - an affine bottom row and a finite first output row in every lane)."""
    rng = np.random.default_rng(seed)
    mats = np.zeros((waves, 4, 4), np.float32)          # [col][row]
    points = rng.uniform(-4, 4, (waves, 64, 3)).astype(np.float32)
    kind = np.arange(waves) % len(KINDS)
    for w in range(waves):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        lin = (q * rng.uniform(0.1, 3.0, 3)).astype(np.float32)
        m = mats[w]
        m[:3, :3] = lin.T
        m[3, :3] = rng.uniform(-2, 2, 3)
        m[3, 3] = 1.0
        k = KINDS[kind[w]]
        if k == "affine_negative_zeros": m[0, 3], m[2, 3] = F(-0.0), F(-0.0)
        elif k == "w2": m[3, 3] = 2.0
        elif k == "perspective": m[1, 3] = 0.25
        elif k == "one_lane_inf": points[w, int(rng.integers(0, 64)), int(rng.integers(0, 3))] = (INF, -INF)[w // 8 % 2]
        elif k == "one_lane_nan": points[w, int(rng.integers(0, 64)), int(rng.integers(0, 3))] = NAN
        elif k == "row0_overflows":                     # a finite point whose first output row overflows: w is 1 all the same
            m[0, 0] = 4.0
            points[w, int(rng.integers(0, 64)), 0] = F(3.0e38)
        elif k == "affine_infinite_entry":              # 0 * inf in row 0 of one lane
            m[1, 0] = INF
            points[w, int(rng.integers(0, 64)), 1] = 0.0
    skips = np.isin(kind, [KINDS.index("affine"), KINDS.index("affine_negative_zeros")])
    return dict(mats=mats.reshape(waves, 16), points=points.reshape(-1, 3), kind=kind, skips=skips)
