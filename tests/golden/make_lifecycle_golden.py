#!/usr/bin/env python3
"""Write tests/golden/lifecycle_epochs.npz: the oracle's epoch image of every scene of tests/test_pt_lifecycle_gpu.py at that
test's size (32x24, depth 3, 2 samples, seed 11).  Needs no GPU:

    python tests/golden/make_lifecycle_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _harness as H  # noqa: E402
import test_pt_lifecycle_gpu as T  # noqa: E402
from _cases import pt_scene  # noqa: E402

if __name__ == "__main__":
    H.build_oracle()
    out = {key: H.OraclePT(pt_scene(name), T.W, T.HT, T.DEPTH, use_bvh).epoch(T.SEED, 0, T.SPP) for (name, use_bvh), key in zip(T.SCENES, T.IDS)}
    np.savez_compressed(T.GOLDEN, **out)
    print("wrote", T.GOLDEN, {k: v.shape for k, v in out.items()})
