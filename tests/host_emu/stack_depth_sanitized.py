"""Sanitizer run of the traversal stacks at full depth, on the CPU, as a stand-alone program (nothing is loaded into Python):

    python tests/host_emu/stack_depth_sanitized.py

writes the deep_max, deep_tlas and deep_both scenes of tests/_cases.py with the rays the GPU tests trace (the camera's, and rays
aimed down the chain) to a temporary file, builds tests/host_emu/stack_depth_main.cpp + flat_host.cpp + the scene layer with
-fsanitize=address,undefined (tests/_harness.py:run_sanitized_main), and runs the program on the file.  Exit status 0 and a last
line "ok": clean."""
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _cases import camera_rays, chain_rays, pt_scene  # noqa: E402
from _harness import run_sanitized_main  # noqa: E402

WANT = {"deep_max": (7, 48), "deep_tlas": (22, 16), "deep_both": (24, 48)}


def write_scenes(path):
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(WANT)))
        for name, want in WANT.items():
            scene = pt_scene(name)
            f.write(struct.pack("<I", len(scene["objects"])))
            for o in scene["objects"]:
                if o["kind"] == "sphere":
                    f.write(struct.pack("<I", 1) + f32(o["T"]) + struct.pack("<f", o["radius"]))
                else:
                    idx = np.ascontiguousarray(o["idx"], np.uint32)
                    f.write(struct.pack("<I", 0) + f32(o["T"]) + struct.pack("<I", len(o["pos"])) + f32(o["pos"]) + f32(o["nrm"])
                            + struct.pack("<I", len(idx)) + idx.tobytes())
            rays = [camera_rays(scene["camera"], 32, 24), chain_rays(7, 3000, scene)]
            org, d, b = (np.concatenate([r[k] for r in rays]) for k in range(3))
            f.write(struct.pack("<I", len(org)) + f32(org) + f32(d) + f32(b) + struct.pack("<II", *want))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "scenes.bin")
        write_scenes(data)
        print(run_sanitized_main(tmp, "stack_depth_main.cpp", extra_srcs=["flat_host.cpp"], args=[data], expect="ok"), end="")
        return 0


if __name__ == "__main__":
    sys.exit(main())
