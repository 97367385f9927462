"""The owners of every HIP allocation and event (csrc/hip_owned.h) on the CPU: tests/host_emu/hip_owned_main.cpp compiles the
header against a counting stand-in for the HIP runtime (tests/host_emu/hip_counting/) and states what the owners promise - an
empty owner makes no call, a sufficient ensure makes none, a growing one frees before it allocates, a failure leaves an empty
owner, moves leave one owner per block, a struct of owners gives everything back whichever allocation fails."""
import os
import subprocess

import _harness as H


def test_sanitized_hip_owned(tmp_path):
    """Built with AddressSanitizer and UndefinedBehaviorSanitizer and run once: a double free, a use after free or a leak fails it."""
    root = H.ROOT
    csrc = os.path.join(root, "soft-rendering-toolsets_amd", "csrc")
    emu = os.path.join(root, "tests", "host_emu")
    exe = str(tmp_path / "hip_owned")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(emu, "hip_counting"), "-I" + csrc, "-I" + os.path.join(root, "include"),
                    os.path.join(emu, "hip_owned_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hip_owned: ok" in r.stdout
