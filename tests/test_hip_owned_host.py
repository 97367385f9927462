"""The owners of every HIP allocation and event (csrc/hip_owned.h) on the CPU: tests/host_emu/hip_owned_main.cpp compiles the
header against a counting stand-in for the HIP runtime (tests/host_emu/hip_counting/) and states what the owners promise - an
empty owner makes no call, a sufficient ensure makes none, a growing one frees before it allocates, a failure leaves an empty
owner, moves leave one owner per block, a struct of owners gives everything back whichever allocation fails."""
import os

import _harness as H


def test_sanitized_hip_owned(tmp_path):
    """Built with AddressSanitizer and UndefinedBehaviorSanitizer and run once: a double free, a use after free or a leak fails it."""
    H.run_sanitized_main(tmp_path, "hip_owned_main.cpp", scene_layer=False, device_headers=False,
                         extra=("-Wall", "-I" + os.path.join(H.HOST_EMU, "hip_counting"), "-I" + H.CSRC))
