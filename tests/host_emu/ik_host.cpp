// TEST-ONLY host emulation of soft-rendering-toolsets_amd/csrc/pt_ik.h, built by tests/_ik_cases.py with g++ -ffp-contract=off: the
// functions the IK kernel runs, compiled for the host, with the intermediate values of the first iteration handed out - the four
// points compute_gradient takes from every joint's matrix and every handle joint's `current` - next to the pose after one whole
// call (50 iterations).  test_pt_ik_host.py compares them with what it derives from the reference's recorded joint_to_posed and
// with the recorded poses.
#include <cstdint>
#include <vector>

#include "pt_ik.h"

extern "C" {

// One Skeleton::do_ik on pose (in place).  frame[12 j ..] = {origin, x, y, z} and current[3 j ..] of the FIRST iteration (zero for a
// joint no enabled handle reaches / that is no enabled handle's joint); active[j] = ik_joint_flags.
void ik_emu_call(const int32_t* parent, const float* extent, uint32_t njoints, const uint32_t* handle_joint, const float* targets, const uint8_t* enabled,
                 uint32_t nhandles, float* pose, float* frame, float* current, uint32_t* active) {
  std::vector<float> cap(4 * (size_t)njoints, 0.0f), scratch((size_t)srt::kIkJointFloats * njoints, 0.0f);
  for (uint32_t j = 0; j < njoints; j++)
    for (int a = 0; a < 3; a++) cap[4 * (size_t)j + a] = extent[3 * (size_t)j + a];
  std::vector<uint32_t> off, list;
  srt::ik_build_csr(parent, njoints, handle_joint, nhandles, off, list);
  float* local = scratch.data();
  for (uint32_t j = 0; j < njoints; j++) {
    active[j] = srt::ik_joint_flags(off.data(), list.data(), handle_joint, enabled, j);
    if (active[j]) srt::ik_phase_local(pose, j, local);
  }
  for (uint32_t j = 0; j < njoints; j++)
    if (active[j]) srt::ik_phase_chain(parent, cap.data(), local, njoints, j, (active[j] & 2u) != 0, frame, current);
  srt::ik_step_host(parent, cap.data(), njoints, handle_joint, off.data(), list.data(), targets, enabled, scratch.data(), pose);
}

// The CSR of ik_build_csr: off[njoints + 1]; list[cap] takes min(cap, off[njoints]) entries.  Returns off[njoints].
uint32_t ik_emu_csr(const int32_t* parent, uint32_t njoints, const uint32_t* handle_joint, uint32_t nhandles, uint32_t* off_out, uint32_t* list_out, uint32_t cap) {
  std::vector<uint32_t> off, list;
  srt::ik_build_csr(parent, njoints, handle_joint, nhandles, off, list);
  for (uint32_t j = 0; j <= njoints; j++) off_out[j] = off[j];
  for (uint32_t k = 0; k < list.size() && k < cap; k++) list_out[k] = list[k];
  return off[njoints];
}

}  // extern "C"
