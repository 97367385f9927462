"""CPU, two stand-alone programs built from tests/host_emu and run once each.

box_minmax_main.cpp: the top-down step's box tests from per-axis min / max (box_hit_minmax, topdown_step<true>, csrc/pt_trace.h)
against box_hit_inv / topdown_step<false> on inputs that pass the guard - 2^18 random sets and constructed ones (flat boxes, origins
on a face, an edge or a corner, reciprocals that make l == h or overflow the products, `times` that are NaN, inverted or infinite,
sets scaled by 2^+-40): hit flags, the flag nibble and the child order equal, `times`, cur_far_t.x and the children's `times` equal
as values and bit-equal wherever the value is not a zero; zeros of the other sign are counted and printed.  The guard's predicates
must refuse a zero, infinite or NaN reciprocal, a non-finite origin, a non-finite or inverted box.

sweep_flag_slot_main.cpp: the flag nibble through the slot word that is dead between the sweeps (csrc/pt_wave.h), all sixteen nibbles
at every node of trees with 2 to 16 leaves against the 64-bit word, in the kernel's order of reads and writes."""
import _harness as H


def _build_and_run(tmp_path, name, ok_line):
    out = H.run_sanitized_main(tmp_path, name + "_main.cpp", scene_layer=False, expect=ok_line, flags=("-O2",),      # (as the product build: no sanitizer)
                               extra=("-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"))
    print(out)
    return out


def test_box_minmax_equals_box_hit_inv_inside_the_guard(tmp_path):
    out = _build_and_run(tmp_path, "box_minmax", "box_minmax: ok")
    counts = out.split("sets: ")[1].split()
    assert int(counts[0]) == 1 << 18 and int(counts[2]) > 100000      # random, constructed
    nibbles = [int(v) for v in out.split("flag nibbles:")[1].split()[:16]]
    assert all(nibbles[f] > 100 for f in (0, 2, 5, 11, 15)), nibbles     # none, right, left, both (right first), both (left first)
    assert sum(nibbles) == sum(nibbles[f] for f in (0, 2, 5, 11, 15))


def test_flag_nibbles_through_the_dead_slot_word(tmp_path):
    _build_and_run(tmp_path, "sweep_flag_slot", "sweep_flag_slot: ok")
