"""SGPR spill traffic of the emit kernel after the single-launch instantiation stopped carrying kernel arguments and
wave-uniform flags through its set-up (tools/emit_isa_budget.py): the compiler spills SGPRs into VGPR lanes, so every
spill and reload is a VALU instruction (v_writelane_b32 / v_readlane_b32) that computes nothing.  Instruction-class
counts and the compiler's resource usage only.  CPU only.

The instantiations with the pre-sigmoid column are held to the parent's row loop too: with the spills gone the register
allocator needed one more copy per row for that column, and the single-launch kernel now stores an unscored row's
pre-sigmoid value from its score's registers instead of keeping a second -1.0."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

# the hot instantiation: (what the change had to reach, what it compiles to today); lower is fine, higher is a regression
SGPR_SPILLS = (26, 8)    # 49 before
SETUP_VALU = (239, 206)  # 276 before; the three-launch instantiation of the same template: 229
ROUNDS_VALU = (415, 404)  # 427 before
# unchanged: the chunk bookkeeping on the scalar unit was measured slower and is not in the tree (profiles/EXPERIMENTS.md)
ROW_LOOP_VALU = (144, 144)
VGPRS = (65, 59)
LANE_OPS = 8  # v_writelane in the set-up, v_readlane in the round loop: 49 + 9 and 52 before

# other instantiations: (SGPR spills, VGPRs, row-loop VALU, occupancy) of the parent commit -- none may be above -- and what
# each compiles to today, which holds the gain of the single-launch ones (the three-launch ones are the parent's)
OTHERS = {
    ("small", True, 20, False, False): ((45, 59, 144, 7), (8, 53, 144, 7)),
    ("large", True, 0, False, False): ((43, 72, 238, 6), (2, 66, 238, 6)),
    ("large", True, 20, True, True): ((46, 66, 152, 6), (2, 60, 152, 6)),
    ("large", False, 20, False, False): ((2, 56, 144, 6), (2, 56, 144, 6)),
    ("small", False, 20, False, False): ((0, 49, 144, 7), (0, 49, 144, 7)),
    # the other variants with the pre-sigmoid column or seed words
    ("large", True, 20, True, False): ((33, 65, 146, 6), (2, 60, 146, 6)),
    ("large", True, 20, False, True): ((41, 66, 150, 6), (2, 60, 150, 6)),
    ("large", True, 0, True, False): ((41, 72, 245, 6), (2, 66, 244, 6)),
    ("small", True, 20, True, True): ((40, 60, 152, 7), (2, 54, 151, 7)),
    ("large", False, 20, True, True): ((12, 57, 153, 6), (12, 57, 153, 6)),
    ("small", False, 0, True, False): ((8, 58, 245, 7), (8, 58, 245, 7)),
}


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as d:
        return isa.compile_asm(d)


@pytest.fixture(scope="module")
def hot(compiled):
    return isa.budget(*compiled, isa.kernel_name())


@pytest.mark.parametrize("k", [0, 1], ids=["required", "reached"])
def test_hot_kernel_spill_traffic(hot, k):
    assert hot["sgpr_spills"] <= SGPR_SPILLS[k]
    assert hot["setup"]["valu"] <= SETUP_VALU[k]
    assert hot["rounds"]["valu"] <= ROUNDS_VALU[k]
    assert hot["row_loop"]["valu"] <= ROW_LOOP_VALU[k]
    assert hot["vgprs"] <= VGPRS[k]


def test_hot_kernel_lane_instructions(hot):
    assert hot["setup"]["writelane"] <= LANE_OPS and hot["setup"]["readlane"] == 0
    assert hot["rounds"]["readlane"] <= LANE_OPS and hot["rounds"]["writelane"] == 0
    assert hot["row_loop"]["readlane"] == 0 and hot["row_loop"]["writelane"] == 0


def test_hot_kernel_keeps_its_resources(hot):
    assert hot["row_loop"]["f64"] == 43
    assert hot["occupancy"] == 6
    assert hot["scratch"] == 0 and hot["vgpr_spills"] == 0
    assert hot["lds"] <= 53760


def test_single_launch_set_up_is_not_above_the_three_launch_one(compiled, hot):
    three = isa.budget(*compiled, isa.kernel_name("large", False, 20, False, False))
    assert hot["setup"]["valu"] <= three["setup"]["valu"]


@pytest.mark.parametrize("k", [0, 1], ids=["parent", "reached"])
@pytest.mark.parametrize("inst", sorted(OTHERS), ids=lambda i: "-".join(str(x) for x in i))
def test_other_instantiations_are_not_above_the_parent_nor_what_they_reached(compiled, inst, k):
    spills, vgprs, row_valu, occupancy = OTHERS[inst][k]
    b = isa.budget(*compiled, isa.kernel_name(*inst))
    assert b["sgpr_spills"] <= spills
    assert b["vgprs"] <= vgprs
    assert b["row_loop"]["valu"] <= row_valu
    assert b["occupancy"] == occupancy
    assert b["scratch"] == 0 and b["vgpr_spills"] == 0
    assert b["row_loop"]["readlane"] == 0 and b["row_loop"]["writelane"] == 0
