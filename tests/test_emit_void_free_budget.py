"""Static budget of the emit kernel's set-up after the void terms of the hit masks moved under a wave-uniform branch
(tools/emit_isa_budget.py): a wave whose own words and two edge words hold no void bit skips deriving void, the two wave
shifts of it and the four void tests.  Plane 3 of the LDS copy holds `up | ac`, which takes one OR out of every row, and
the block scan's six DPP steps are six instructions.  Instruction-class counts and the compiler's resource usage only.
CPU only.

Every ceiling is what the instantiation compiles to with this change; lower is fine, higher is a regression.  The parent's
figures are beside them.  `short` is the set-up of a void-free wave: the whole set-up less the conditional region."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

# (geometry, single launch) at l = 20, no pre-sigmoid column, no seed words:
#   set-up VALU (all blocks), set-up VALU of a void-free wave, rounds VALU, row-loop VALU
SETUPS = {
    ("large", True): (200, 156, 403, 143),    # parent: 206, 206, 404, 144 -- the kernel bench.py times
    ("small", True): (146, 122, 339, 143),    # parent: 154, 154, 340, 144
    ("large", False): (229, 184, 286, 143),   # parent: 229, 229, 287, 144
    ("small", False): (171, 146, 220, 143),   # parent: 173, 173, 221, 144
}
# the parent's other figures, which stay: (VGPRs, SGPR spills, occupancy, LDS bytes)
RESOURCES = {
    ("large", True): (59, 8, 6, 53728),
    ("small", True): (53, 8, 7, 33456),
    ("large", False): (56, 2, 6, 53712),
    ("small", False): (49, 0, 7, 33440),
}
# row-loop VALU of other instantiations (geometry, single launch, LFIX, pre-sigmoid column, seed words): each one below the
# parent's (tests/test_emit_sgpr_budget.py, "reached") by the row's OR.  (The generic-length scorer's OR was fused with an AND: its
# row loops are the parent's, held there.)
ROW_LOOPS = {
    ("large", True, 20, True, True): 151,
    ("large", True, 20, True, False): 145,
    ("large", True, 20, False, True): 149,
    ("large", False, 20, True, True): 152,
}


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as d:
        return isa.compile_asm(d)


@pytest.mark.parametrize("inst", sorted(SETUPS), ids=lambda i: "%s-%s" % (i[0], "single" if i[1] else "three"))
def test_set_up_with_and_without_the_void_terms(compiled, inst):
    setup, short, rounds, row = SETUPS[inst]
    b = isa.budget(*compiled, isa.kernel_name(inst[0], inst[1], 20, False, False))
    void = b["setup_void"]
    # one region, entered past a scalar branch: no exec mask around the wave shifts
    assert void["uniform"], void
    assert void["valu"] >= 20, void  # (the region is there: void derived, shifted and tested in it, not ahead of the branch)
    assert b["setup"]["valu"] <= setup
    assert b["setup"]["valu"] - void["valu"] <= short
    assert b["rounds"]["valu"] <= rounds
    assert b["row_loop"]["valu"] <= row
    assert b["row_loop"]["f64"] == 43


@pytest.mark.parametrize("inst", sorted(RESOURCES), ids=lambda i: "%s-%s" % (i[0], "single" if i[1] else "three"))
def test_resources_are_the_parents(compiled, inst):
    vgprs, spills, occupancy, lds = RESOURCES[inst]
    b = isa.budget(*compiled, isa.kernel_name(inst[0], inst[1], 20, False, False))
    assert b["vgprs"] <= vgprs
    assert b["sgpr_spills"] <= spills
    assert b["occupancy"] == occupancy
    assert b["lds"] <= lds
    assert b["scratch"] == 0 and b["vgpr_spills"] == 0


@pytest.mark.parametrize("inst", sorted(ROW_LOOPS), ids=lambda i: "-".join(str(x) for x in i))
def test_row_loops_of_the_other_instantiations(compiled, inst):
    b = isa.budget(*compiled, isa.kernel_name(*inst))
    assert b["row_loop"]["valu"] <= ROW_LOOPS[inst]
    assert b["setup_void"]["uniform"], b["setup_void"]


def test_hot_set_up_scan_is_six_dpp_adds(compiled):
    """the block scan's wave scan: six v_add_u32_dpp in the set-up, and no scan step as a v_mov_b32_dpp with an add of
    its own (the only DPP moves are the wave shifts)"""
    asm, _ = compiled
    setup = []
    for label, header, _, ins in isa.blocks_of(asm, isa.kernel_name()):
        if header:
            break
        setup += ins
    assert sum(i.startswith("v_add_u32_dpp") for i in setup) == 6
    moves = [i for i in setup if i.startswith("v_mov_b32_dpp")]
    assert moves and all("wave_shl:1" in i or "wave_shr:1" in i for i in moves), moves
