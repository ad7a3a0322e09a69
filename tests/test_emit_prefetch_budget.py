"""Static budget of the emit kernel with the successor prefetch (tools/emit_isa_budget.py): a wave of the single-launch
kernel that is done with its rows asks for one plane of a later tile by ONE indexed buffer load, built on the scalar unit.
The four l = 20 instantiations of tests/test_emit_void_free_budget.py stay within the figures that file pins (copied here,
not imported), the single-launch ones hold exactly one prefetch instruction -- in the round loop, outside the row loop --
and the three-launch ones none.  Instruction-class counts and the compiler's resource usage only.  CPU only."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

# (geometry, single launch) at l = 20, no pre-sigmoid column, no seed words:
#   set-up VALU (all blocks), set-up VALU of a void-free wave, rounds VALU, row-loop VALU
SETUPS = {
    ("large", True): (200, 156, 403, 143),    # the kernel bench.py times
    ("small", True): (146, 122, 339, 143),
    ("large", False): (229, 184, 286, 143),
    ("small", False): (171, 146, 220, 143),
}
# (VGPRs, SGPR spills, occupancy, LDS bytes)
RESOURCES = {
    ("large", True): (59, 8, 6, 53728),
    ("small", True): (53, 8, 7, 33456),
    ("large", False): (56, 2, 6, 53712),
    ("small", False): (49, 0, 7, 33440),
}
# One static instruction: waves 1 ... 4 run it once each, one plane per wave (four wave-instructions per tile).
PREFETCH_LOADS = 1
IDS = lambda i: "%s-%s" % (i[0], "single" if i[1] else "three")  # noqa: E731


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as d:
        return isa.compile_asm(d)


@pytest.fixture(scope="module")
def budgets(compiled):
    return {inst: isa.budget(*compiled, isa.kernel_name(inst[0], inst[1], 20, False, False)) for inst in SETUPS}


@pytest.mark.parametrize("inst", sorted(SETUPS), ids=IDS)
def test_instruction_budget_is_held(budgets, inst):
    setup, short, rounds, row = SETUPS[inst]
    b = budgets[inst]
    void = b["setup_void"]
    assert void["uniform"], void
    assert b["setup"]["valu"] <= setup
    assert b["setup"]["valu"] - void["valu"] <= short
    assert b["rounds"]["valu"] <= rounds
    assert b["row_loop"]["valu"] <= row
    assert b["row_loop"]["f64"] == 43


@pytest.mark.parametrize("inst", sorted(RESOURCES), ids=IDS)
def test_resources_are_held(budgets, inst):
    vgprs, spills, occupancy, lds = RESOURCES[inst]
    b = budgets[inst]
    assert b["vgprs"] <= vgprs
    assert b["sgpr_spills"] <= spills
    assert b["occupancy"] == occupancy
    assert b["lds"] <= lds
    assert b["scratch"] == 0 and b["vgpr_spills"] == 0


@pytest.mark.parametrize("inst", sorted(SETUPS), ids=IDS)
def test_prefetch_loads_sit_in_the_round_loop_only(budgets, inst):
    loads = budgets[inst]["vmem_loads"]
    assert loads["rounds"]["prefetch"] == (PREFETCH_LOADS if inst[1] else 0), loads["rounds"]
    assert loads["row_loop"]["prefetch"] == 0 and loads["tail"]["prefetch"] == 0, loads
    # the row loop reads nothing from memory at all: a row is LDS reads, arithmetic and stores
    assert loads["row_loop"]["count"] == 0, loads["row_loop"]


def test_prefetch_is_in_every_single_launch_instantiation(compiled):
    """all PRE / SEEDS variants and the generic-length kernel carry the one instruction; no three-launch kernel does"""
    asm, remarks = compiled
    for geo in sorted(isa.GEOMETRY):
        for lfix, pre, seeds in ((20, False, False), (20, True, False), (20, False, True), (20, True, True), (0, False, False),
                                 (0, True, False)):
            for single in (True, False):
                b = isa.budget(asm, remarks, isa.kernel_name(geo, single, lfix, pre, seeds))
                n = sum(v["prefetch"] for v in b["vmem_loads"].values())
                assert n == (PREFETCH_LOADS if single else 0), (geo, lfix, pre, seeds, single, n)
                assert b["vmem_loads"]["rounds"]["prefetch"] == n
                # the load returns while the row loop runs: no instruction of the loop may write its destination register
                assert b["prefetch"]["dst_written_in_row_loop"] == [], (geo, lfix, pre, seeds, single)
                assert b["scratch"] == 0 and b["vgpr_spills"] == 0
