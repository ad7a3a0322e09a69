"""The loads at the head of a tile's serial chain leave together (tools/emit_isa_budget.py): in every single-launch
instantiation of the emit kernel the descriptor loads of the look-back's first look -- one per lane, two in the
instantiation with both extra columns -- are issued with no `s_waitcnt vmcnt` between them, and a thread's scorer-table
loads -- ceil(units / 512) of 16 bytes each: two with the chain tables of l = 20, one for the generic length -- are all
issued before the first wait.  The instantiation bench.py times holds the parent commit's instruction counts and
resources (its figures from the tool on that commit, as constants).  Instruction-class counts and the compiler's
resource usage only.  CPU only."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

BLOCK = 512                            # threads per tile
TAB_UNITS = {20: 676, 0: 128}          # 16-byte units staged: exp table and chain tables (l = 20), the 2 KiB exp table alone
# (lfix, pre-sigmoid column, seed words): every variant the library instantiates
VARIANTS = ((20, False, False), (20, True, False), (20, False, True), (20, True, True), (0, False, False), (0, True, False))
# descriptors per lane and look (crp_kernels.hip): one, but two in the instantiation with both extra columns
LB_DEPTH, LB_DEPTH_BOTH_COLUMNS = 1, 2
SINGLE = [(geo,) + v for geo in sorted(isa.GEOMETRY) for v in VARIANTS]
IDS = lambda i: "-".join(str(x) for x in i)  # noqa: E731

# the parent commit's figures of the LARGE single-launch l = 20 kernel
PARENT_HOT = {"setup": 193, "rounds": 397, "row_loop": 143, "vgprs": 58, "sgpr_spills": 2, "lds": 53760, "occupancy": 6}


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as d:
        return isa.compile_asm(d)


def test_trip_counts():
    assert -(-TAB_UNITS[20] // BLOCK) == 2 and -(-TAB_UNITS[0] // BLOCK) == 1


@pytest.mark.parametrize("inst", SINGLE, ids=IDS)
def test_head_loads_are_in_flight_together(compiled, inst):
    geo, lfix, pre, seeds = inst
    b = isa.budget(*compiled, isa.kernel_name(geo, True, lfix, pre, seeds))
    assert b["lookback"]["first_window_waits_between_loads"] == 0, b["vmem_loads"]["rounds"]
    assert b["lookback"]["first_window_loads"] == (LB_DEPTH_BOTH_COLUMNS if pre and seeds else LB_DEPTH)
    assert b["staging"]["loads_before_first_wait"] == -(-TAB_UNITS[lfix] // BLOCK)
    assert b["scratch"] == 0 and b["vgpr_spills"] == 0


def test_three_launch_kernels_have_no_look_back_and_share_the_staging(compiled):
    for geo in sorted(isa.GEOMETRY):
        for lfix, pre, seeds in VARIANTS:
            b = isa.budget(*compiled, isa.kernel_name(geo, False, lfix, pre, seeds))
            assert b["lookback"] == {"first_window_loads": 0, "first_window_waits_between_loads": None}, (geo, lfix, pre, seeds)
            assert b["staging"]["loads_before_first_wait"] == -(-TAB_UNITS[lfix] // BLOCK), (geo, lfix, pre, seeds)


def test_hot_kernel_holds_the_parents_budget(compiled):
    b = isa.budget(*compiled, isa.kernel_name())
    assert b["setup"]["valu"] <= PARENT_HOT["setup"]
    assert b["rounds"]["valu"] <= PARENT_HOT["rounds"]
    assert b["row_loop"]["valu"] <= PARENT_HOT["row_loop"]
    assert b["row_loop"]["f64"] == 43
    assert b["vgprs"] <= PARENT_HOT["vgprs"]
    assert b["sgpr_spills"] <= PARENT_HOT["sgpr_spills"]
    assert b["lds"] <= PARENT_HOT["lds"]
    assert b["occupancy"] == PARENT_HOT["occupancy"]
    assert b["scratch"] == 0 and b["vgpr_spills"] == 0
