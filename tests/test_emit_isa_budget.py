"""Static ISA budget of the emit kernel (tools/emit_isa_budget.py): the gfx950 code the compiler makes of the hot
instantiation must keep its occupancy, registers and LDS, and must not give back the VALU work removed from the row loop
and the per-wave set-up.  CPU only: hipcc cross-compiles for gfx950 without a GPU."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

# what the hot instantiation compiles to today (python tools/emit_isa_budget.py); lower is fine, higher is a regression
ROW_LOOP_VALU = 168
SETUP_VALU = 316
SGPR_SPILLS = 51


@pytest.fixture(scope="module")
def compiled():
    with tempfile.TemporaryDirectory() as d:
        return isa.compile_asm(d)


@pytest.fixture(scope="module")
def hot(compiled):
    return isa.budget(*compiled, isa.kernel_name())


def test_hot_kernel_occupancy_registers_lds(hot):
    assert hot["occupancy"] == 6
    assert hot["scratch"] == 0 and hot["vgpr_spills"] == 0
    assert hot["vgprs"] <= 80
    assert hot["lds"] <= 53760  # 42 allocation units of 1 280 B: three workgroups per CU


def test_hot_kernel_valu_budget(hot):
    assert hot["row_loop"]["f64"] == 43  # the scorer's f64 work is fixed by bit-exactness
    assert hot["row_loop"]["valu"] <= ROW_LOOP_VALU
    assert hot["setup"]["valu"] <= SETUP_VALU
    assert hot["sgpr_spills"] <= SGPR_SPILLS


@pytest.mark.parametrize("geo,chained,lfix,pre,seeds", [
    ("large", True, 20, True, False),    # PRE
    ("large", True, 20, False, True),    # SEEDS
    ("large", True, 0, False, False),    # any guide length
    ("small", True, 20, False, False),   # SMALL geometry
    ("large", False, 20, False, False),  # three-launch mode
])
def test_other_instantiations_have_no_scratch(compiled, geo, chained, lfix, pre, seeds):
    res = isa.resources(compiled[1], isa.kernel_name(geo, chained, lfix, pre, seeds))
    assert int(res["ScratchSize [bytes/lane]"]) == 0
    assert int(res["VGPRs Spill"]) == 0
