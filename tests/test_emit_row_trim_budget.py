"""Row-loop ceiling of the hot emit kernel after the strand flag, the '+' orientation and the -1.0 of an unscored row
left the per-row path (tools/emit_isa_budget.py): one compare per row for the strand, the orientation and the default
as regions that whole waves skip, the three-address FMAs of crp_exp, three induction registers.  Instruction-class
counts and the compiler's resource usage only.  CPU only."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

ROW_LOOP_VALU = 144  # 153 before


@pytest.fixture(scope="module")
def hot():
    with tempfile.TemporaryDirectory() as d:
        return isa.budget(*isa.compile_asm(d), isa.kernel_name())


def test_hot_kernel_row_loop_after_the_trim(hot):
    assert hot["row_loop"]["f64"] == 43
    assert hot["row_loop"]["valu"] <= ROW_LOOP_VALU


def test_hot_kernel_resources_after_the_trim(hot):
    assert hot["sgpr_spills"] <= 51
    assert hot["vgprs"] <= 72
    assert hot["vgpr_spills"] == 0 and hot["scratch"] == 0
    assert hot["occupancy"] == 6
    assert hot["lds"] <= 53760
    assert hot["row_loop"]["readlane"] == 0 and hot["row_loop"]["writelane"] == 0
