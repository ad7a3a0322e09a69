"""Set-up ceiling of the hot emit kernel after the edge words of a wave moved to scalar loads (tools/emit_isa_budget.py):
the word on either side of a wave's words is loaded, range-tested and derived into its G / C / void masks on the SALU, and a
tile's halo words come from the same values; this must not give the VALU work back, nor cost the row loop or the SGPR
budget anything.  CPU only."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

SETUP_VALU = 284  # 316 before the edge words became wave-uniform values
SGPR_SPILLS = 51


def test_hot_kernel_setup_valu():
    with tempfile.TemporaryDirectory() as d:
        b = isa.budget(*isa.compile_asm(d), isa.kernel_name())
    assert b["setup"]["valu"] <= SETUP_VALU
    assert b["row_loop"]["f64"] == 43
    assert b["sgpr_spills"] <= SGPR_SPILLS
