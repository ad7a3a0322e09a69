"""Row-loop ceiling of the hot emit kernel after the PAM scorer's index and gate rework (tools/emit_isa_budget.py).
The scorer's table indices read the unshifted masks, or a shifted copy another chain computes anyway, and the gated
FMAs after the tables read the unshifted masks; this must not give the VALU work back.  CPU only."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import emit_isa_budget as isa  # noqa: E402

ROW_LOOP_VALU = 153  # 168 before the rework


def test_hot_kernel_row_loop_valu():
    with tempfile.TemporaryDirectory() as d:
        b = isa.budget(*isa.compile_asm(d), isa.kernel_name())
    assert b["row_loop"]["f64"] == 43
    assert b["row_loop"]["valu"] <= ROW_LOOP_VALU
