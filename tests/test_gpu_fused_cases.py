"""GPU: every row of tests/fused_kernel_cases.py through the launch the trunks use (``PlanBuilder.conv_short`` / ``conv_se`` / ``conv_pair`` /
``x3d_edp`` / ``se_gate``) -- the launch runs the kernel instance the row names; every output, handed over full of NaN, comes back finite
and within the row's bound of the fp64 reference; the padded channels read back as exact zeros.  The table, the reference and the bounds'
derivation are in tests/fused_kernel_cases.py; tests/test_cpu_fused_kernel_cases.py proves without a GPU that the four tables together claim
every launch of the default plans and that the bounds fail a subtly wrong kernel.  With ``PASN_PARITY_LOG`` set every comparison appends its
largest err / bound ratio (profiles/fused_ladder_parity_observed.tsv)."""
import pytest

import fused_kernel_cases as fk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", fk.CASES, ids=[c.id for c in fk.CASES])
def test_fused_ladder_case(case):
    with fk.switches(case):
        built = fk.build(case, "cuda")
        assert (built.kind, built.name) == (fk.kind(case), case.expect), f"{case.id}: the launch runs {built.kind} {built.name}, the row says {fk.kind(case)} {case.expect}"
        outs = fk.launch(built)
    worst = fk.check(case, outs, built.name)
    print(f"{case.id}: {built.name} max err / bound = {worst:.3f}")
