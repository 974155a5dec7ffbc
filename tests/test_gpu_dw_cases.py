"""GPU: every row of tests/dw_kernel_cases.py through ``pasn_dwconv3d_fwd`` / ``pasn_dwconv3d_se_fwd`` / ``pasn_x3d_expdw_fwd`` -- the launch
runs the kernel instance the row names; every output element stays within the row's bound of the fp64 reference and the padded channels
read back as exact zeros; the pool partial rows, handed over full of NaN, come back finite and sum to the fp64 pool sums within their
bound; a fused gate stays within its bound, and the launch repeated with nothing cleared leaves its arrival counters at zero and gives the
same bits.  The table, the reference and the bounds' derivation are in tests/dw_kernel_cases.py; tests/test_cpu_dw_kernel_cases.py proves
without a GPU that the table covers the default plans' instances and that the bounds fail a subtly wrong kernel.  With ``PASN_PARITY_LOG``
set every comparison appends its largest err / bound ratio (profiles/dw_ladder_parity_observed.tsv)."""
import pytest
import torch

import dw_kernel_cases as dk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", dk.CASES, ids=[c.id for c in dk.CASES])
def test_dw_ladder_case(case):
    with dk.switches(case):
        built = dk.build(case, "cuda")
        assert built.name == case.expect, f"{case.id}: the launch runs {built.name}, the row says {case.expect}"
        if not case.se:
            dk.check(case, dk.launch(built))
            return
        first, second, counters = dk.launch(built, twice=True)
    dk.check(case, first)
    # the last-arriving-block protocol's contract (PlanBuilder.dwconv_se): the counters read zero after every launch, a repeat is bit-identical
    for i, c in enumerate(counters):
        assert c is not None and int(c.abs().max()) == 0, f"{case.id}: arrival counters after launch {i + 1}: {c.tolist()}"
    assert torch.equal(first.gate, second.gate) and torch.equal(first.out, second.out) and torch.equal(first.pool, second.pool), f"{case.id}: the repeated launch differs"
