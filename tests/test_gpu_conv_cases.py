"""GPU: every row of tests/conv_kernel_cases.py through ``pasn_conv3d_fwd`` -- the launch runs the kernel instance the row names, every
output element stays within the row's bound of the fp64 reference, and the padded channels read back as exact zeros.  The table, the
reference and the bound's derivation are in tests/conv_kernel_cases.py; tests/test_cpu_conv_kernel_cases.py proves without a GPU that
the table covers the default plans' instances and that the bound fails a subtly wrong kernel.  With ``PASN_PARITY_LOG`` set every
comparison appends its largest err / bound ratio (profiles/conv_ladder_parity_observed.tsv)."""
import pytest

import conv_kernel_cases as ck

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ck.CASES, ids=[c.id for c in ck.CASES])
def test_conv_ladder_case(case):
    with ck.switches(case):
        built = ck.build(case, "cuda")
        assert built.name == case.expect, f"{case.id}: the launch runs {built.name}, the row says {case.expect}"
        out = ck.launch(built)
    ck.check(case, out)
