"""GPU: every row of tests/stem_kernel_cases.py through ``pasn_first_conv_fwd`` / ``pasn_first_conv_gray_fwd`` / ``pasn_first_conv_mfma_fwd``
/ ``pasn_x3d_stem_fwd`` / ``pasn_x3d_stem_gray_fwd`` / ``pasn_x3d_stem_mfma_fwd`` -- the launch runs the kernel instance the row names; every
output element, handed over as NaN, comes back within the row's bound of the fp64 reference, and the padded channels read back as exact
zeros.  The pair rows run the two unfused launches a three-channel uint8 clip takes off the matrix-core arm end to end against the stem's
reference.  One row per family runs twice and gives the same bits.  The table, the reference and the bound's derivation are in
tests/stem_kernel_cases.py; tests/test_cpu_stem_kernel_cases.py proves without a GPU that the table covers every name a plan can print and
that the bound fails a subtly wrong kernel.  With ``PASN_PARITY_LOG`` set every comparison appends its largest err / bound ratio
(profiles/stem_ladder_parity_observed.tsv)."""
import pytest
import torch

import stem_kernel_cases as sk

pytestmark = pytest.mark.gpu

TWICE = ("fc_u8_bf16_48_grey", "fcm_bf16_2_11", "st_f32_bf16", "sm_u8_1")


@pytest.mark.parametrize("case", sk.CASES, ids=[c.id for c in sk.CASES])
def test_stem_ladder_case(case):
    with sk.switches(case):
        built = sk.build(case, "cuda")
        assert built.name == case.expect, f"{case.id}: the launch runs {built.name}, the row says {case.expect}"
        out = sk.launch(built)
    sk.check(case, out)


@pytest.mark.parametrize("case", [sk.BY_ID[i] for i in TWICE], ids=TWICE)
def test_stem_ladder_case_repeats_bit_for_bit(case):
    with sk.switches(case):
        first, second = sk.launch(sk.build(case, "cuda")), sk.launch(sk.build(case, "cuda"))
    assert {sk.family(sk.BY_ID[i]) for i in TWICE} == {"first_conv_kernel", "first_conv_mfma_kernel", "x3d_stem_kernel", "x3d_stem_mfma_kernel"}
    assert torch.equal(first, second), f"{case.id}: the repeated launch differs"
