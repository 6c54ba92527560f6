"""CPU test of the preconditions of tests/test_gpu_sizes.py: at the sizes and frames of tests/size_cases.py the free-running
oracle has as many near-tie pixels as the table says.  Where that number is 0 the GPU test compares every row with the
free-running oracle and demands identical decisions; without this test nobody could tell from a GPU run whether a row left out
of a comparison was left out legitimately."""
import pytest
import torch

import size_cases as SC


@pytest.mark.parametrize("case", SC.SIZE_CASES, ids=SC.case_id)
def test_oracle_near_ties_are_as_the_case_table_states(case):
    """(32, 64) and (64, 128): the hard mask (fg > 0.5) is off at every pixel with the synthetic weights -- asserted here so that
    nobody reads those two cases as covering the gated branch of the alignments; the other cases have it on somewhere."""
    fg = SC.oracle_fg(case.crop, case.B, case.seed)
    fh, fw = case.crop[0] // 8, case.crop[1] // 8
    assert fg.shape == (case.B, 36, fh, fw)
    near = SC.near_tie_mask(fg)
    n, clean = int(near.sum()), SC.clean_fraction(near)
    hard = (fg.max(dim=1)[0] > 0.5).float().mean().item()
    print("%s: near-tie pixels %d of %d, clean rows %.3f, hard mask on at %.3f" % (SC.case_id(case), n, near.numel(), clean, hard))
    if case.near_ties is not None:
        assert n == case.near_ties
    else:
        assert clean >= SC.CLEAN_MIN
    if case.crop in ((32, 64), (64, 128)):
        assert hard == 0.0
    else:
        assert 0.0 < hard < 1.0
    if case.crop == (160, 416):
        assert 0.4 < hard < 0.7            # both branches of the gate, in bulk


def test_case_table_covers_the_thresholds_it_was_chosen_for():
    """Pure arithmetic on the table: the properties of the feature maps that steer the plan builder."""
    hw = {c.crop: (c.crop[0] // 8) * (c.crop[1] // 8) for c in SC.SIZE_CASES}
    assert hw[(96, 224)] % 32 != 0 and hw[(160, 416)] % 32 != 0                       # igemm logits / softmax / igemm P.V
    assert hw[(96, 256)] % 128 == 0 and 12 % 16 != 0                                  # fused attend, generic pooling
    assert hw[(64, 128)] == 128 and hw[(32, 64)] == 32
    assert 36 * hw[(32, 64)] == 1152                                                  # fewer anchors than nms_topN_pre (3000)
    assert hw[(256, 256)] % 128 == 0 and 32 % 16 == 0                                 # fused attend, nested pooling
    c = SC.by_crop((160, 192))
    assert hw[c.crop] % 32 == 0 and hw[c.crop] % 128 != 0 and c.B * hw[c.crop] // 32 * 3 >= 900   # wave-kernel ANAB GEMMs
    assert all(c.crop[0] % 32 == 0 and c.crop[1] % 32 == 0 for c in SC.SIZE_CASES)
    for c in SC.SIZE_CASES:                                                           # level 5 odd in at least one direction
        if c.crop in ((96, 224), (96, 256), (160, 416), (160, 192)):
            assert (c.crop[0] // 32) % 2 == 1
