"""Host-only guards of the loss-head width and magnitude tests (tests/test_gpu_loss_widths.py, test_gpu_loss_extreme.py): the
width lists they are parametrised over reach every kernel instantiation the launchers can pick, and the extreme-logit inputs
hold the situations they are named after.  A later trimming of a list, or a change of a generator, that silently drops one
turns these red on a machine without a GPU."""
import pytest

from tests import loss_extreme_cases as X
from tests.loss_refs import ALIGN_OFFSETS, ALIGN_WIDTHS, FAKE_CASES, REQUIRED_WIDTHS, TNEG_SHAPES, WIDTHS, tneg_shape, xent_ks


def test_width_list_reaches_every_ks_instantiation():
    assert {xent_ks(d) for d in WIDTHS} == set(range(1, 17))
    assert set(REQUIRED_WIDTHS) <= set(WIDTHS) and all(1 <= d <= 64 for d in WIDTHS)
    # the backward's column tiles NC = ceil(KS / 4) follow from KS
    assert {(xent_ks(d) + 3) // 4 for d in WIDTHS} == {1, 2, 3, 4}


def test_widths_and_alignments_reach_every_gather_shape():
    aligned = {tneg_shape(d, 0) for d in WIDTHS}
    assert aligned == {(4, 1), (2, 1), (2, 2), (1, 1), (1, 2), (1, 3), (1, 4)} == TNEG_SHAPES
    shifted = {tneg_shape(d, 4 * off) for d in ALIGN_WIDTHS for off in ALIGN_OFFSETS}
    assert shifted == TNEG_SHAPES
    # at the widths of the alignment test every shape but (4, 1) is reachable through the address alone
    assert all(tneg_shape(d, 0) == (4, 1) for d in ALIGN_WIDTHS)


def test_fake_slice_cases():
    assert {d for d, _ in FAKE_CASES} == {3, 4, 26, 27, 45, 59, 63} and {f for _, f in FAKE_CASES} == {1, 5}
    assert all(d + f <= 64 for d, f in FAKE_CASES)
    assert len(FAKE_CASES) == 13                          # every pair but 63 + 5


@pytest.mark.parametrize("d_item, d_fake", X.EXTREME_WIDTHS)
def test_extreme_inputs_hold_their_situations(d_item, d_fake):
    X.check_xent_case(X.xent_case(d_item, d_fake, seed=d_item))
    X.check_sxent_case(X.sxent_case(d_item, d_fake, seed=d_item))
    for objective in ("softmax", "gbce"):                 # the very inputs tests/test_gpu_loss_extreme.py runs
        di, df, seed = X.tneg_case_args(d_item, d_fake, objective)
        X.check_tneg_case(X.tneg_case(di, df, seed=seed))
