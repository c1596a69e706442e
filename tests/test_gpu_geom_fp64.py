"""-m gpu: the run-time-geometry encoder kernels at other widths and head splits, against the fp64 oracle (tests/geom_refs.py:
the sixteen cases and their seams; tests/test_geom_refs.py and tests/test_geom_cover.py: their CPU side).

``srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>``, ``encoder_bwd_kernel<0,0,0,0,-1,0,0>`` and their ``srfrd_long::`` builds run every
layout whose width is not 50 or that has more than one head.  The fp64 suites hold them at D = 50 (one and two heads) and
D = 40; here they run at D = 64, 63, 33, 32, 17, 16, 8 and 4, head widths 1, 4, 5, 8, 9, 10, 11, 16 and 32, and SRFR's last_conv
over 2 and 4 tiles - through the runners of tests/test_gpu_grad_fp64.py (``run_autograd``, ``run_fused`` in both scatter modes)
and tests/test_gpu_fwd_fp64.py (``run_eval``, ``run_last``, ``run_train``), not copies of them: every launch asserts its planned
kernel names first, and the metric, bounds and checks are those suites' own - row_errors <= bound(e32), rows whose fp64 gradient
is zero exactly zero, the K-bias rule, the second moment under twice the bound, the fused step's loss within max(16 e32, 1e-6),
row_errors_inf <= max(16 e32, 4e-6) on every forward output with NaN-poisoned pad rows counted, predict() on shared and
per-user candidates behind the last-position state.  No tolerance is defined here.

The bf16 item-table shadow runs test_gpu_bf16_families' four checks at two of the widths: w33 (a 66-byte shadow row) and w64b
(128 bytes, srfrd_long:: backward).

profiles/geom_fp64_errors.json holds the measured figures (tools/geom_fp64_report.py).
"""
import pytest

from tests import fwd_refs as R
from tests import geom_refs as W
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests import test_gpu_fwd_fp64 as TF
from tests import test_gpu_grad_fp64 as TG

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", W.CASES, ids=W.case_ids())
bf16_cases = pytest.mark.parametrize("c", W.BF16_CASES, ids=W.case_ids(W.BF16_CASES))


@cases
def test_autograd_gradients_meet_the_fp64_oracle(c, monkeypatch):
    G.assert_holds(TG.run_autograd(c, monkeypatch.setenv), f"case {c.id} autograd")


@TG.scatter
@cases
def test_fused_step_gradients_meet_the_fp64_oracle(c, det, monkeypatch):
    figs, figs2 = TG.run_fused(c, det, monkeypatch.setenv)
    G.assert_holds(figs, f"case {c.id} fused det={det}")
    G.assert_holds(figs2, f"case {c.id} fused det={det} second moment")


@cases
def test_eval_forward_meets_the_fp64_oracle(c, monkeypatch):
    R.assert_holds(TF.run_eval(c, monkeypatch.setenv), f"case {c.id} eval")


@cases
def test_last_position_state_and_candidate_logits_meet_the_fp64_oracle(c, monkeypatch):
    R.assert_holds(TF.run_last(c, monkeypatch.setenv), f"case {c.id} last")


@cases
def test_train_forward_with_dropout_meets_the_fp64_oracle(c, monkeypatch):
    figs, _, _ = TF.run_train(c, monkeypatch.setenv)
    R.assert_holds(figs, f"case {c.id} train")


# the bf16 shadow: test_gpu_bf16_families' own checks, on cases that file's CASES does not hold
@bf16_cases
def test_bf16_eval_forward_matches_the_bf16_oracle(c, monkeypatch):
    F.test_eval_forward_matches_the_bf16_oracle(c, monkeypatch)


@bf16_cases
def test_bf16_autograd_loss_and_gradients_match_the_bf16_oracle(c, monkeypatch):
    F.test_autograd_loss_and_gradients_match_the_bf16_oracle(c, monkeypatch)


@bf16_cases
def test_bf16_fused_steps_match_the_bf16_oracle_and_keep_the_shadow_current(c, monkeypatch):
    F.test_fused_steps_match_the_bf16_oracle_and_keep_the_shadow_current(c, monkeypatch)


@bf16_cases
def test_bf16_last_position_forward_and_ranking_match_the_bf16_oracle(c, monkeypatch):
    F.test_last_position_forward_and_ranking_match_the_bf16_oracle(c, monkeypatch)
