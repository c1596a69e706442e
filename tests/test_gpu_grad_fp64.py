"""-m gpu, fp32 item table: every encoder gradient against the fp64 oracle, relative to its own row's size (tests/grad_refs.py:
reference, metric, bound, cases and seeds; tests/test_grad_refs.py: their CPU side).

Two ways to a gradient, both on every case of grad_refs.ALL_CASES - test_gpu_bf16_families.CASES, which reach every encoder
kernel family, plus the <50,32,8,0> pair, the default geometry's tile-boundary and duplicate-heavy batches, and grad_refs.DEPTH:
every family again at depths 1 and 3 and five cases at depth 8 (ids "-b<n>"; every other case has two blocks):

  autograd  a training-mode forward (dropout 0) and ``loss.backward()`` through ``model(...)``: ``p.grad``;
  fused     ONE ``FusedTrainer.step`` from fresh moments with dropout 0.5, both scatter modes: the optimizer state then holds
            exp_avg = (1 - beta1) g and exp_avg_sq = (1 - beta2) g^2 - the fused BCE head, the head gradient computed in the
            train kernel's forward, the hand-off and the 1 / count scale, none of which runs under autograd and none of whose
            SCALE the stepped weights can show (Adam's first step moves an element by lr g / (|g| + eps)).

Before each launch the planned kernel names are asserted as the bf16 file does (the names carry no table flag).  At the default
geometry the plan must offer the one-launch train kernel; the tile-boundary batch also runs as two launches.  One fused case
runs with l2_emb = 1e-3: that term is not divided by the target count, so it pins the relative scale of the two parts.

The step's loss is held to the fp64 loss of the same reference (tests/fwd_refs.py: relative error <= max(16 e32, 1e-6)).

Per tensor: row_errors <= bound(e32), rows whose fp64 gradient is exactly zero exactly zero, the K slice of in_proj_bias under
its own rule; exp_avg_sq / (1 - beta2) against g64^2 under twice the bound.  profiles/grad_fp64_errors.json holds the measured
figures (tools/grad_fp64_report.py calls run_autograd / run_fused below).
"""
import pytest
import torch

from tests import fwd_refs as R
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", G.ALL_CASES, ids=G.case_ids())
scatter = pytest.mark.parametrize("det", [True, False], ids=["deterministic", "atomics"])


def _model(c, ref, setenv):
    from tests.gpu_util import build_model
    if c.switch:
        setenv(c.switch, "1")
    model = build_model(ref.cfg, {k: v.clone() for k, v in ref.sd.items()}).train()
    assert not model.bf16_table
    return model


def run_autograd(c, setenv):
    """-> {tensor: grad_refs.tensor_figures} of p.grad after a training-mode forward and backward"""
    from tests.gpu_util import cuda
    ref = G.reference(c.id, "autograd")
    G.assert_admissible(ref, f"case {c.id} autograd")          # (e32 is this machine's: the bounds below come from it)
    model = _model(c, ref, setenv)
    F._assert_plan(c, model, "autograd", c.autograd)
    seq, rsq, pos, prs, neg, nrs = cuda(*ref.batch)
    _, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    F._bce(pl, nl, pos).backward()
    return G.compare({k: p.grad for k, p in model.named_parameters()}, ref)


def run_fused(c, det, setenv, train_launch=True, l2=0.0):
    """-> (figures of exp_avg / (1 - beta1), figures of exp_avg_sq / (1 - beta2) against g64^2) after one step"""
    import srfrd_amd
    from srfrd_amd import _lib
    from tests.gpu_util import cuda
    ref = G.reference(c.id, "fused", l2)
    G.assert_admissible(ref, f"case {c.id} fused")
    model = _model(c, ref, setenv)
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=det, l2_emb=l2)
    tr.train_launch = train_launch
    F._assert_plan(c, model, "fused", c.fused, scratch=tr.n_scratch)
    if c.id in G.TRAIN_KERNEL_IDS:
        assert _lib.encoder_plan_train(tr.lay, c.B, c.L, tr._train_mode, _lib.env_switches())[0].startswith(
            "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here"
    loss = tr.step(None, *cuda(*ref.batch))
    assert bool(torch.isfinite(loss).all())
    # the step's loss (the fused BCE head's partial sums, the 1 / count scale, the l2_emb term) against the fp64 loss of the
    # same reference: tests/fwd_refs.py, |loss - loss64| / loss64 <= max(16 e32, 1e-6)
    R.assert_loss_holds(loss.detach().cpu(), R.fused_step_reference(c.id), f"case {c.id} fused det={det} l2={l2}", l2)
    g, g2 = G.fused_gradients(tr, model)
    return G.compare(g, ref), G.compare(g2, ref, squares=True)


@cases
def test_autograd_gradients_meet_the_fp64_oracle(c, monkeypatch):
    G.assert_holds(run_autograd(c, monkeypatch.setenv), f"case {c.id} autograd")


@scatter
@cases
def test_fused_step_gradients_meet_the_fp64_oracle(c, det, monkeypatch):
    figs, figs2 = run_fused(c, det, monkeypatch.setenv)
    G.assert_holds(figs, f"case {c.id} fused det={det}")
    G.assert_holds(figs2, f"case {c.id} fused det={det} second moment")


@scatter
@pytest.mark.parametrize("cid", G.TRAIN_KERNEL_IDS)
def test_two_launch_step_gradients_meet_the_fp64_oracle(cid, det, monkeypatch):
    """the tile-boundary batch through srfrd_encoder_fwd_sched + srfrd_encoder_bwd_sched (the test above runs it through the
    one-launch train kernel)"""
    figs, figs2 = run_fused(G.BY_ID[cid], det, monkeypatch.setenv, train_launch=False)
    G.assert_holds(figs, f"case {cid} two launches det={det}")
    G.assert_holds(figs2, f"case {cid} two launches det={det} second moment")


@scatter
def test_fused_step_with_l2_emb_meets_the_fp64_oracle(det, monkeypatch):
    figs, figs2 = run_fused(G.BY_ID[G.L2_ID], det, monkeypatch.setenv, l2=G.L2_EMB)
    G.assert_holds(figs, f"case {G.L2_ID} l2_emb det={det}")
    G.assert_holds(figs2, f"case {G.L2_ID} l2_emb det={det} second moment")
