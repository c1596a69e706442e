"""-m gpu, fp32 item table: every encoder forward output against the fp64 oracle, relative to its own row's size
(tests/fwd_refs.py: reference, metric, bound, modes and seeds; tests/test_fwd_refs.py: their CPU side).

Three launches on every case of grad_refs.ALL_CASES - the gradient suite's list, which reaches every encoder kernel family at
two blocks and, through grad_refs.DEPTH, again at depths 1 and 3, with five cases at depth 8:

  eval   ``model.eval()``, ``model(...)`` under no_grad: hidden state, positive and negative logits - the evaluation
         instantiations (T = 0, no checkpoint), which no gradient test runs;
  last   ``model._launch_fwd_last``: the state every ranking call starts from, against ``H64[:, -1]``; then ``model.predict``
         with a candidate list shared by the batch and with a per-user (B, 37) matrix that holds id 0 and repeated ids
         (``srfrd_predict_logits``; on SRFRN with the predict-time label);
  train  ``model.train()`` with dropout 0.5 and the first step's seed: the instantiations autograd runs behind, masks on
         every site, against ``O.forward(..., train=True, seed=...)`` in fp64; the BCE loss of the device's logits too.

Before each launch the planned kernel name is asserted under the mode bits the launcher derives (fwd_refs.plan_bits).  The
model allocates every output, so a NaN sentinel cannot be planted in them directly: a buffer of each output's size is filled
with NaN and freed just before the launch (the caching allocator hands the freed block to the next request of that size), and
the metric counts every row - a padded position the kernel left unwritten shows as NaN or as a stale value, never as the last
LayerNorm's bias.

One more batch, fwd_refs.WAVE: more sequences than the evaluation forward has workgroups, through the eval and the last launch.

Per output: row_errors_inf <= bound(e32).  profiles/fwd_fp64_errors.json holds the measured figures (tools/fwd_fp64_report.py
calls run_eval / run_last / run_train / run_wave below).
"""
import pytest
import torch

from tests import fwd_refs as R
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", R.ALL_CASES, ids=G.case_ids())


def _model(cfg, sd, switch, setenv):
    from tests.gpu_util import build_model
    if switch:
        setenv(switch, "1")
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()})
    assert not model.bf16_table
    return model


def _assert_plan(model, B, L, mode, switch, want):
    """as test_gpu_bf16_families._assert_plan, under fwd_refs.plan_bits(mode) and the scratch the module path passes"""
    from srfrd_amd import _lib
    if switch:
        assert _lib.env_switches() == _lib.SWITCHES[switch]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    scratch = _lib.scratch_floats(model.layout, B, L)[0]
    got = _lib.encoder_plan(model.layout, B, L, R.plan_bits(mode), _lib.env_switches(), n_cu, scratch)[0][0]
    assert got == want, (mode, got, want)


def _poison(*shapes):
    """NaN into the blocks the next allocations of these sizes will be handed"""
    bufs = [torch.full(s, float("nan"), device="cuda", dtype=torch.float32) for s in shapes]
    del bufs


def _eval(model, ref):
    from tests.gpu_util import cuda
    B, L = ref.batch[0].shape
    model.eval()
    ids = cuda(*ref.batch)
    _poison((B, L, ref.cfg.d_out), (B, L), (B, L))
    with torch.no_grad():
        h, pl, nl = model(None, *ids)
    return {"hidden": h, "pos_logits": pl, "neg_logits": nl}


def _last(model, ref):
    from tests.gpu_util import cuda
    B = ref.batch[0].shape[0]
    model.eval()
    seq, rsq = cuda(*ref.batch[:2])
    shared, user = cuda(*ref.cands)
    with torch.no_grad():
        ids = model._prep(seq, rsq, None, None, None, None)
        _poison((B, 1, ref.cfg.d_out))
        state = model._launch_fwd_last(ids[0], ids[1])
    assert tuple(state.shape) == (B, 1, ref.cfg.d_out)
    out = {"last_state": state[:, 0]}
    _poison((B, 1, ref.cfg.d_out), (B, shared.numel()))
    out["cand_shared"] = model.predict(None, seq, rsq, shared)
    _poison((B, 1, ref.cfg.d_out), tuple(user.shape))
    out["cand_user"] = model.predict(None, seq, rsq, user)
    return out


def run_eval(c, setenv):
    """-> {output: fwd_refs.figures} of the evaluation forward"""
    ref = R.reference(c.id, "eval")
    R.assert_admissible(ref, f"case {c.id} eval")             # (e32 is this machine's: the bounds below come from it)
    model = _model(ref.cfg, ref.sd, c.switch, setenv)
    _assert_plan(model, c.B, c.L, "eval", c.switch, R.plan_name(c, "eval"))
    return R.compare(_eval(model, ref), ref)


def run_last(c, setenv):
    """-> {output: figures} of the last-position forward and of predict() behind it"""
    ref = R.reference(c.id, "last")
    R.assert_admissible(ref, f"case {c.id} last")
    model = _model(ref.cfg, ref.sd, c.switch, setenv)
    _assert_plan(model, c.B, c.L, "last", c.switch, R.plan_name(c, "last"))
    return R.compare(_last(model, ref), ref)


def run_train(c, setenv):
    """-> ({output: figures}, relative loss error, its bound) of the training-mode forward under the first step's seed"""
    from tests.gpu_util import cuda
    ref = R.reference(c.id, "train")
    R.assert_admissible(ref, f"case {c.id} train")
    assert ref.cfg.dropout == 0.5 and ref.train
    model = _model(ref.cfg, ref.sd, c.switch, setenv).train()
    model._next_seed = lambda: ref.seed
    _assert_plan(model, c.B, c.L, "train", c.switch, R.plan_name(c, "train"))
    seq, rsq, pos, prs, neg, nrs = cuda(*ref.batch)
    _poison((c.B, c.L, ref.cfg.d_out), (c.B, c.L), (c.B, c.L))
    h, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    assert h.requires_grad                                   # (the autograd path: checkpoints written, the mode bits asserted)
    figs = R.compare({"hidden": h, "pos_logits": pl, "neg_logits": nl}, ref)
    loss = F._bce(pl.detach(), nl.detach(), pos)
    err = R.assert_loss_holds(loss, ref, f"case {c.id} train")
    return figs, err, R.loss_bound(R.loss_reference(ref)[1])


def run_wave(mode, setenv=None):
    """-> {output: figures} of fwd_refs.WAVE through the eval or the last launch"""
    w = R.WAVE
    ref = R.wave_reference(mode)
    assert ref.clamp
    model = _model(ref.cfg, ref.sd, None, setenv)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert w["B"] > 2 * 2 * n_cu                              # some workgroup takes a third sequence
    _assert_plan(model, w["B"], w["L"], mode, None, w["name"])
    return R.compare((_eval if mode == "eval" else _last)(model, ref), ref)


@cases
def test_eval_forward_meets_the_fp64_oracle(c, monkeypatch):
    R.assert_holds(run_eval(c, monkeypatch.setenv), f"case {c.id} eval")


@cases
def test_last_position_state_and_candidate_logits_meet_the_fp64_oracle(c, monkeypatch):
    R.assert_holds(run_last(c, monkeypatch.setenv), f"case {c.id} last")


@cases
def test_train_forward_with_dropout_meets_the_fp64_oracle(c, monkeypatch):
    figs, _, _ = run_train(c, monkeypatch.setenv)
    R.assert_holds(figs, f"case {c.id} train")


@pytest.mark.parametrize("mode", ["eval", "last"])
def test_more_sequences_than_workgroups_meet_the_fp64_oracle(mode):
    R.assert_holds(run_wave(mode), f"wave {mode}")
