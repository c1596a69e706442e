"""-m gpu: the forward -> backward hand-off inside the one-launch train step (encoder_train_ragged_kernel).
The train kernel's backward takes the last block's output, the head's hidden-state gradient and the ids from the LDS rows and
registers its forward left them in (rag_seam_handoff); the two-launch step (srfrd_encoder_fwd_sched + srfrd_encoder_bwd_sched)
reads all of it from global memory.  Under the deterministic scatter the two agree BIT FOR BIT, on batches built for the
hand-off's edges: every count of leading pads, head rows in front of the blocks' rows, a workgroup's second sequence."""
import pytest
import torch

import srfrd_amd
from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests.gpu_util import build_model, random_sd
from tests.helpers import assert_post_adam, oracle_step_with_grads

pytestmark = pytest.mark.gpu
I, L = 400, 50
TOL = 1e-4
SEED = 31


def _model(kind, dropout):
    torch.manual_seed(0)
    if kind == "SASRec":
        m = srfrd_amd.SASRec(I, L, 50, dropout, 2, 1, "cuda")
    elif kind == "SRFR":
        m = srfrd_amd.SRFR(I, L, 45, 5, dropout, 2, 1, "cuda")
    elif kind == "SRFRN":
        m = srfrd_amd.SRFRN(I, L, 45, 5, dropout, 2, 1, "cuda")
    else:
        m = srfrd_amd.SRFU_B(I, L, 50, 3, dropout, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _full(B, step, seed):
    """B sequences without a pad: (seq, rsq, pos, prs, neg, nrs), each (B, L), on the CPU"""
    t = [x.clone() for x in srfrd_amd.synthetic_batch(I, L, B, seed=seed, index=step, device="cpu", min_len=L)[1:]]
    assert bool((t[0] != 0).all() and (t[2] != 0).all() and (t[4] != 0).all())
    return t


def _every_pad_count(step):
    """B = L + 1: sequence i has exactly i leading pads (the last one is all pad)"""
    t = _full(L + 1, step, 53)
    for i in range(L + 1):
        for x in t:
            x[i, :i] = 0
    assert [int((row != 0).sum()) for row in t[0]] == list(range(L, -1, -1))
    return t


HEAD_ROWS = [(t0, k) for k in (1, 15, 16, 17) for t0 in (20, 21, 37)]      # (first input, targets start k in front of it)


def _head_in_front(step):
    """rows whose first non-zero TARGET lies k positions in front of their first non-zero INPUT - the head's range starts in
    front of the blocks' (for k >= 15 in an earlier 16-row tile: rows ph0 .. p0 - 1 of the last block's output are pad rows) -
    and, last, a row of ten inputs whose only target is at position 0"""
    t = _full(len(HEAD_ROWS) + 1, step, 59)
    seq, rsq, pos, prs, neg, nrs = t
    for i, (t0, k) in enumerate(HEAD_ROWS):
        seq[i, :t0] = 0
        rsq[i, :t0] = 0
        for x in (pos, prs, neg, nrs):
            x[i, :t0 - k] = 0
    i = len(HEAD_ROWS)
    seq[i, :L - 10] = 0
    rsq[i, :L - 10] = 0
    for x in (pos, prs, neg, nrs):
        x[i, 1:] = 0
    assert int(pos[i, 0]) != 0 and int((pos[i] != 0).sum()) == 1
    return t


def _second_sequences(B, grid, step):
    """a batch larger than the grid, all-pad and no-pad rows alternating at the front - and, in the opposite phase, from row
    `grid` on: a workgroup's second sequence is the other kind than its first"""
    t = [x.clone() for x in srfrd_amd.synthetic_batch(I, L, B, seed=61, index=step, device="cpu")[1:]]
    full = _full(128, step, 67)
    for j in range(64):
        for first, phase in ((0, 0), (grid, 1)):
            b = first + j
            if b >= B:
                continue
            for x, f in zip(t, full):
                if (j + phase) % 2 == 0:
                    x[b] = 0
                else:
                    x[b] = f[(64 if first else 0) + j]
    return t


def _run(model, batches, one_launch):
    B = batches[0][0].shape[0]
    tr = srfrd_amd.FusedTrainer(model, B, L, seed=SEED, use_graph=False, deterministic=True)
    tr.train_launch = one_launch
    if one_launch:
        assert _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches())[0].startswith(
            "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here: nothing would be compared"
    losses = [tr.step(None, *[x.cuda() for x in batch]).clone() for batch in batches]
    torch.cuda.synchronize()
    return (torch.stack(losses), model._flat.clone(), tr.m.clone(), tr.v.clone()), tr


def _assert_bitwise(fused, split):
    for name, a, b in zip(("loss", "parameters", "m", "v"), fused, split):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} of {a.numel()} elements differ"


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN", "SRFR", "SRFU_B"])
def test_every_pad_count(kind):
    """t0 = 0 .. 50: every first row tile (t0 - 1 + 12 crossing 16, 32, 48) and both neighbours of each boundary"""
    batches = [_every_pad_count(step) for step in range(2)]
    _assert_bitwise(_run(_model(kind, 0.5), batches, True)[0], _run(_model(kind, 0.5), batches, False)[0])


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_head_range_in_front_of_the_block_range(kind):
    batches = [_head_in_front(step) for step in range(2)]
    _assert_bitwise(_run(_model(kind, 0.5), batches, True)[0], _run(_model(kind, 0.5), batches, False)[0])


def test_outputs_still_written():
    """what the backward no longer reads is still there for everybody else: hidden states, logits, loss partial sums and the
    three checkpoint planes of the one-launch step are the two-launch step's, bit for bit"""
    batches = [_every_pad_count(0)]
    _, one = _run(_model("SASRec", 0.5), batches, True)
    _, two = _run(_model("SASRec", 0.5), batches, False)
    for name in ("hidden", "pl", "nl", "loss_part", "save_x", "save_h1", "save_aux"):
        a, b = getattr(one, name), getattr(two, name)
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} of {a.numel()} elements differ"


def test_second_sequence_does_not_see_the_first_hand_off():
    """B = 4 x CU count + 37: workgroups walk a second and a third sequence; the forward of each starts from zeros, not from the
    rows the previous sequence handed over (iter > 0)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * n_cu + 37
    m = _model("SASRec", 0.5)
    tr = srfrd_amd.FusedTrainer(m, B, L, seed=SEED, use_graph=False, deterministic=True)
    grid = _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches(), n_cu)[1]
    assert 0 < grid < B, "every workgroup would take one sequence: nothing would be tested"
    del tr
    batches = [_second_sequences(B, grid, step) for step in range(2)]
    _assert_bitwise(_run(m, batches, True)[0], _run(_model("SASRec", 0.5), batches, False)[0])


def test_every_pad_count_against_the_oracle():
    """one dropout step of the every-pad-count batch against the CPU oracle: the bar of tests/test_gpu_train.py's dropout steps"""
    cfg = O.Cfg("SASRec", I, L, 50, dropout=0.5)
    sd = random_sd(O.Cfg("SASRec", I, L, 50, dropout=0.0), 17)
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}).train()
    batch = _every_pad_count(0)
    loss_o, g_o = oracle_step_with_grads(cfg, sd, O.Adam(sd), tuple(batch), train=True, seed=O.step_seed(SEED, 1), b0=0)
    (loss, *_), _ = _run(model, [batch], True)
    assert abs(float(loss[0].cpu()) - float(loss_o)) < TOL
    assert_post_adam(model.state_dict(), sd, [g_o], cfg.D)
