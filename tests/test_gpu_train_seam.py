"""-m gpu: the head seam of the one-launch train step.  The train kernel's forward computes the fused-BCE logit gradients, the
head's hidden-state gradient and the target rows' item-table contributions; its backward starts from them
(encoder_train_ragged_kernel).  The two-launch step (srfrd_encoder_fwd_sched + srfrd_encoder_bwd_sched)
still does all of it in the backward: under the deterministic scatter the two agree BIT FOR BIT over three steps on batches
built to hit the head's edges; the float-atomic scatter and the CPU oracle are held to tests/helpers.adam_tolerance."""
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
HOT = 7                   # the item id that row 5 repeats among its inputs, positives and negatives (rows 0 and 3 use it too)


def _cfg(kind, dropout):
    if kind == "SASRec":
        return O.Cfg(kind, I, L, 50, dropout=dropout)
    return O.Cfg(kind, I, L, 45, d_fake=5, dropout=dropout)


def _edge_rows(step):
    """seven sequences (seq, rsq, pos, prs, neg, nrs), each (7, L), on the CPU:
    0 no pad; 1 length 2; 2 the only non-zero target is the last position; 3 pos == 0 at interior positions (dp = dn = 0 inside
    the head range); 4 interior zero input ids; 5 one item id several times among inputs, positives and negatives; 6 all pad"""
    t = [x.clone() for x in srfrd_amd.synthetic_batch(I, L, 7, seed=41, index=step, device="cpu", min_len=30)[1:]]
    seq, rsq, pos, prs, neg, nrs = t

    def keep_last(row, n):
        for x in t:
            x[row, :L - n] = 0

    full = [x.clone() for x in srfrd_amd.synthetic_batch(I, L, 1, seed=43, index=step, device="cpu", min_len=L)[1:]]
    for x, f in zip(t, full):
        x[0] = f[0]
    assert bool((seq[0] != 0).all())
    keep_last(1, 2)
    keep_last(2, 20)
    pos[2, :L - 1] = 0
    prs[2, :L - 1] = 0
    keep_last(3, 30)
    pos[3, 33] = pos[3, 40] = pos[3, 41] = 0
    prs[3, 33] = prs[3, 40] = prs[3, 41] = 0
    keep_last(4, 25)
    seq[4, 35] = seq[4, 36] = seq[4, 44] = 0
    rsq[4, 35] = rsq[4, 36] = rsq[4, 44] = 0
    keep_last(5, 12)
    seq[5, -6:] = torch.tensor([HOT, 9, HOT, HOT, 11, HOT])
    pos[5, -6:] = torch.tensor([9, HOT, HOT, 11, HOT, 13])
    neg[5, -8:-4] = HOT
    neg[5, -1] = HOT
    pos[0, 10] = pos[3, 45] = HOT         # ... and in two other sequences: contributions of several workgroups on one row
    neg[0, 20] = HOT
    keep_last(6, 0)
    assert not bool(seq[6].any() or pos[6].any() or neg[6].any())
    return t


def _batch(B, step):
    """B = 7: the edge rows; B = 3: the length-2, interior-zero-target and all-pad rows; larger: the edge rows in front of a
    synthetic batch"""
    rows = _edge_rows(step)
    if B == 7:
        out = rows
    elif B == 3:
        out = [x[[1, 3, 6]] for x in rows]
    else:
        out = [x.clone() for x in srfrd_amd.synthetic_batch(I, L, B, seed=47, index=step, device="cpu")[1:]]
        for x, r in zip(out, rows):
            x[:7] = r
    return [x.cuda() for x in out]


_SD = {}


def _sd(kind, dropout):
    if kind not in _SD:
        _SD[kind] = random_sd(_cfg(kind, 0.0), 17)
    return {k: v.clone() for k, v in _SD[kind].items()}


def _run(kind, dropout, B, one_launch, steps=3, deterministic=True, bf16=False):
    model = build_model(_cfg(kind, dropout), _sd(kind, dropout)).train()
    if bf16:
        model.use_bf16_table()
    tr = srfrd_amd.FusedTrainer(model, B, L, seed=29, use_graph=False, deterministic=deterministic)
    tr.train_launch = one_launch
    if one_launch:
        assert _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches())[0].startswith(
            "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here: nothing would be compared"
    losses = [tr.step(None, *_batch(B, step)).clone() for step in range(steps)]
    torch.cuda.synchronize()
    return torch.stack(losses), model._flat.clone(), tr.m.clone(), tr.v.clone(), model


def _assert_bitwise(fused, split):
    for name, a, b in zip(("loss", "parameters", "m", "v"), fused[:4], split[:4]):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} of {a.numel()} elements differ"


@pytest.mark.parametrize("B", [7, 3])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_seam_step_is_bitwise_the_two_launch_step(kind, dropout, B):
    _assert_bitwise(_run(kind, dropout, B, True), _run(kind, dropout, B, False))


def test_seam_step_is_bitwise_the_two_launch_step_over_the_bf16_shadow():
    _assert_bitwise(_run("SASRec", 0.5, 7, True, bf16=True), _run("SASRec", 0.5, 7, False, bf16=True))


def test_seam_step_with_second_sequences_per_workgroup():
    """a batch larger than the grid: a workgroup's second sequence goes through the same hand-off buffer rows as nobody's first"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * n_cu * 2 + 37
    _assert_bitwise(_run("SASRec", 0.5, B, True), _run("SASRec", 0.5, B, False))


def _oracle_step(kind, dropout, B):
    cfg = _cfg(kind, dropout)
    sd = _sd(kind, dropout)
    batch = tuple(x.cpu() for x in _batch(B, 0))
    loss_o, g_o = oracle_step_with_grads(cfg, sd, O.Adam(sd), batch, train=dropout > 0.0, seed=O.step_seed(29, 1), b0=0)
    return cfg, sd, float(loss_o), g_o


@pytest.mark.parametrize("B", [7, 3])
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_float_atomic_scatter_from_the_forward_head(kind, dropout, B):
    """deterministic=False: the target rows' contributions leave the forward's head as float atomics.  One step against the
    deterministic scatter of the same kernel: the same loss bits (a forward output), every parameter within
    tests/helpers.adam_tolerance of it (the oracle's gradients tell a real gradient from rounding noise)"""
    det = _run(kind, dropout, B, True, steps=1)
    atom = _run(kind, dropout, B, True, steps=1, deterministic=False)
    assert torch.equal(det[0], atom[0])
    cfg, _, _, g_o = _oracle_step(kind, dropout, B)
    want = {k: v.detach().cpu() for k, v in det[4].state_dict().items()}
    assert_post_adam(atom[4].state_dict(), want, [g_o], cfg.D)


def test_seam_step_against_the_oracle():
    """one dropout step of the edge batch against the CPU oracle: the bar of tests/test_gpu_train.py's dropout steps"""
    cfg, sd, loss_o, g_o = _oracle_step("SASRec", 0.5, 7)
    loss, _, _, _, model = _run("SASRec", 0.5, 7, True, steps=1, deterministic=False)
    assert abs(float(loss[0].cpu()) - loss_o) < TOL
    assert_post_adam(model.state_dict(), sd, [g_o], cfg.D)
