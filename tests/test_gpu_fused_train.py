"""-m gpu: the one-launch train step (srfrd_encoder_train_sched) against the two-launch step (srfrd_encoder_fwd_sched +
srfrd_encoder_bwd_sched) it replaces: same model, ids and seed, deterministic item-table scatter - the loss, every parameter
and both Adam moments agree BIT FOR BIT after every one of three steps, for every kind variant of the ragged kernels, with
and without dropout, at the flagship batch, a partial one, a tiny one, and batches of all-full and all-short sequences."""
import pytest
import torch

import srfrd_amd
from srfrd_amd import _lib

pytestmark = pytest.mark.gpu
I, L = 1000, 50
KINDS = ["SASRec", "SRFR", "SRFRN", "SRFU_B"]          # kind variants 0, 1, 2, 3 of the ragged kernels
BATCHES = {"B512": (512, None), "B300": (300, None), "B7": (7, None), "full50": (256, 50), "len2": (256, 2)}


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


def _batch(B, length, step):
    ids = list(srfrd_amd.synthetic_batch(I, L, B, seed=5, index=step, device="cuda", min_len=length or 2))[1:]
    if length is not None:                   # every sequence exactly `length` long (left padded)
        for t in ids:
            t[:, :L - length] = 0
    return ids


def _run(kind, dropout, B, length, one_launch):
    m = _model(kind, dropout)
    tr = srfrd_amd.FusedTrainer(m, B, L, use_graph=False, deterministic=True)
    tr.train_launch = one_launch
    losses = []
    for step in range(3):
        losses.append(tr.step(None, *_batch(B, length, step)).clone())
    torch.cuda.synchronize()
    return torch.stack(losses), m._flat.clone(), tr.m.clone(), tr.v.clone(), tr


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("kind", KINDS)
def test_one_launch_step_is_bitwise_the_two_launch_step(kind, dropout, batch):
    B, length = BATCHES[batch]
    fused = _run(kind, dropout, B, length, True)
    tr = fused[-1]
    assert _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches())[0].startswith(
        "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here: nothing would be compared"
    split = _run(kind, dropout, B, length, False)
    for name, a, b in zip(("loss", "parameters", "m", "v"), fused[:4], split[:4]):
        assert torch.isfinite(a).all(), name
        diff = (a != b).sum().item()
        assert diff == 0, f"{name}: {diff} of {a.numel()} elements differ"


def test_one_launch_step_with_second_sequences_per_workgroup():
    """a batch larger than the grid: workgroups take a second sequence (read-modify-write slabs, identity order)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * n_cu * 2 + 37
    fused = _run("SASRec", 0.5, B, None, True)
    split = _run("SASRec", 0.5, B, None, False)
    for name, a, b in zip(("loss", "parameters", "m", "v"), fused[:4], split[:4]):
        diff = (a != b).sum().item()
        assert diff == 0, f"{name}: {diff} of {a.numel()} elements differ"
