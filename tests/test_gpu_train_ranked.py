"""-m gpu: the one-launch train step that ranks the batch itself (srfrd_encoder_train_ranked) against the
two-launch step, which takes the ranking from srfrd_seq_order's workspace.  Every workgroup of the train kernel reads the id
plane, finds every sequence's first item and selects its own sequence from those; the slab a sequence lands in fixes the bits
of the deterministic step, so the two agree BIT FOR BIT - loss, parameters, both moments and every workgroup's dense-gradient
slab - exactly when the order is srfrd_seq_order's: first item ascending, then index ascending, a zero behind the first item
not counted as padding."""
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
SEED = 37
STEPS = 2


def _model(kind, dropout=0.5):
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, dropout, 2, 1, "cuda") if kind == "SASRec" else srfrd_amd.SRFRN(I, L, 45, 5, dropout, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _full(B, step, seed):
    """B sequences without a pad: (seq, rsq, pos, prs, neg, nrs), each (B, L), on the CPU"""
    return [x.clone() for x in srfrd_amd.synthetic_batch(I, L, B, seed=seed, index=step, device="cpu", min_len=L)[1:]]


def _mixed(B, step):
    """row i has (7 i + 3 step) mod 51 leading pads - with B >= 51 every count from 0 (no pad) to 50 (all pad), many times
    over and never sorted by index - and every third row two zero INPUTS behind its first item (no padding: the row keeps its
    rank); with B < 51 the step moves the counts"""
    t = _full(B, step, 71)
    for i in range(B):
        pads = (7 * i + 3 * step) % (L + 1)
        for x in t:
            x[i, :pads] = 0
        if i % 3 == 0 and pads + 4 < L:
            for x in t[:2]:
                x[i, pads + 1] = 0
                x[i, pads + 3] = 0
    if B >= L + 1:
        assert sorted({int((row != 0).to(torch.int64).argmax()) if bool((row != 0).any()) else L for row in t[0]}) == list(range(L + 1))
    return t


def _every_pad_count(step):
    """B = 51: sequence i has exactly i leading pads; the last one is all pad, and the odd rows carry an interior zero input"""
    t = _full(L + 1, step, 53)
    for i in range(L + 1):
        for x in t:
            x[i, :i] = 0
        if i % 2 == 1 and i + 2 < L:
            for x in t[:2]:
                x[i, i + 1] = 0
    return t


def _all_pad(B, step):
    """all-pad rows and rows without a pad, alternating (the step decides which come first): the two ends of the order, tied
    many times over"""
    t = _full(B, step, 73)
    for x in t:
        x[step % 2::2] = 0
    assert bool((t[2] != 0).any())
    return t


def _length(n):
    def fill(B, step):
        t = _full(B, step, 79 + n)
        for x in t:
            x[:, :L - n] = 0
        return t
    return fill


FILLS = {"mixed": _mixed, "all_pad": _all_pad, "len2": _length(2), "len50": _length(L)}


def _run(model, batches, one_launch):
    B = batches[0][0].shape[0]
    tr = srfrd_amd.FusedTrainer(model, B, L, seed=SEED, use_graph=False, deterministic=True)
    tr.train_launch = one_launch
    if one_launch:
        assert _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches())[0].startswith(
            "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here: nothing would be compared"
        assert tr.sched_mode == 1, "no length order asked for: nothing would be ranked"
    losses = [tr.step(None, *[x.cuda() for x in batch]).clone() for batch in batches]
    torch.cuda.synchronize()
    return (torch.stack(losses), model._flat.clone(), tr.m.clone(), tr.v.clone(), tr.slabs.clone()), tr


def _assert_bitwise(fused, split):
    for name, a, b in zip(("loss", "parameters", "m", "v", "slabs"), fused, split):
        assert torch.isfinite(a).all(), name
        if name == "slabs":      # slab for slab: the same sequences went to the same workgroups
            bad = [int(i) for i in (a != b).any(dim=1).nonzero().flatten()[:8]]
            assert not bad, f"slabs {bad} ... differ: another schedule"
        assert torch.equal(a, b), f"{name}: {(a != b).sum().item()} of {a.numel()} elements differ"


def _compare(kind, B, fill):
    batches = [FILLS[fill](B, step) for step in range(STEPS)]
    (fused, tr) = _run(_model(kind), batches, True)
    assert tr.sched is None or not bool(tr.sched.any()), "the one-launch step filled the schedule workspace: srfrd_seq_order ran"
    _assert_bitwise(fused, _run(_model(kind), batches, False)[0])


def _second_sequences_B():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count + 37


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("B", [3, 7])
@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_small_batches(kind, B, fill):
    _compare(kind, B, fill)


@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_second_sequences_per_workgroup(kind, fill):
    """B = 4 x CU count + 37: every workgroup walks a second sequence and some a third"""
    _compare(kind, _second_sequences_B(), fill)


def test_identity_order_above_1024():
    """B = 1025: more lengths than a workgroup holds - workgroup x takes sequence x in both forms"""
    _compare("SASRec", 1025, "mixed")


@pytest.mark.parametrize("B", [51, 512, 513, 600, 1024])
def test_chunk_edges(B):
    """the id plane is read in rounds of 512 ids and chunks of 512 sequences: one chunk exactly (the flagship's batch), one
    sequence more, a second chunk part full (and second sequences: the grid is 512), both chunks full; 51: every pad count once"""
    _compare("SASRec", B, "mixed")


def test_ranked_entry_point_refuses_a_negative_stride():
    lay = _lib.make_layout("SASRec", I, L, 50, 0, 0, 2, 1)
    import ctypes as C
    assert _lib.lib().srfrd_encoder_train_ranked(C.byref(lay), *([None] * 9), 8, L, 0.0, 0, None, 0, *([None] * 7), 1, None, None, None,
                                                 -1, None) == -1


def test_every_pad_count_against_the_oracle():
    """one fused dropout step of the every-pad-count batch against the CPU oracle: the bar of tests/test_gpu_train.py's dropout
    steps (tests/helpers.adam_tolerance inside assert_post_adam)"""
    cfg = O.Cfg("SASRec", I, L, 50, dropout=0.5)
    sd = random_sd(O.Cfg("SASRec", I, L, 50, dropout=0.0), 17)
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}).train()
    batch = _every_pad_count(0)
    loss_o, g_o = oracle_step_with_grads(cfg, sd, O.Adam(sd), tuple(batch), train=True, seed=O.step_seed(SEED, 1), b0=0)
    (loss, *_), _ = _run(model, [batch], True)
    assert abs(float(loss[0].cpu()) - float(loss_o)) < TOL
    assert_post_adam(model.state_dict(), sd, [g_o], cfg.D)
