"""-m gpu: the bf16 item-table shadow (``layout.table_bf16``) on every encoder kernel family, against the bf16 oracle.

Each forward source builds its own ``ItemTable{a.table, a.table16}`` gather and each backward source carries its own copy of
the two-instantiation target gather (2-byte loads, the ``item ? shadow : side`` select of SRFRN's fake channel, per-kernel chunk
and tail arithmetic); the ``srfrd_long::`` builds compile the same sources a second time.  The backward sources share the
order of their per-position arrays, ``bce_dlogits`` and the zero fill (``srfrd_enc_bwd_head.h``), not the gather: written as one
function it changed every kernel's instruction schedule.  tests/test_gpu_bf16_table.py meets
the ragged pair and the <50,32,8> first-generation pair; the cases below meet the rest: every shape and switch already runs in
fp32 (test_gpu_long.py, test_gpu_train.py, test_gpu_heads.py, test_encoder_plan.py) - the only new input is table_bf16 = 1.

Before it launches anything a test asks the plan (with the launcher's own mode bits, the environment's switches, the device's
CU count and the scratch the caller really passes) and asserts the kernel names of its case, the read-modify-write flag
dropped: a later plan change cannot move a case onto another family unnoticed.  tests/test_bf16_family_cover.py (CPU) holds
the case list to every family key the plan can produce.

Parity is like for like (the oracle rounds the table the same way), so the bar is the project's 1e-4; the rounding itself is
visible: with I = 300, ``random_sd(cfg, 7)`` and the batch seeds below the bf16 and the fp32 oracle differ by 2.44e-3 .. 4.69e-3
in the positive logits (smallest: case h), and every user's top 11 scores are at least 3.16e-4 apart (smallest: cases a / q),
both measured on the CPU oracle alone.
"""
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
I = 300
# A pre-activation is a 50-term fp32 dot product of O(1) terms: two correct implementations differ by at most ~50 * 6e-8 = 3e-6
# on it (observed on the hidden states: 1.4e-6).  Batches are chosen so that no ReLU input is closer to zero than three times that.
RELU_MARGIN = 1e-5

Case = namedtuple("Case", "id kind d_item d_fake heads L B switch seed fused_seed eval_fwd last_fwd autograd fused blocks",
                  defaults=(2,))          # blocks: the depth (tests/grad_refs.py, DEPTH, holds the others)

_F = "srfrd::encoder_fwd_kernel"
_B = "srfrd::encoder_bwd_kernel"
_GEN = "<0,0,0,0,-1,0,0>"
_ROWS = "srfrd::encoder_fwd_rows_kernel"
_SLOTS = "srfrd::encoder_bwd_slots_kernel"
_CHUNKS = "srfrd::encoder_bwd_chunks_kernel"
_FL = "srfrd_long::encoder_fwd_kernel"
_BL = "srfrd_long::encoder_bwd_kernel"


def _same(fwd, bwd):
    """a case whose four launch modes run one forward and one backward instantiation"""
    return dict(eval_fwd=fwd, last_fwd=fwd, autograd=(fwd, bwd), fused=(fwd, bwd))


def _rows(targs, bwd):
    """the row-owner forward: its plain instantiation <..., 0> for the last-position call, <..., 1> for every other"""
    f1 = f"{_ROWS}<{targs},1>"
    return dict(eval_fwd=f1, last_fwd=f"{_ROWS}<{targs},0>", autograd=(f1, bwd), fused=(f1, bwd))


def _first(f_targs, b_auto, b_fused, f_fused=None):
    """a first-generation forward <.., T, ..> whose training instantiation (T = 1) only the fused step reaches"""
    f0 = _F + "<" + f_targs.format(T=0) + ">"
    return dict(eval_fwd=f0, last_fwd=f0, autograd=(f0, b_auto), fused=(_F + "<" + (f_fused or f_targs).format(T=1) + ">", b_fused))


# Kernel names as srfrd_encoder_plan prints them on the built library, the trailing read-modify-write flag of the slot-placed and
# row-chunked backward dropped.  B = 6 below seq_len 100, 5 from there on; `seed`: the batch the eval / autograd / ranking
# checks run on, `fused_seed` and `fused_seed + 1`: the batches of the two fused steps - the first seeds from 6 / 50 on at which,
# on the CPU oracle, the top-11 gaps exceed 3 * TOL, the two oracles' positive logits differ by 20 * TOL and relu_margin
# exceeds 2 * RELU_MARGIN.
CASES = [
    Case("a", "SASRec", 50, 0, 1, 50, 6, "SRFRD_NO_RAGGED", 8, 50,
         **_first("50,64,8,50,0,{T},50", f"{_SLOTS}<50,50,0,50>", f"{_SLOTS}<50,50,0,50>")),
    Case("b", "SRFRN", 45, 5, 1, 50, 6, "SRFRD_NO_SLOTS50", 6, 54,
         **_first("50,64,8,50,2,{T},45", f"{_B}<50,64,8,50,2,0,45>", f"{_B}<50,64,8,50,2,1,45>")),
    Case("c", "SRFR", 45, 5, 1, 50, 6, "SRFRD_GENERIC", 7, 50, **_same(_F + _GEN, _B + _GEN)),       # d_out < D: last_conv
    Case("d", "SASRec", 50, 0, 2, 50, 6, None, 7, 50, **_same(_F + _GEN, _B + _GEN)),                # two heads
    Case("e", "SASRec", 40, 0, 1, 37, 6, None, 6, 50, **_same(_F + _GEN, _B + _GEN)),                # odd LP, row stride 80 B
    Case("f", "SRFU_B", 50, 0, 1, 64, 6, None, 8, 50, **_same(_F + "<50,64,8,0,-1,0,0>", _B + "<50,64,8,0,-1,0,0>")),
    Case("g", "SASRec", 50, 0, 1, 100, 5, None, 9, 50,                                               # C4's kernels
         **_first("50,112,8,100,0,{T},50", f"{_SLOTS}<50,100,0,50>", f"{_SLOTS}<50,100,0,50>", "50,112,16,100,0,{T},50")),
    Case("h", "SRFRN", 45, 5, 1, 100, 5, None, 8, 50, **_same(_F + _GEN, f"{_SLOTS}<50,100,2,45>")),
    Case("i", "SASRec", 50, 0, 1, 100, 5, "SRFRD_NO_SLOTS", 9, 50,
         **_first("50,112,8,100,0,{T},50", _BL + _GEN, f"{_BL}<50,112,8,100,0,1,50>", "50,112,16,100,0,{T},50")),
    Case("j", "SASRec", 50, 0, 1, 200, 5, None, 11, 56, **_rows("50,0,50", f"{_CHUNKS}<50,0,50>")),   # C5_bf16_table's kernels
    # 203, not 207: from seq_len 205 on the row-chunked backward's LDS no longer fits and the plan answers srfrd_long::
    # (13 row tiles and five chunks, 4 x 48 + 11 rows, as at 207)
    Case("k", "SRFRN", 45, 5, 1, 203, 5, None, 11, 70, **_rows("50,2,45", f"{_CHUNKS}<50,2,45>")),
    Case("l", "SRFU_B", 50, 0, 1, 113, 5, None, 7, 50, **_rows("50,-1,50", f"{_CHUNKS}<50,-1,50>")),
    Case("m", "SRFR", 45, 5, 1, 128, 5, None, 8, 56, **_rows("50,1,45", f"{_CHUNKS}<50,1,45>")),     # 32-row tail
    Case("n", "SASRec", 50, 0, 1, 200, 5, "SRFRD_NO_ROWS", 11, 56, **_same(_FL + _GEN, f"{_CHUNKS}<50,0,50>")),
    Case("o", "SASRec", 50, 0, 2, 200, 5, None, 13, 70, **_same(_FL + _GEN, _BL + _GEN)),
    Case("p", "SRFRN", 45, 5, 1, 50, 6, "SRFRD_ROWS_ALWAYS", 6, 54, **_rows("50,2,45", f"{_SLOTS}<50,50,2,45>")),
    # the <50,64,8,50> first-generation backward with d_fake = 0 (case b holds its SRFRN variant)
    Case("q", "SASRec", 50, 0, 1, 50, 6, "SRFRD_NO_SLOTS50", 8, 50,
         **_first("50,64,8,50,0,{T},50", f"{_B}<50,64,8,50,0,0,50>", f"{_B}<50,64,8,50,0,1,50>")),
]


def _plan_bits():
    from srfrd_amd import _lib as P
    tgt = P.PLAN_POS | P.PLAN_NEG
    # launch mode -> (srfrd_encoder_fwd's mode bits, srfrd_encoder_bwd's) as the two launchers derive them from their arguments
    # ("head": the catalog-loss step, FusedTrainer._enqueue_ce_compute - no targets, the backward driven by d_hidden)
    return {"eval": (tgt, None), "last": (0, None), "autograd": (tgt | P.PLAN_CKPT, tgt),
            "fused": (tgt | P.PLAN_CKPT | P.PLAN_LOSS | P.PLAN_DROPOUT, tgt | P.PLAN_FUSED_BCE | P.PLAN_DROPOUT),
            "head": (P.PLAN_CKPT | P.PLAN_DROPOUT, P.PLAN_DROPOUT)}


def strip_rmw(name):
    """the read-modify-write flag (a function of the batch size and the CU count only) off a backward's name"""
    return re.sub(r",(?:true|false)>$", ">", name)


def planned(layout, B, L, launch, switches, n_cu, scratch_fwd, scratch_bwd):
    """(forward, backward | None) names the plan gives the launches of one mode"""
    from srfrd_amd import _lib
    fbits, bbits = _plan_bits()[launch]
    fwd = _lib.encoder_plan(layout, B, L, fbits, switches, n_cu, scratch_fwd)[0][0]
    bwd = None if bbits is None else strip_rmw(_lib.encoder_plan(layout, B, L, bbits, switches, n_cu, scratch_bwd)[1][0])
    return fwd, bwd


def case_scratch(layout, B, L, launch):
    """floats of scratch the callers pass: the module path sizes it per direction, FusedTrainer once for both"""
    from srfrd_amd import _lib
    nf, nb = _lib.scratch_floats(layout, B, L)
    return (max(nf, nb),) * 2 if launch in ("fused", "head") else (nf, nb)


def cfg_of(c, bf16=True, dropout=0.0):
    return O.Cfg(c.kind, I, c.L, c.d_item, d_fake=c.d_fake, n_labels=3 if c.kind.startswith("SRFU") else 0, num_heads=c.heads,
                 num_blocks=c.blocks, dropout=dropout, table_bf16=bf16)


def relu_margin(cfg, sd, batch, train=False, seed=0):
    """On the oracle alone: the smallest |pre-activation| of a feed-forward ReLU over the tokens that carry gradient (padded
    positions are masked behind the block).  A unit whose pre-activation is within fp32 rounding of zero has derivative 1 in
    one implementation and 0 in another while every forward value agrees: the gradient of that token is then not defined to
    1e-4 (tests/helpers.py, assert_post_adam).  Case k's first batch seed had such a unit: 1.5e-8 at sequence 2, position 156,
    unit 21 of block 0; flipping it alone in the oracle moves conv1.weight's gradient by 1.90e-4, which is what the
    row-chunked backward showed against the oracle, every other tensor within 5e-7."""
    taps = {}
    O.forward(cfg, sd, *batch, train=train, seed=seed, b0=0, taps=taps)
    live = batch[0] != 0
    out = float("inf")
    for i in range(cfg.num_blocks):
        w, b = sd[f"forward_layers.{i}.conv1.weight"], sd[f"forward_layers.{i}.conv1.bias"]
        out = min(out, float((taps[f"h2{i}"] @ w.squeeze(-1).T + b)[live].abs().min()))
    return out


def _setup(c, monkeypatch, dropout=0.0):
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    if c.switch:
        monkeypatch.setenv(c.switch, "1")
    cfg = cfg_of(c, dropout=dropout)
    sd = random_sd(cfg, 7)
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}).use_bf16_table()
    assert model.bf16_table and model._lay16.table_bf16 == 1
    batch = srfrd_amd.synthetic_batch(I, c.L, c.B, seed=c.seed, device="cpu")[1:]
    return cfg, sd, model, batch


def _assert_plan(c, model, launch, want, scratch=None):
    from srfrd_amd import _lib
    if c.switch:
        assert _lib.env_switches() == _lib.SWITCHES[c.switch]
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    sf, sb = case_scratch(model.layout, c.B, c.L, launch) if scratch is None else (scratch, scratch)
    got = planned(model.layout, c.B, c.L, launch, _lib.env_switches(), n_cu, sf, sb)
    assert got == want, (c.id, launch, got, want)


def _bce(pl, nl, pos):
    idx = torch.where(pos != 0)
    crit = torch.nn.BCEWithLogitsLoss()
    return crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])


_ids = [f"{c.id}-{c.kind}-L{c.L}" + (f"-{c.switch}" if c.switch else "") + (f"-h{c.heads}" if c.heads > 1 else "") for c in CASES]
cases = pytest.mark.parametrize("c", CASES, ids=_ids)


@cases
def test_eval_forward_matches_the_bf16_oracle(c, monkeypatch):
    from tests.gpu_util import cuda, maxerr
    cfg, sd, model, batch = _setup(c, monkeypatch)
    _assert_plan(c, model, "eval", (c.eval_fwd, None))
    model.eval()
    with torch.no_grad():
        h, pl, nl = model(None, *cuda(*batch))
    ho, plo, nlo = O.forward(cfg, sd, *batch)
    errs = maxerr(h, ho), maxerr(pl, plo), maxerr(nl, nlo)
    _, pl32, _ = O.forward(cfg_of(c, bf16=False), sd, *batch)
    seen = maxerr(pl, pl32)
    print(f"case {c.id}: hidden {errs[0]:.2e} pos {errs[1]:.2e} neg {errs[2]:.2e}; pos vs the fp32 oracle {seen:.2e}")
    assert max(errs) < TOL, errs
    assert seen > 10 * TOL                      # the rounding is visible: a gather of the fp32 master would pass nothing here


@cases
def test_autograd_loss_and_gradients_match_the_bf16_oracle(c, monkeypatch):
    from tests.gpu_util import cuda, maxerr
    cfg, sd, model, batch = _setup(c, monkeypatch)
    _assert_plan(c, model, "autograd", c.autograd)
    model.train()                                   # dropout 0
    assert relu_margin(cfg, sd, batch) > RELU_MARGIN            # (on the oracle alone: every ReLU derivative is defined)
    loss_o, grads_o, h_o, pl_o, nl_o = O.grads_of(cfg, sd, batch)
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    h, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    assert maxerr(h, h_o) < TOL and maxerr(pl, pl_o) < TOL and maxerr(nl, nl_o) < TOL
    loss = _bce(pl, nl, pos)
    loss.backward()
    errs = {k: maxerr(p.grad, grads_o[k]) for k, p in model.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"case {c.id}: loss {abs(float(loss.detach()) - float(loss_o)):.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert abs(float(loss.detach()) - float(loss_o)) < TOL
    for k, e in errs.items():
        assert e < TOL, (k, e)


@cases
def test_fused_steps_match_the_bf16_oracle_and_keep_the_shadow_current(c, monkeypatch):
    """two FusedTrainer steps with dropout 0.5 on fresh batches: the training instantiations (<..., 1, ...>), which the autograd
    path does not reach"""
    import srfrd_amd
    from tests.gpu_util import cuda
    from tests.helpers import assert_post_adam, oracle_step_with_grads
    cfg, sd, model, _ = _setup(c, monkeypatch, dropout=0.5)
    model.train()
    base = 77
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=base, use_graph=False)
    _assert_plan(c, model, "fused", c.fused, scratch=tr.n_scratch)
    opt = O.Adam(sd)
    hist = []
    for step in range(2):
        batch = srfrd_amd.synthetic_batch(I, c.L, c.B, seed=c.fused_seed + step, device="cpu")
        loss = tr.step(*cuda(*batch))
        assert relu_margin(cfg, sd, batch[1:], train=True, seed=O.step_seed(base, step + 1)) > RELU_MARGIN
        loss_o, g_o = oracle_step_with_grads(cfg, sd, opt, batch[1:], train=True, seed=O.step_seed(base, step + 1), b0=0)
        hist.append(g_o)
        print(f"case {c.id} step {step}: loss {abs(float(loss.cpu()) - float(loss_o)):.2e}")
        assert abs(float(loss.cpu()) - float(loss_o)) < TOL, step
        table = model._item_param().detach()
        assert torch.equal(model._table16, table.to(torch.bfloat16).view(torch.int16).flatten()), step
    assert_post_adam(model.state_dict(), sd, hist, cfg.D)


@cases
def test_last_position_forward_and_ranking_match_the_bf16_oracle(c, monkeypatch):
    from tests.gpu_util import cuda, maxerr
    cfg, sd, model, batch = _setup(c, monkeypatch)
    _assert_plan(c, model, "last", (c.last_fwd, None))
    model.eval()
    seq, rsq = batch[:2]
    ref = O.predict(cfg, sd, seq, rsq, torch.arange(1, I + 1))
    # on the oracle alone: the order of every user's top 10 is decided by more than twice the tolerance
    top = -np.sort(-ref.numpy(), axis=1)[:, :11]
    assert float((top[:, :-1] - top[:, 1:]).min()) > 2 * TOL
    cand = torch.randint(1, I + 1, (c.B, 31), generator=torch.Generator().manual_seed(c.seed))
    got = model.predict(None, *cuda(seq, rsq), cand.cuda())
    err = maxerr(got, O.predict(cfg, sd, seq, rsq, cand))
    print(f"case {c.id}: predict {err:.2e}")
    assert err < TOL
    idx10, _ = model.topk(None, *cuda(seq, rsq), k=10)
    order = np.argsort(-ref.numpy(), axis=1, kind="stable")[:, :10]
    assert (idx10.cpu().numpy() == order + 1).all()
