"""-m gpu: the three loss heads at every item width.  The heads are compiled per width class and chosen at run time: with_ks
(srfrd_xent_common.h) picks one of 16 KS instantiations of each of the six streaming kernels of the two softmax losses from
ceil(d_item / 4), with_shape (srfrd_tneg.hip) one of seven (VEC, NJ) row-gather shapes from d_item and the table's address.
The other loss tests run d_item = 50 and 45 + 5 only; here every d_item in 1..64 runs (tests/test_loss_width_cover.py keeps
the list complete), d_out > d_item with a fake slice of about 1e3 that a single leaked column would carry into the loss, the
gather shapes that only a misaligned table reaches, and the fused train step at D = 32, 64 and 27 + 5.

References are fp64 torch on materialised logits (tests/loss_refs.py).  Tolerances are those of the three loss test files:
loss |d| <= 1e-5 max(1, |ref|); d_hidden and the table gradient ||d||_inf <= 1e-4 ||ref||_inf (no floor: nothing cancels in
these inputs)."""
import ctypes as C

import pytest
import torch

from tests.loss_refs import (ALIGN_OFFSETS, ALIGN_WIDTHS, FAKE_CASES, WIDTHS, head_model, head_table, make_inputs, rel, run_head,
                             shared_negatives, sxent_ref, tneg_ref, tneg_shape, xent_ref)

pytestmark = pytest.mark.gpu

B, L = 5, 13                    # 65 positions: one past the 64-token tile
REDUCTIONS = ("mean", "sum", "none")
_table = head_table


def _model(d_item, d_fake, n_items):
    return head_model(d_item, d_fake, n_items, L)


def _hidden(d_item, d_fake):
    h = torch.randn(B, L, d_item + d_fake, device="cuda") * 0.5
    if d_fake:
        h[..., d_item:] = 1e3 * (1.0 + 0.2 * h[..., d_item:])
    return h


def _targets(n_items, seed):
    """about 30 % ignored positions, one row of the batch without targets, the first and the last catalog id among them"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, n_items + 1, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 0.3] = 0
    y[2] = 0
    flat = y.view(-1)
    nz = (flat != 0).nonzero().view(-1)
    flat[nz[0]] = 1
    flat[nz[-1]] = n_items
    return y


def _check(m, call, ref, h, y, tag):
    """one (loss, reduction) call against its fp64 reference, twice: the second call must give the same bits"""
    d = _table(m).shape[1]
    loss, dh, de = run_head(m, call, h)
    rl, rdh, rde = ref
    el, eh, ee = float((loss.double() - rl).abs().max()), rel(dh, rdh), rel(de, rde)
    print(tag, "loss", el, "dh", eh, "de", ee)
    assert bool(loss.isfinite().all()) and bool(dh.isfinite().all()) and bool(de.isfinite().all()), tag
    assert el <= 1e-5 * max(1.0, float(rl.abs().max())), (tag, loss, rl)
    assert eh <= 1e-4, (tag, eh)
    assert ee <= 1e-4, (tag, ee)
    assert float(de[0].abs().max()) == 0.0, tag
    if dh.shape[-1] > d:                                  # the fake slice
        assert float(dh[..., d:].abs().max()) == 0.0, tag
        # (hidden is a leaf here, so no autograd path to fake_embed exists: this line only pins that the head does not
        # invent one; the exact zero above is the check that can fail)
        assert m.embedding_layer.fake_embed.weight.grad is None
    if loss.dim():
        assert bool((loss[y == 0] == 0).all()), tag
    again = run_head(m, call, h)
    for a, b in zip((loss, dh, de), again):
        assert torch.equal(a, b), tag


def _xent(d_item, d_fake):
    for n_items in (17, 257):                             # a partial 64-row chunk; several chunks and candidate splits
        torch.manual_seed(1000 * d_item + n_items)
        m = _model(d_item, d_fake, n_items)
        h = _hidden(d_item, d_fake)
        y = _targets(n_items, d_item + n_items).cuda()
        for red in REDUCTIONS:
            _check(m, lambda hh: m.full_catalog_loss(hh, y, red), xent_ref(h, _table(m), y, red), h, y,
                   ("xent", d_item, d_fake, n_items, red))


def _sxent(d_item, d_fake):
    for n_items, K in ((17, 1), (257, 65)):
        torch.manual_seed(2000 * d_item + K)
        m = _model(d_item, d_fake, n_items)
        h = _hidden(d_item, d_fake)
        y = _targets(n_items, d_item + K)
        neg = shared_negatives(K, n_items, y, d_item + K)
        if K == 1:
            neg[0] = y[0, (y[0] != 0).nonzero()[0, 0]]    # the one slot is an accidental hit of some token
        else:
            assert bool((neg == 0).any()) and neg.unique().numel() < K and bool((neg.view(-1, 1, 1) == y).any())
        y, neg = y.cuda(), neg.cuda()
        log_q = (torch.randn(K) * 2.0).cuda()
        for lq in (None, log_q):
            for red in REDUCTIONS:
                _check(m, lambda hh: m.sampled_softmax_loss(hh, y, neg, lq, True, red),
                       sxent_ref(h, _table(m), y, neg, lq, True, red), h, y, ("sxent", d_item, d_fake, K, lq is not None, red))


def _tneg_inputs(d_item, n_items, K):
    """(targets, negatives (B, L, K), log_q) on the GPU: id-0 slots, duplicates inside a position, accidental hits"""
    _, neg = make_inputs(B, L, K, n_items, d_item * 1009 + K)
    y = _targets(n_items, d_item + K)
    hit = torch.rand(B, L, K, generator=torch.Generator().manual_seed(K)) < 0.15
    neg = torch.where(hit, y.unsqueeze(-1).expand_as(neg), neg)               # accidental hits of these targets
    if K > 1:
        neg[..., 2] = neg[..., 0]                                             # duplicates inside a position
        part = (neg != 0) & (neg != y.unsqueeze(-1))
        assert bool((neg == 0).any()) and bool(hit.any())
        assert 0.5 < float(part.any(-1)[y != 0].double().mean())              # most tokens have negatives left
    return y.cuda(), neg.cuda(), (torch.randn(B, L, K) * 2.0).cuda()


def _tneg(d_item, d_fake):
    for n_items, K in ((17, 1), (257, 65)):
        torch.manual_seed(3000 * d_item + K)
        m = _model(d_item, d_fake, n_items)
        h = _hidden(d_item, d_fake)
        y, neg, log_q = _tneg_inputs(d_item, n_items, K)
        cases = [("softmax", None, 1.0), ("softmax", log_q, 1.0)]
        if not d_fake:                                    # gbce is refused for SRFRN
            cases += [("gbce", None, 1.0), ("gbce", None, 0.3)]
        for objective, lq, beta in cases:
            for red in REDUCTIONS:
                _check(m, lambda hh: m.token_negatives_loss(hh, y, neg, objective, lq, beta, True, red),
                       tneg_ref(h, _table(m), y, neg, lq, True, red, objective, beta), h, y,
                       ("tneg", d_item, d_fake, K, objective, lq is not None, beta, red))


HEADS = {"xent": _xent, "sxent": _sxent, "tneg": _tneg}


@pytest.mark.parametrize("d_item", WIDTHS)
@pytest.mark.parametrize("head", list(HEADS))
def test_every_width_against_fp64(head, d_item):
    HEADS[head](d_item, 0)


@pytest.mark.parametrize("d_item, d_fake", FAKE_CASES)
@pytest.mark.parametrize("head", list(HEADS))
def test_fake_slice_never_reaches_the_loss(head, d_item, d_fake):
    HEADS[head](d_item, d_fake)


def test_gbce_is_refused_for_srfrn_at_another_width():
    m = _model(27, 5, 100)
    h = _hidden(27, 5)
    y = _targets(100, 1).cuda()
    neg = torch.randint(1, 101, (B, L, 3), device="cuda")
    with pytest.raises(ValueError, match="SRFRN"):
        m.token_negatives_loss(h, y, neg, objective="gbce")
    m.token_negatives_loss(h, y, neg, objective="softmax")


@pytest.mark.parametrize("d_item", ALIGN_WIDTHS)
def test_tneg_gather_shapes_of_a_misaligned_table(d_item):
    """with_shape narrows the row loads when the table does not start on a 16- or 8-byte boundary.  torch's allocations always
    do, so the launch-level functions the srfrd::tneg_* ops call are given a table that starts 0, 1 and 2 floats into a larger
    buffer.  The three results agree to the tolerances, not bitwise: the shapes group the dot product's sum differently."""
    from srfrd_amd import _lib
    from srfrd_amd.loss_heads import TNEG, launch_bwd, launch_fwd
    n_items, K = 257, 65
    torch.manual_seed(4000 + d_item)
    m = _model(d_item, 0, n_items)
    lay = m.layout
    h = _hidden(d_item, 0)
    y, neg, log_q = _tneg_inputs(d_item, n_items, K)
    E = _table(m).detach().clone()
    buf = torch.zeros(E.numel() + 8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ones = torch.ones(B, L, device="cuda")
    shapes = set()
    for objective, lq, beta in (("softmax", log_q, 1.0), ("gbce", None, 0.7)):
        code = _lib.TNEG_OBJECTIVES[objective]
        rl, _, _ = tneg_ref(h, E, y, neg, lq, True, "none", objective, beta)
        rs, rdh, rde = tneg_ref(h, E, y, neg, lq, True, "sum", objective, beta)
        got = []
        for off in ALIGN_OFFSETS:
            buf.zero_()
            view = buf[off:off + E.numel()].view_as(E)
            view.copy_(E)
            addr = view.data_ptr()
            assert addr == buf.data_ptr() + 4 * off
            shapes.add(tneg_shape(d_item, addr))
            out = []
            for _ in range(2):
                tl, lse, stats = launch_fwd(TNEG, lay, C.c_void_p(addr), h, y, (neg, lq, code, beta, True))
                dh, de = launch_bwd(TNEG, lay, C.c_void_p(addr), h, y, (neg, lq, code, beta, True), lse, ones)
                out.append((tl, stats, dh, de))
            for a, b in zip(*out):
                assert torch.equal(a, b), (objective, off)
            tl, stats, dh, de = out[0]
            tag = (objective, d_item, off, tneg_shape(d_item, addr))
            el, es = float((tl.double() - rl).abs().max()), abs(float(stats[0]) - float(rs))
            print(tag, "loss", el, es, "dh", rel(dh, rdh), "de", rel(de, rde))
            assert el <= 1e-5 * max(1.0, float(rl.abs().max())), tag
            assert es <= 1e-5 * max(1.0, abs(float(rs))) and float(stats[1]) == float((y != 0).sum()), tag
            assert rel(dh, rdh) <= 1e-4 and rel(de, rde) <= 1e-4, tag
            assert float(de[0].abs().max()) == 0.0 and bool((tl[y == 0] == 0).all()), tag
            got.append((tl, dh, de))
        for tl, dh, de in got[1:]:
            assert float((tl - got[0][0]).abs().max()) <= 1e-5 * max(1.0, float(rl.abs().max()))
            assert rel(dh, got[0][1]) <= 1e-4 and rel(de, got[0][2]) <= 1e-4
    want = {(4, 1), (1, d_item // 16), (2, 1) if d_item <= 32 else (2, 2)}
    assert shapes == want, (shapes, want)


# ------------------------------------------------------------------------------------------------ the fused train step
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("L_", [20, 50])
@pytest.mark.parametrize("kind, d_item, d_fake", [("SASRec", 32, 0), ("SASRec", 64, 0), ("SRFRN", 27, 5)])
@pytest.mark.parametrize("loss", ["softmax", "sampled_softmax"])
def test_one_train_step_against_fp64_oracle_at_other_widths(loss, kind, d_item, d_fake, L_, use_graph):
    """test_one_step_against_fp64_oracle of tests/test_gpu_ce_trainer.py, its tolerances, at the widths a user who sets
    hidden_units to 32 or 64 trains with: the width-generic heads behind the width-generic encoder in FusedTrainer"""
    import srfrd_amd
    from oracle import srfrd_oracle as O
    from tests.gpu_util import build_model, random_sd
    from tests.helpers import assert_post_adam
    from tests.test_gpu_ce_trainer import _batch, _oracle_step
    cfg = O.Cfg(kind, 300, L_, d_item, d_fake=d_fake) if d_fake else O.Cfg(kind, 300, L_, d_item)
    sd = random_sd(cfg, 8)
    Bt = 8
    model = build_model(cfg, sd).train()
    counts = torch.arange(cfg.item_number + 1.0) ** 0.5
    kw = dict(num_negatives=512, neg_counts=counts, neg_alpha=0.75) if loss == "sampled_softmax" else {}
    tr = srfrd_amd.FusedTrainer(model, Bt, L_, loss=loss, use_graph=use_graph, **kw)
    batch = _batch(cfg, Bt, 5)
    got = float(tr.step(None, *batch))
    neg, log_q = (tr.negatives.cpu(), tr.log_q.cpu().double()) if loss == "sampled_softmax" else (None, None)
    want, grads, sd_step = _oracle_step(cfg, sd, batch, loss, neg, log_q, 0.0)
    print(loss, kind, d_item, d_fake, L_, use_graph, "loss", got, want)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    assert_post_adam(model.state_dict(), sd_step, [{k: g.float() for k, g in grads.items()}], cfg.D)
