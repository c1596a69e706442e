"""-m gpu: the three loss heads at logits of magnitude about 200.  exp(200) overflows fp32, so any path that exponentiates before
it subtracts the maximum gives inf or NaN here, and a running sum that is not rescaled when the maximum moves is off by tens
of orders of magnitude; the other loss tests keep |logit| below about 8, where neither shows.  The inputs
(tests/loss_extreme_cases.py) plant, per head: the maximum at the first candidate, on both sides of a chunk seam and at the
last candidate of a partial chunk, in another candidate split than the target; the target itself as the maximum by a wide
gap; the target far below the maximum; a zero hidden row; log_q up to +-30 with a slot that is the maximum only through its
log_q; a token that loses every negative to hit removal next to one that loses none; for gBCE positives and negatives near
+200 and -200.  Each test asserts from the fp64 logits that its situations occur before it looks at the kernels.

Every output must be finite.  Gradients: ||d||_inf <= 1e-4 ||ref||_inf, as everywhere.  Loss: "mean" / "sum" |d| <= 1e-5
max(1, |ref|); per token (reduction "none") |d_t| <= 1e-5 max(1, |lse_t|, |s_t+|): loss_t = lse_t - s_t+ is a difference of
two fp32 numbers of that magnitude, an ulp of which is 1.2e-7 of it, so the bar leaves about 80 ulp to the dot product, the
running sum and the fast exp / log.

gBCE has no lse, which leaves 1e-5 max(1, |s_t+|).  loss_t = beta softplus(-s_t+) + sum_k softplus(s_tk) is a sum of 1 + K
non-negative terms that reaches 1400 here while |s_t+| may be small, and no fp32 arithmetic meets that bar: plain fp32 torch
on the same inputs does not either.  So the test measures it: e32 = max_t |fp32 torch loss_t - fp64 loss_t| on the same inputs,
and the per-token bar is max(1e-5 max(1, |s_t+|), 8 e32).  DESIGN.md section 15 records e32 and the kernel's error."""
import pytest
import torch

from tests import loss_extreme_cases as X
from tests.loss_refs import head_model, head_table, rel, run_head, sxent_logits_ref, sxent_ref, tneg_ref, tneg_token_loss, xent_ref

pytestmark = pytest.mark.gpu

REDUCTIONS = ("mean", "sum", "none")
_table = head_table


def _model(c, d_item, d_fake):
    return head_model(d_item, d_fake, c["n_items"], X.L, c["E"])


def _check(m, call, ref, h, y, bar, tag):
    """bar (B, L) fp64: the per-token loss bar"""
    d = _table(m).shape[1]
    loss, dh, de = run_head(m, call, h)
    rl, rdh, rde = ref
    assert bool(loss.isfinite().all()) and bool(dh.isfinite().all()) and bool(de.isfinite().all()), tag
    err = (loss.double() - rl).abs()
    print(tag, "loss", float(err.max()), "of", float(rl.abs().max()), "dh", rel(dh, rdh), "de", rel(de, rde))
    if loss.dim():
        worst = (err - bar).argmax()
        assert bool((err <= bar).all()), (tag, int(worst), float(err.view(-1)[worst]), float(bar.view(-1)[worst]))
        assert bool((loss[y == 0] == 0).all()), tag
    else:
        assert float(err) <= 1e-5 * max(1.0, abs(float(rl))), (tag, float(loss), float(rl))
    assert rel(dh, rdh) <= 1e-4, (tag, rel(dh, rdh))
    assert rel(de, rde) <= 1e-4, (tag, rel(de, rde))
    assert float(de[0].abs().max()) == 0.0, tag
    if dh.shape[-1] > d:
        assert float(dh[..., d:].abs().max()) == 0.0, tag
    return loss


def _grid(v, y):
    """per-token values (tokens in position order) -> (B, L), zeros at ignored positions"""
    out = torch.zeros(y.numel(), dtype=torch.float64, device=y.device)
    out[(y.view(-1) != 0)] = v
    return out.view(y.shape)


@pytest.mark.parametrize("d_item, d_fake", X.EXTREME_WIDTHS)
def test_full_catalog(d_item, d_fake):
    c = X.xent_case(d_item, d_fake, seed=d_item)
    X.check_xent_case(c)
    m = _model(c, d_item, d_fake)
    h, y, E = c["h"].cuda(), c["y"].cuda(), c["E"].cuda()
    s = (h.double()[..., :d_item] @ E.double().T)[..., 1:]
    lse, sp = torch.logsumexp(s, -1), s.gather(-1, (y - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
    scale = torch.maximum(lse.abs(), sp.abs()) * (y != 0)
    for red in REDUCTIONS:
        _check(m, lambda hh: m.full_catalog_loss(hh, y, red), xent_ref(h, E, y, red), h, y, 1e-5 * scale.clamp(min=1.0), ("xent", d_item, d_fake, red))


@pytest.mark.parametrize("d_item, d_fake", X.EXTREME_WIDTHS)
def test_shared_negatives(d_item, d_fake):
    c = X.sxent_case(d_item, d_fake, seed=d_item)
    X.check_sxent_case(c)
    m = _model(c, d_item, d_fake)
    h, y, E, neg, log_q = (c[k].cuda() for k in ("h", "y", "E", "neg", "log_q"))
    for lq in (None, log_q):
        _, sp, sn = sxent_logits_ref(h.double(), E.double(), y, neg, lq, True)
        lse = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1)
        scale = _grid(torch.maximum(lse.abs(), sp.abs()), y)
        for red in REDUCTIONS:
            _check(m, lambda hh: m.sampled_softmax_loss(hh, y, neg, lq, True, red),
                   sxent_ref(h, E, y, neg, lq, True, red), h, y, 1e-5 * scale.clamp(min=1.0), ("sxent", d_item, d_fake, lq is not None, red))


@pytest.mark.parametrize("d_item, d_fake", X.EXTREME_WIDTHS)
def test_shared_negatives_all_removed_next_to_none_removed(d_item, d_fake):
    c = X.sxent_hits_case(d_item, d_fake, seed=d_item)
    m = _model(c, d_item, d_fake)
    h, y, E, neg, log_q = (c[k].cuda() for k in ("h", "y", "E", "neg", "log_q"))
    _, sp, sn = sxent_logits_ref(h.double(), E.double(), y, neg, log_q, True)
    tg = y.view(-1)[y.view(-1) != 0]
    assert bool((tg == 40).any()) and bool((~sn[tg == 40].isfinite()).all())            # every slot removed
    assert bool((sn[tg == 41].isfinite().sum(1) == 3).all())                            # none removed (one slot is unused)
    assert 150.0 < max(float(sp.abs().max()), float(sn[sn.isfinite()].abs().max())) < 260.0
    lse = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1)
    scale = _grid(torch.maximum(lse.abs(), sp.abs()), y)
    for red in REDUCTIONS:
        loss = _check(m, lambda hh: m.sampled_softmax_loss(hh, y, neg, log_q, True, red),
                      sxent_ref(h, E, y, neg, log_q, True, red), h, y, 1e-5 * scale.clamp(min=1.0), ("sxent hits", d_item, d_fake, red))
    assert bool((loss[y == 40] == 0).all())


@pytest.mark.parametrize("objective", ["softmax", "gbce"])
@pytest.mark.parametrize("d_item, d_fake", X.EXTREME_WIDTHS)
def test_token_negatives(d_item, d_fake, objective):
    d_item, d_fake, seed = X.tneg_case_args(d_item, d_fake, objective)
    c = X.tneg_case(d_item, d_fake, seed=seed)
    X.check_tneg_case(c)
    m = _model(c, d_item, d_fake)
    h, y, E, neg, log_q = (c[k].cuda() for k in ("h", "y", "E", "neg", "log_q"))
    cases = [(None, 1.0), (log_q, 1.0)] if objective == "softmax" else [(None, 1.0), (None, 0.3)]
    for lq, beta in cases:
        none_ref = tneg_ref(h, E, y, neg, lq, True, "none", objective, beta)[0]
        cc = dict(c, log_q=c["log_q"] if lq is not None else torch.zeros_like(c["log_q"]))
        sp, sn, part = X.tneg_logits(cc, True)
        live = c["y"].view(-1) != 0
        if objective == "softmax":
            lse = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn.masked_fill(~part, -float("inf"))], 1), 1)
            assert float(((lse - sp).view(y.shape).cuda() * (y != 0) - none_ref).abs().max()) < 1e-9
            bar = 1e-5 * (torch.maximum(lse.abs(), sp.abs()) * live).view(y.shape).cuda().clamp(min=1.0)
        else:
            e32 = float((tneg_token_loss(h, E, y, neg, None, True, objective, beta).double() - none_ref).abs().max())
            stated = 1e-5 * (sp.abs() * live).view(y.shape).cuda().clamp(min=1.0)
            bar = stated.clamp(min=8.0 * e32)
            print(("tneg", objective, d_item, beta), "fp32 torch per-token error", e32, "bar at most", float(bar.max()))
        for red in REDUCTIONS:
            loss = _check(m, lambda hh: m.token_negatives_loss(hh, y, neg, objective, lq, beta, True, red),
                          tneg_ref(h, E, y, neg, lq, True, red, objective, beta), h, y, bar,
                          ("tneg", objective, d_item, d_fake, lq is not None, beta, red))
        if objective == "softmax":
            assert float(loss.view(-1)[c["plan"]["all_removed"]]) == 0.0
            assert float(loss.view(-1)[c["plan"]["none_removed"]]) > 0.0
