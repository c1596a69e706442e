"""-m gpu: sampled softmax cross-entropy with shared negatives (model.sampled_softmax_loss, srfrd_sxent_fwd / _bwd) against
fp64 torch on materialised logits: s_t+ = <h_t, E[y_t]>, s_tj = <h_t, E[n_j]> - log_q[j], id-0 slots (and, with hit
removal, slots equal to the target) masked to -inf, loss_t = logsumexp([s_t+, s_t.]) - s_t+.
Tolerances as tests/test_gpu_xent.py: loss |d| <= 1e-5 max(1, |ref|); d_hidden and the table gradient ||d||_inf <= 1e-4
||ref||_inf; whole-model parameter gradients 1e-4 absolute; post-Adam weights by tests/helpers.assert_post_adam.  One
addition: where a gradient's terms cancel (a catalog of one item, or every slot holding the target's own id: the target
and its copies share one logit), the exact gradient is ~0 and fp32 rounding is relative to the terms, not to it; the
inf-norm scale is therefore floored at 10 % of the inf-norm of the same gradient summed over absolute values."""
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.helpers import assert_post_adam
from tests.loss_refs import rel as _rel
from tests.loss_refs import shared_negatives as _negatives
from tests.loss_refs import sxent_logits_ref as _logits_ref
from tests.loss_refs import sxent_ref as _ref

pytestmark = pytest.mark.gpu


def _sasrec(n_items, d=50, L=20):
    import srfrd_amd
    return srfrd_amd.SASRec(n_items, L, d, 0.0, 2, 1, "cuda").to("cuda")


def _targets(B, L, n_items, seed, empty_rows=(), zero_frac=0.3):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, n_items + 1, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < zero_frac] = 0
    for b in empty_rows:
        y[b] = 0
    return y


def _run(m, h, y, neg, log_q=None, remove=True, reduction="mean"):
    table = m.item_emb.weight
    table.grad = None
    hh = h.detach().clone().requires_grad_(True)
    loss = m.sampled_softmax_loss(hh, y, neg, log_q, remove, reduction)
    loss.backward(torch.ones_like(loss))
    return loss.detach(), hh.grad, table.grad.clone()


def _check(m, h, y, neg, log_q, remove, red):
    loss, dh, de = _run(m, h, y, neg, log_q, remove, red)
    rl, rdh, rde, ah, ae = _ref(h, m.item_emb.weight, y, neg, log_q, remove, red, with_abs=True)
    assert float((loss.double() - rl).abs().max()) <= 1e-5 * max(1.0, float(rl.abs().max())), (red, remove, loss, rl)
    assert _rel(dh, rdh, ah) <= 1e-4, (red, remove, _rel(dh, rdh, ah))
    assert _rel(de, rde, ae) <= 1e-4, (red, remove, _rel(de, rde, ae))
    assert float(de[0].abs().max()) == 0.0
    if red == "none":
        assert bool((loss[y == 0] == 0).all())
    return loss


@pytest.mark.parametrize("K", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_items", [1, 63, 64, 65, 5000])
def test_op_matches_fp64_sampled_softmax(n_items, K):
    torch.manual_seed(n_items * 1009 + K)
    B, L, d = 5, 13, 50                                 # B * L = 65: not a multiple of the 64-token tile
    m = _sasrec(n_items, d, L)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.5)
    h = torch.randn(B, L, d, device="cuda") * 0.5
    y = _targets(B, L, n_items, n_items + K, empty_rows=(2,)).cuda()
    neg = _negatives(K, n_items, y, K).cuda()
    log_q = (torch.randn(K) * 2.0).cuda()
    for remove in (True, False):
        for lq in (None, log_q):
            sums = {}
            for red in ("mean", "sum", "none"):
                sums[red] = _check(m, h, y, neg, lq, remove, red)
            cnt = int((y != 0).sum())
            s, none_sum = float(sums["sum"]), float(sums["none"].double().sum())
            assert abs(s - none_sum) <= 1e-5 * max(1.0, abs(s))
            assert abs(float(sums["mean"]) - s / cnt) <= 1e-5 * max(1.0, abs(float(sums["mean"])))


def test_no_targets_gives_nan_mean_and_zero_gradients():
    m = _sasrec(100)
    h = torch.randn(3, 7, 50, device="cuda")
    y = torch.zeros(3, 7, dtype=torch.int64, device="cuda")
    neg = torch.randint(0, 101, (40,), device="cuda")
    loss, dh, de = _run(m, h, y, neg, reduction="mean")
    assert bool(torch.isnan(loss))
    assert float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0
    s, dh, de = _run(m, h, y, neg, reduction="sum")
    assert float(s) == 0.0 and float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0


def test_every_slot_an_accidental_hit_gives_zero_loss_and_gradients():
    m = _sasrec(100)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.5)
    h = torch.randn(4, 9, 50, device="cuda")
    y = torch.full((4, 9), 17, dtype=torch.int64, device="cuda")
    y[1, :3] = 0
    neg = torch.tensor([17, 0, 17, 17, 0], device="cuda")
    log_q = torch.randn(5, device="cuda")
    for red in ("mean", "sum", "none"):
        loss, dh, de = _run(m, h, y, neg, log_q, True, red)
        assert float(loss.abs().max()) == 0.0, red
        assert float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0, red
    # without hit removal the same slots are candidates
    loss, dh, de = _run(m, h, y, neg, log_q, False, "mean")
    rl, rdh, rde, ah, ae = _ref(h, m.item_emb.weight, y, neg, log_q, False, "mean", with_abs=True)
    assert abs(float(loss) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl))) and float(loss) > 0
    assert _rel(dh, rdh, ah) <= 1e-4 and _rel(de, rde, ae) <= 1e-4


@pytest.mark.parametrize("n_items", [65, 5000])
def test_whole_catalog_as_negatives_is_full_catalog_loss(n_items):
    torch.manual_seed(4)
    m = _sasrec(n_items, 50, 20)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.5)
    h = torch.randn(6, 20, 50, device="cuda") * 0.5
    y = _targets(6, 20, n_items, 3, empty_rows=(1,)).cuda()
    neg = torch.arange(1, n_items + 1, device="cuda")
    for red in ("mean", "none"):
        loss, dh, de = _run(m, h, y, neg, None, True, red)
        m.item_emb.weight.grad = None
        hh = h.clone().requires_grad_(True)
        full = m.full_catalog_loss(hh, y, red)
        full.backward(torch.ones_like(full))
        fdh, fde = hh.grad, m.item_emb.weight.grad
        assert float((loss.double() - full.detach().double()).abs().max()) <= 1e-5 * max(1.0, float(full.detach().abs().max()))
        assert _rel(dh, fdh) <= 1e-4 and _rel(de, fde) <= 1e-4


def test_bitwise_deterministic_with_duplicate_ids():
    torch.manual_seed(0)
    n = 50_000
    m = _sasrec(n, 50, 50)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.3)
    h = torch.randn(64, 50, 50, device="cuda") * 0.3
    y = _targets(64, 50, 300, 5).cuda()                 # few distinct targets: long runs of equal keys
    neg = torch.randint(1, 300, (2048,), device="cuda")   # heavy duplication, many accidental hits
    log_q = torch.randn(2048, device="cuda")
    for red in ("mean", "none"):
        a = _run(m, h, y, neg, log_q, True, red)
        b = _run(m, h, y, neg, log_q, True, red)
        for x, z in zip(a, b):
            assert torch.equal(x, z), red


def test_srfrn_fake_slice_gets_no_gradient():
    from tests.gpu_util import build_model, random_sd
    cfg = O.Cfg("SRFRN", 300, 20, 45, d_fake=5)
    sd = random_sd(cfg, 2)
    model = build_model(cfg, sd)
    torch.manual_seed(3)
    h = torch.randn(6, 20, cfg.d_out, device="cuda", requires_grad=True)
    y = _targets(6, 20, 300, 4).cuda()
    neg = _negatives(200, 300, y, 1).cuda()
    loss = model.sampled_softmax_loss(h, y, neg)
    loss.backward()
    assert float(h.grad[..., cfg.d_item:].abs().max()) == 0.0
    assert model.embedding_layer.fake_embed.weight.grad is None
    E = model.embedding_layer.item_embed.weight
    rl, rdh, rde = _ref(h, E, y, neg, None, True, "mean")
    assert abs(float(loss.detach()) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl)))
    assert _rel(h.grad[..., :cfg.d_item], rdh[..., :cfg.d_item]) <= 1e-4
    assert _rel(E.grad, rde) <= 1e-4


def _kind_cfg(kind, L, dropout=0.0):
    I = 300
    if kind == "SASRec":
        return O.Cfg(kind, I, L, 50, dropout=dropout)
    if kind in ("SRFR", "SRFRN"):
        return O.Cfg(kind, I, L, 45, d_fake=5, dropout=dropout)
    return O.Cfg(kind, I, L, 50, n_labels=3, dropout=dropout)


KINDS = ("SASRec", "SRFR", "SRFRN", "SRFU_B")


@pytest.mark.parametrize("L", [20, 50])
@pytest.mark.parametrize("kind", KINDS)
def test_through_encoder_train_dropout_matches_torch_materialised(kind, L):
    """Whole-model gradients of the fused loss against the same model (same weights, same dropout masks) with torch's
    materialised fp32 sampled softmax on its own hidden states; L = 50 runs the ragged encoder plan."""
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr, random_sd
    cfg = _kind_cfg(kind, L, dropout=0.5)
    sd = random_sd(cfg, 5)
    batch = srfrd_amd.synthetic_batch(cfg.item_number, L, 16, seed=13, device="cpu", min_len=1)[1:]
    seq, rsq, pos = cuda(*batch[:3])
    neg = _negatives(500, cfg.item_number, pos, 9).cuda()
    log_q = torch.randn(500, device="cuda")
    seed = 0xC0FFEE
    grads = []
    for fused in (True, False):
        model = build_model(cfg, sd).train()
        model._next_seed = lambda: seed
        hidden, _, _ = model(None, seq, rsq)
        if fused:
            loss = model.sampled_softmax_loss(hidden, pos, neg, log_q)
        else:
            E = dict(model.named_parameters())[O.key_item(cfg)]
            tok, sp, sn = _logits_ref(hidden, E, pos, neg, log_q, True)
            loss = (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()
        loss.backward()
        grads.append((float(loss.detach()), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (lf, gf), (lt, gt) = grads
    assert abs(lf - lt) <= 1e-5 * max(1.0, abs(lt))
    assert set(gf) == set(gt)
    for k in gt:
        assert maxerr(gf[k], gt[k]) < 1e-4, (k, maxerr(gf[k], gt[k]))


def _oracle_sampled_grads(cfg, sd, batch, neg, log_q):
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    seq, rsq, pos = batch[0], batch[1], batch[2]
    h, _, _ = O.forward(cfg, leaves, seq, rsq)
    E = O.item_table(cfg, leaves)
    tok, sp, sn = _logits_ref(h, E, pos, neg, log_q, True)
    loss = (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).clone() for k, v in leaves.items()}
    grads[O.key_item(cfg)][0].zero_()
    if cfg.kind in ("SRFR", "SRFRN"):
        grads[O.key_side(cfg)][0].zero_()
    return loss.detach(), grads, {k: v.detach().clone() for k, v in leaves.items()}


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_and_one_adam_step_against_oracle(kind):
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr, random_sd
    cfg = _kind_cfg(kind, 20)
    sd = random_sd(cfg, 7)
    batch = srfrd_amd.synthetic_batch(cfg.item_number, cfg.max_len, 8, seed=11, device="cpu", min_len=1)[1:]
    neg, log_q = srfrd_amd.sample_negatives(cfg.item_number, 256, counts=torch.arange(cfg.item_number + 1.0), alpha=0.75,
                                            generator=torch.Generator().manual_seed(3), device="cpu")
    loss_o, grads_o, sd64 = _oracle_sampled_grads(cfg, sd, batch, neg, log_q.double())
    for opt_kind in ("srfrd", "torch"):
        model = build_model(cfg, sd).train()
        seq, rsq, pos = cuda(*batch[:3])
        params = list(model.parameters())
        opt = srfrd_amd.Adam(params, lr=1e-3, betas=(0.9, 0.98)) if opt_kind == "srfrd" else \
            torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98))
        hidden, _, _ = model(None, seq, rsq)
        loss = model.sampled_softmax_loss(hidden, pos, neg.cuda(), log_q.cuda())
        loss.backward()
        assert abs(float(loss.detach()) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
        for k, p in model.named_parameters():
            assert maxerr(p.grad, grads_o[k]) < 1e-4, (k, maxerr(p.grad, grads_o[k]))
        opt.step()
        sd_step = {k: v.clone() for k, v in sd64.items()}
        O.Adam(sd_step, lr=1e-3, betas=(0.9, 0.98)).step(sd_step, grads_o)
        assert_post_adam(model.state_dict(), sd_step, [{k: g.float() for k, g in grads_o.items()}], cfg.D)


def test_c2_size_against_materialised_fp64():
    torch.manual_seed(1)
    import srfrd_amd
    B, L, n, K = 512, 50, 50_000, 4096
    m = _sasrec(n, 50, L)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.3)
    _, seq, _, pos, *_ = srfrd_amd.synthetic_batch(n, L, B, seed=21, device="cuda")
    h = torch.randn(B, L, 50, device="cuda") * 0.3
    neg, log_q = srfrd_amd.sample_negatives(n, K, generator=torch.Generator(device="cuda").manual_seed(5))
    loss, dh, de = _run(m, h, pos, neg, log_q, True, "mean")
    rl, rdh, rde = _ref(h, m.item_emb.weight, pos, neg, log_q, True, "mean")
    assert abs(float(loss) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl)))
    assert _rel(dh, rdh) <= 1e-4 and _rel(de, rde) <= 1e-4


def test_c5_size_against_materialised_fp64():
    torch.manual_seed(2)
    B, L, n, K, d = 64, 200, 1_000_000, 8192, 50
    m = _sasrec(n, d, L)
    with torch.no_grad():
        m.item_emb.weight.normal_(0, 0.3)
    y = _targets(B, L, n, 9, empty_rows=(5,)).cuda()
    h = torch.randn(B, L, d, device="cuda") * 0.3
    import srfrd_amd
    counts = torch.rand(n + 1, generator=torch.Generator().manual_seed(6)) ** 4
    neg, log_q = srfrd_amd.sample_negatives(n, K, counts=counts.cuda(), generator=torch.Generator(device="cuda").manual_seed(7))
    loss, dh, de = _run(m, h, y, neg, log_q, True, "mean")
    rl, rdh, rde = _ref(h, m.item_emb.weight, y, neg, log_q, True, "mean")
    assert abs(float(loss) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl)))
    assert _rel(dh, rdh) <= 1e-4 and _rel(de, rde) <= 1e-4


def test_refusals():
    m = _sasrec(100)
    h = torch.randn(2, 20, 50, device="cuda")
    y = torch.ones(2, 20, dtype=torch.int64, device="cuda")
    neg = torch.tensor([1, 2, 3], device="cuda")
    m.validate_ids = "eager"
    with pytest.raises(IndexError):
        m.sampled_softmax_loss(h, y, torch.tensor([1, 101, 3], device="cuda"))
    with pytest.raises(IndexError):
        m.sampled_softmax_loss(h, y, torch.tensor([1, -1, 3], device="cuda"))
    m.sampled_softmax_loss(h, y, torch.tensor([0, 100, 3], device="cuda"))       # 0 (unused slot) and n_items are in range
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h.double(), y, neg)
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h[:, :, :40], y, neg)
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y[:, :10], neg)
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg.view(1, 3))
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg.float())
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg[:0])
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg, log_q=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg, log_q=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        m.sampled_softmax_loss(h, y, neg, reduction="avg")
    m.use_bf16_table(True)
    with pytest.raises(RuntimeError, match="fp32 item table"):
        m.sampled_softmax_loss(h, y, neg)
