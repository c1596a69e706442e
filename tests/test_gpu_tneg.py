"""-m gpu: the losses with K negatives per position (model.token_negatives_loss, srfrd_tneg_fwd / _bwd and
srfrd_table_reduce_rank1) against fp64 torch on materialised logits: s_t+ = <h_t, E[y_t]>, s_tk = <h_t, E[n_tk]>, id-0 slots
(and, with hit removal, slots equal to the target) masked;
    softmax  loss_t = logsumexp([s_t+, s_tk - log_q[t, k]]) - s_t+        gbce  loss_t = beta softplus(-s_t+) + sum_k softplus(s_tk)
Tolerances are those of tests/test_gpu_sxent.py and tests/test_gpu_train.py: loss |d| <= 1e-5 max(1, |ref|); d_hidden and the
table gradient ||d||_inf <= 1e-4 ||ref||_inf, the scale floored at 10 % of the inf-norm of the same gradient summed over
absolute values where terms cancel (tests/test_gpu_sxent.py says why); whole-model parameter gradients and the golden loss
1e-4 absolute; post-Adam weights by tests/helpers.assert_post_adam."""
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.helpers import KINDS as GOLDEN_KINDS
from tests.helpers import assert_post_adam, golden_cfg, load_golden, sub
from tests.loss_refs import make_inputs
from tests.loss_refs import rel as _rel
from tests.loss_refs import tneg_mean_loss as _torch_loss
from tests.loss_refs import tneg_ref as _ref

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # tests/test_gpu_train.py


def _model(kind, n_items, L=20):
    import srfrd_amd
    if kind == "SRFRN":
        return srfrd_amd.SRFRN(n_items, L, 45, 5, 0.0, 2, 1, "cuda").to("cuda")
    return srfrd_amd.SASRec(n_items, L, 50, 0.0, 2, 1, "cuda").to("cuda")


def _table(m):
    return m.item_emb.weight if hasattr(m, "item_emb") else m.embedding_layer.item_embed.weight


def degenerate_fraction(y, neg, remove):
    """fraction of the tokens none of whose slots takes part"""
    live = y != 0
    part = neg != 0
    if remove:
        part = part & (neg != y.unsqueeze(-1))
    return float((~part.any(-1))[live].double().mean())


def test_input_generator_keeps_the_degenerate_branch_a_minority():
    """CPU arithmetic only (kept in this file so that the comparison below cannot run on inputs that bypass it)"""
    for K in (3, 64, 65, 257):
        y, neg = make_inputs(5, 13, K, 1000, 1000 * 1009 + K)
        for remove in (True, False):
            assert 0.0 < degenerate_fraction(y, neg, remove) < 0.5, (K, remove)


def _run(m, h, y, neg, objective="softmax", log_q=None, beta=1.0, remove=True, reduction="mean"):
    table = _table(m)
    table.grad = None
    hh = h.detach().clone().requires_grad_(True)
    loss = m.token_negatives_loss(hh, y, neg, objective, log_q, beta, remove, reduction)
    loss.backward(torch.ones_like(loss))
    return loss.detach(), hh.grad, table.grad.clone()


def _check(m, h, y, neg, objective, log_q, beta, remove, red, floor=True):
    d = _table(m).shape[1]
    loss, dh, de = _run(m, h, y, neg, objective, log_q, beta, remove, red)
    rl, rdh, rde, ah, ae = _ref(h, _table(m), y, neg, log_q, remove, red, objective, beta, with_abs=True)
    if not floor:
        ah = ae = 0.0
    tag = (objective, log_q is not None, beta, remove, red)
    print(tag, "loss", float((loss.double() - rl).abs().max()), "dh", _rel(dh, rdh, ah), "de", _rel(de, rde, ae))
    assert float((loss.double() - rl).abs().max()) <= 1e-5 * max(1.0, float(rl.abs().max())), (tag, loss, rl)
    assert _rel(dh, rdh, ah) <= 1e-4, (tag, _rel(dh, rdh, ah))
    assert _rel(de, rde, ae) <= 1e-4, (tag, _rel(de, rde, ae))
    assert float(de[0].abs().max()) == 0.0
    assert float(dh[..., d:].abs().max()) == 0.0 if dh.shape[-1] > d else True
    if red == "none":
        assert bool((loss[y == 0] == 0).all())
    return loss


@pytest.mark.parametrize("K", [1, 3, 64, 65, 257])
@pytest.mark.parametrize("n_items", [1, 7, 1000])
@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_op_matches_fp64_materialised(kind, n_items, K):
    torch.manual_seed(n_items * 1009 + K)
    B, L = 5, 13
    m = _model(kind, n_items, L)
    with torch.no_grad():
        _table(m).normal_(0, 0.5)
    h = torch.randn(B, L, m.layout.d_out, device="cuda") * 0.5
    y, neg = make_inputs(B, L, K, n_items, n_items * 1009 + K)
    if n_items == 1000 and K >= 3:
        for remove in (True, False):
            assert 0.0 < degenerate_fraction(y, neg, remove) < 0.5
    y, neg = y.cuda(), neg.cuda()
    log_q = (torch.randn(B, L, K) * 2.0).cuda()
    cases = [("softmax", lq, 1.0) for lq in (None, log_q)]
    if kind != "SRFRN":
        cases += [("gbce", None, beta) for beta in (1.0, 0.3)]
    for objective, lq, beta in cases:
        for remove in (True, False):
            sums = {red: _check(m, h, y, neg, objective, lq, beta, remove, red) for red in ("mean", "sum", "none")}
            cnt = int((y != 0).sum())
            s, none_sum = float(sums["sum"]), float(sums["none"].double().sum())
            assert abs(s - none_sum) <= 1e-5 * max(1.0, abs(s))
            assert abs(float(sums["mean"]) - s / cnt) <= 1e-5 * max(1.0, abs(float(sums["mean"])))


@pytest.mark.parametrize("kind", [k for k in GOLDEN_KINDS if k != "SRFRN"])
def test_gbce_k1_beta1_is_the_reference_loss_on_the_golden_fixtures(kind):
    """The fixtures the reference's own classes generated (l2_emb = 0): loss0 and every parameter gradient."""
    from tests.gpu_util import build_model, cuda, maxerr
    g, sd, batch = load_golden(kind)
    cfg = golden_cfg(kind)
    model = build_model(cfg, sd).train()            # dropout_rate = 0 in the golden config
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    h = model(None, seq, rsq)[0]
    loss = model.token_negatives_loss(h, pos, neg.unsqueeze(-1), objective="gbce", beta=1.0, remove_accidental_hits=False)
    loss.backward()
    print(kind, "loss", float(loss.detach()), float(g["loss0"]))
    assert abs(float(loss.detach()) - float(g["loss0"])) < TOL
    gg = sub(g, "g/")
    errs = {k: maxerr(p.grad if p.grad is not None else torch.zeros_like(p), gg[k]) for k, p in model.named_parameters()}
    print(kind, "max gradient error", max(errs.values()))
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, f"gradient mismatch: {bad}"
    assert set(errs) == set(gg)


def test_gbce_is_refused_for_srfrn():
    from tests.gpu_util import build_model, cuda
    g, sd, batch = load_golden("SRFRN")
    model = build_model(golden_cfg("SRFRN"), sd)
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    h = model(None, seq, rsq)[0]
    with pytest.raises(ValueError, match="SRFRN"):
        model.token_negatives_loss(h, pos, neg.unsqueeze(-1), objective="gbce")
    model.token_negatives_loss(h, pos, neg.unsqueeze(-1), objective="softmax")


def test_shared_ids_at_every_position_is_sampled_softmax_loss():
    torch.manual_seed(4)
    n_items, B, L, K = 5000, 6, 20, 200
    m = _model("SASRec", n_items, L)
    with torch.no_grad():
        _table(m).normal_(0, 0.5)
    h = torch.randn(B, L, 50, device="cuda") * 0.5
    y, _ = make_inputs(B, L, 1, n_items, 3, empty_rows=(1,))
    y = y.cuda()
    g = torch.Generator().manual_seed(8)
    shared = torch.randint(0, n_items + 1, (K,), generator=g)
    shared[5::9] = y[y != 0][:len(range(5, K, 9))].cpu()          # accidental hits
    shared = shared.cuda()
    log_q = torch.randn(K, device="cuda")
    neg3, lq3 = shared.expand(B, L, K).contiguous(), log_q.expand(B, L, K).contiguous()
    for remove in (True, False):
        for red in ("mean", "none"):
            loss, dh, de = _run(m, h, y, neg3, "softmax", lq3, 1.0, remove, red)
            _table(m).grad = None
            hh = h.clone().requires_grad_(True)
            ref = m.sampled_softmax_loss(hh, y, shared, log_q, remove, red)
            ref.backward(torch.ones_like(ref))
            assert float((loss.double() - ref.detach().double()).abs().max()) <= 1e-5 * max(1.0, float(ref.detach().abs().max()))
            assert _rel(dh, hh.grad) <= 1e-4 and _rel(de, _table(m).grad) <= 1e-4


@pytest.mark.parametrize("kind", ["SASRec", "SRFR", "SRFU_B"])
def test_gbce_k1_is_the_models_own_bce_through_autograd(kind):
    """K = 1, beta = 1 against the loss formed from the model's own pos_logits / neg_logits (the existing autograd path)"""
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr, random_sd
    cfg = _kind_cfg(kind, 20)
    sd = random_sd(cfg, 3)
    batch = srfrd_amd.synthetic_batch(cfg.item_number, 20, 16, seed=5, device="cpu", min_len=1)[1:]
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    out = []
    for fused in (True, False):
        model = build_model(cfg, sd).train()        # dropout 0
        if fused:
            h = model(None, seq, rsq)[0]
            loss = model.token_negatives_loss(h, pos, neg.unsqueeze(-1), "gbce", None, 1.0, False, "mean")
        else:
            _, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
            keep = pos != 0
            sp = torch.nn.functional.softplus
            loss = sp(-pl[keep]).mean() + sp(nl[keep]).mean()
        loss.backward()
        out.append((float(loss.detach()), {k: (p.grad if p.grad is not None else torch.zeros_like(p)).clone()
                                           for k, p in model.named_parameters()}))
    (lf, gf), (lt, gt) = out
    assert abs(lf - lt) <= 1e-5 * max(1.0, abs(lt))
    for k in gt:
        assert maxerr(gf[k], gt[k]) < TOL, (k, maxerr(gf[k], gt[k]))


def test_bitwise_deterministic_with_runs_longer_than_the_split():
    from srfrd_amd import _lib
    torch.manual_seed(0)
    n, B, L, K = 50_000, 16, 50, 64
    m = _model("SASRec", n, L)
    with torch.no_grad():
        _table(m).normal_(0, 0.3)
    h = torch.randn(B, L, 50, device="cuda") * 0.3
    g = torch.Generator().manual_seed(5)
    y = torch.randint(1, 6, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 0.3] = 0
    neg = torch.randint(1, 6, (B, L, K), generator=g)              # every id drawn from 5 items
    log_q = torch.randn(B, L, K, generator=g)
    # key histogram of the contribution list: the participating slots of the live positions, and their targets
    live = y != 0
    part = live.unsqueeze(-1) & (neg != y.unsqueeze(-1))
    hist = torch.bincount(neg[part], minlength=6) + torch.bincount(y[live], minlength=6)
    assert int(hist[1:].max()) > 4 * _lib.TNEG_SPLIT_ROWS            # runs that cross several segments of the rank-1 reduce
    y, neg, log_q = y.cuda(), neg.cuda(), log_q.cuda()
    for objective, lq in (("softmax", log_q), ("gbce", None)):
        for red in ("mean", "none"):
            a = _run(m, h, y, neg, objective, lq, 0.7, True, red)
            b = _run(m, h, y, neg, objective, lq, 0.7, True, red)
            for x, z in zip(a, b):
                assert torch.equal(x, z), (objective, red)
            rl, rdh, rde = _ref(h, _table(m), y, neg, lq, True, red, objective, 0.7)
            assert float((a[0].double() - rl).abs().max()) <= 1e-5 * max(1.0, float(rl.abs().max()))
            assert _rel(a[1], rdh) <= 1e-4 and _rel(a[2], rde) <= 1e-4, (objective, red, _rel(a[1], rdh), _rel(a[2], rde))


def test_no_targets_gives_nan_mean_and_zero_gradients():
    m = _model("SASRec", 100)
    h = torch.randn(3, 7, 50, device="cuda")
    y = torch.zeros(3, 7, dtype=torch.int64, device="cuda")
    neg = torch.randint(0, 101, (3, 7, 40), device="cuda")
    for objective in ("softmax", "gbce"):
        loss, dh, de = _run(m, h, y, neg, objective, reduction="mean")
        assert bool(torch.isnan(loss))
        assert float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0
        s, dh, de = _run(m, h, y, neg, objective, reduction="sum")
        assert float(s) == 0.0 and float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0


def test_every_slot_removed_gives_zero_loss_and_gradients():
    m = _model("SASRec", 100)
    with torch.no_grad():
        _table(m).normal_(0, 0.5)
    h = torch.randn(4, 9, 50, device="cuda")
    y = torch.full((4, 9), 17, dtype=torch.int64, device="cuda")
    y[1, :3] = 0
    neg = torch.tensor([17, 0, 17, 17, 0], device="cuda").expand(4, 9, 5).contiguous()
    log_q = torch.randn(4, 9, 5, device="cuda")
    for red in ("mean", "sum", "none"):
        loss, dh, de = _run(m, h, y, neg, "softmax", log_q, 1.0, True, red)
        assert float(loss.abs().max()) == 0.0, red
        assert float(dh.abs().max()) == 0.0 and float(de.abs().max()) == 0.0, red
    # without hit removal the same slots are candidates
    _check(m, h, y, neg, "softmax", log_q, 1.0, False, "mean")


def _kind_cfg(kind, L, dropout=0.0):
    I = 300
    if kind == "SASRec":
        return O.Cfg(kind, I, L, 50, dropout=dropout)
    if kind in ("SRFR", "SRFRN"):
        return O.Cfg(kind, I, L, 45, d_fake=5, dropout=dropout)
    return O.Cfg(kind, I, L, 50, n_labels=3, dropout=dropout)


@pytest.mark.parametrize("L", [20, 50])
@pytest.mark.parametrize("objective", ["softmax", "gbce"])
def test_through_encoder_train_dropout_matches_torch_materialised(objective, L):
    """Whole-model gradients of the fused loss against the same model (same weights, same dropout masks) with torch's
    materialised fp32 loss on its own hidden states; L = 50 runs the ragged encoder plan."""
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr, random_sd
    cfg = _kind_cfg("SASRec", L, dropout=0.5)
    sd = random_sd(cfg, 5)
    batch = srfrd_amd.synthetic_batch(cfg.item_number, L, 16, seed=13, device="cpu", min_len=1)[1:]
    seq, rsq, pos = cuda(*batch[:3])
    neg, log_q = srfrd_amd.sample_token_negatives(cfg.item_number, pos, 40, generator=torch.Generator("cuda").manual_seed(9))
    log_q = log_q + torch.randn(log_q.shape, device="cuda") * (pos != 0).unsqueeze(-1)
    lq = log_q if objective == "softmax" else None
    seed = 0xC0FFEE
    grads = []
    for fused in (True, False):
        model = build_model(cfg, sd).train()
        model._next_seed = lambda: seed
        hidden, _, _ = model(None, seq, rsq)
        if fused:
            loss = model.token_negatives_loss(hidden, pos, neg, objective, lq, 0.4)
        else:
            loss = _torch_loss(hidden, dict(model.named_parameters())[O.key_item(cfg)], pos, neg, lq, objective, 0.4)
        loss.backward()
        grads.append((float(loss.detach()), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    (lf, gf), (lt, gt) = grads
    assert abs(lf - lt) <= 1e-5 * max(1.0, abs(lt))
    assert set(gf) == set(gt)
    for k in gt:
        assert maxerr(gf[k], gt[k]) < TOL, (k, maxerr(gf[k], gt[k]))


@pytest.mark.parametrize("L", [20, 50])
@pytest.mark.parametrize("objective", ["softmax", "gbce"])
def test_gradients_and_one_adam_step_against_oracle(objective, L):
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr, random_sd
    cfg = _kind_cfg("SASRec", L)
    sd = random_sd(cfg, 7)
    batch = srfrd_amd.synthetic_batch(cfg.item_number, cfg.max_len, 8, seed=11, device="cpu", min_len=1)[1:]
    neg, log_q = srfrd_amd.sample_token_negatives(cfg.item_number, batch[2], 24, counts=torch.arange(cfg.item_number + 1.0),
                                                  alpha=0.75, generator=torch.Generator().manual_seed(3))
    lq = log_q if objective == "softmax" else None
    beta = srfrd_amd.gbce_beta(cfg.item_number, 24, 0.75)
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    h, _, _ = O.forward(cfg, leaves, batch[0], batch[1])
    loss_o = _torch_loss(h, O.item_table(cfg, leaves), batch[2], neg, None if lq is None else lq.double(), objective, beta)
    loss_o.backward()
    grads_o = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).clone() for k, v in leaves.items()}
    grads_o[O.key_item(cfg)][0].zero_()
    sd64 = {k: v.detach().clone() for k, v in leaves.items()}
    for opt_kind in ("srfrd", "torch"):
        model = build_model(cfg, sd).train()
        seq, rsq, pos = cuda(*batch[:3])
        params = list(model.parameters())
        opt = srfrd_amd.Adam(params, lr=1e-3, betas=(0.9, 0.98)) if opt_kind == "srfrd" else \
            torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.98))
        hidden, _, _ = model(None, seq, rsq)
        loss = model.token_negatives_loss(hidden, pos, neg.cuda(), objective, None if lq is None else lq.cuda(), beta)
        loss.backward()
        assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
        for k, p in model.named_parameters():
            assert maxerr(p.grad, grads_o[k]) < TOL, (k, maxerr(p.grad, grads_o[k]))
        opt.step()
        sd_step = {k: v.clone() for k, v in sd64.items()}
        O.Adam(sd_step, lr=1e-3, betas=(0.9, 0.98)).step(sd_step, grads_o)
        assert_post_adam(model.state_dict(), sd_step, [{k: g.float() for k, g in grads_o.items()}], cfg.D)


@pytest.mark.parametrize("objective", ["softmax", "gbce"])
def test_c2_size_against_materialised_fp64(objective):
    import srfrd_amd
    torch.manual_seed(1)
    B, L, n, K = 512, 50, 50_000, 256
    m = _model("SASRec", n, L)
    with torch.no_grad():
        _table(m).normal_(0, 0.3)
    _, seq, _, pos, *_ = srfrd_amd.synthetic_batch(n, L, B, seed=21, device="cuda")
    h = torch.randn(B, L, 50, device="cuda") * 0.3
    neg, log_q = srfrd_amd.sample_token_negatives(n, pos, K, generator=torch.Generator(device="cuda").manual_seed(5))
    lq = log_q if objective == "softmax" else None
    beta = srfrd_amd.gbce_beta(n, K, 0.75)
    loss, dh, de = _run(m, h, pos, neg, objective, lq, beta, True, "mean")
    rl, rdh, rde = _ref(h, _table(m), pos, neg, lq, True, "mean", objective, beta, chunk=1024)
    print(objective, "loss", float(loss), float(rl), "dh", _rel(dh, rdh), "de", _rel(de, rde))
    assert abs(float(loss) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl)))
    assert _rel(dh, rdh) <= 1e-4 and _rel(de, rde) <= 1e-4


@pytest.mark.parametrize("objective", ["softmax", "gbce"])
def test_c5_shape_against_materialised_fp64(objective):
    import srfrd_amd
    torch.manual_seed(2)
    B, L, n, K = 64, 200, 1_000_000, 128
    m = _model("SASRec", n, L)
    with torch.no_grad():
        _table(m).normal_(0, 0.3)
    y, _ = make_inputs(B, L, 1, n, 9, empty_rows=(5,))
    y = y.cuda()
    h = torch.randn(B, L, 50, device="cuda") * 0.3
    counts = torch.rand(n + 1, generator=torch.Generator().manual_seed(6)) ** 4
    neg, log_q = srfrd_amd.sample_token_negatives(n, y, K, counts=counts.cuda(), generator=torch.Generator(device="cuda").manual_seed(7))
    lq = log_q if objective == "softmax" else None
    loss, dh, de = _run(m, h, y, neg, objective, lq, 0.5, True, "mean")
    rl, rdh, rde = _ref(h, _table(m), y, neg, lq, True, "mean", objective, 0.5, chunk=1024)
    print(objective, "loss", float(loss), float(rl), "dh", _rel(dh, rdh), "de", _rel(de, rde))
    assert abs(float(loss) - float(rl)) <= 1e-5 * max(1.0, abs(float(rl)))
    assert _rel(dh, rdh) <= 1e-4 and _rel(de, rde) <= 1e-4


def test_refusals():
    m = _model("SASRec", 100)
    h = torch.randn(2, 20, 50, device="cuda")
    y = torch.ones(2, 20, dtype=torch.int64, device="cuda")
    neg = torch.randint(1, 101, (2, 20, 3), device="cuda")
    m.validate_ids = "eager"
    bad = neg.clone()
    bad[1, 4, 2] = 101
    with pytest.raises(IndexError):
        m.token_negatives_loss(h, y, bad)
    bad[1, 4, 2] = -1
    with pytest.raises(IndexError):
        m.token_negatives_loss(h, y, bad)
    bad[1, 4, 2] = 0
    bad[0, 0, 0] = 100
    m.token_negatives_loss(h, y, bad)                         # 0 (unused slot) and n_items are in range
    for kw in (dict(hidden_state=h.double()), dict(hidden_state=h[:, :, :40]), dict(positive_ids=y[:, :10]),
               dict(negative_ids=neg[0]), dict(negative_ids=neg[:, :10]), dict(negative_ids=neg.view(2, 20 * 3)),
               dict(negative_ids=neg.float()), dict(negative_ids=neg[:, :, :0]), dict(objective="bce"),
               dict(log_q=torch.zeros(2, 20, 3, dtype=torch.float64, device="cuda")),
               dict(log_q=torch.zeros(2, 20, 4, device="cuda")), dict(log_q=torch.zeros(3, device="cuda")),
               dict(objective="gbce", log_q=torch.zeros(2, 20, 3, device="cuda")), dict(objective="gbce", beta=-0.1),
               dict(objective="gbce", beta=float("inf")), dict(objective="gbce", beta=float("nan")), dict(reduction="avg")):
        args = dict(hidden_state=h, positive_ids=y, negative_ids=neg)
        args.update(kw)
        with pytest.raises(ValueError):
            m.token_negatives_loss(**args)
    m.use_bf16_table(True)
    with pytest.raises(RuntimeError, match="fp32 item table"):
        m.token_negatives_loss(h, y, neg)
