"""FusedTrainer(loss="token_softmax" | "gbce") on the GPU: the step with K negatives per position against
the module-level loop, an fp64 oracle and the BCE step; graph = eager and resume, bit for bit; the negative ring fed by
DeviceSampler.  The trainer shapes built here are tests/token_trainer_refs.TRAINER_SHAPES, whose key lists
tests/test_token_trainer_abi.py audits on the CPU."""
import math

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests import token_trainer_refs as R
from tests.helpers import assert_post_adam
from tests.loss_refs import tneg_mean_loss as _torch_loss
from tests.test_gpu_sxent import KINDS, _kind_cfg

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF
OBJECTIVE = {"token_softmax": "softmax", "gbce": "gbce"}


def _batch(cfg, B, seed, min_len=1):
    import srfrd_amd
    return srfrd_amd.synthetic_batch(cfg.item_number, cfg.max_len, B, seed=seed, device="cuda", min_len=min_len)[1:]


def _negatives(cfg, pos, K, seed):
    import srfrd_amd
    neg, log_q = srfrd_amd.sample_token_negatives(cfg.item_number, pos, K, generator=torch.Generator("cuda").manual_seed(seed))
    log_q = log_q + torch.randn(log_q.shape, device="cuda") * (pos != 0).unsqueeze(-1)      # (a log-Q that matters)
    return neg, log_q.contiguous()


def _seed_word(tr):
    return int(tr.state[2].item()) & M32


def _trainer(cfg, sd, B, loss, K, **kw):
    import srfrd_amd
    from tests.gpu_util import build_model
    assert (B, cfg.max_len, K, cfg.item_number) in R.TRAINER_SHAPES
    return srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), B, cfg.max_len, loss=loss, num_negatives=K, **kw)


def _step(tr, batch, neg, log_q=None):
    return tr.step(None, batch[0], batch[1], batch[2], batch[3], neg, batch[5], log_q=log_q)


def _module_steps(cfg, sd, tr, batches, negs, loss, beta, remove, lr_tol=1e-5):
    """every (batch, negatives, log_q) through the trainer and through model(...) -> token_negatives_loss -> srfrd_amd.Adam on
    the trainer's dropout seed words; the project's bars: loss within 1e-5 max(1, |loss|), parameters by assert_post_adam"""
    import srfrd_amd
    from tests.gpu_util import build_model
    ref = build_model(cfg, sd).train()
    opt = srfrd_amd.Adam(list(ref.parameters()), lr=1e-3, betas=(0.9, 0.98))
    hists = []
    for step, (batch, (neg, log_q)) in enumerate(zip(batches, negs)):
        seed = _seed_word(tr)
        loss_f = float(_step(tr, batch, neg, log_q))
        assert torch.equal(tr.negatives, neg)
        ref._next_seed = lambda s=seed: s
        opt.zero_grad()
        hidden, _, _ = ref(None, batch[0], batch[1])
        lq = log_q if loss == "token_softmax" else None
        loss_r = ref.token_negatives_loss(hidden, batch[2], neg, OBJECTIVE[loss], lq, beta, remove)
        loss_r.backward()
        params = dict(ref.named_parameters())
        hists.append({k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])).detach().cpu().clone()
                      for k in ref.state_dict()})
        opt.step()
        lr_ = float(loss_r.detach())
        print(f"step {step}: fused {loss_f:.7f} module {lr_:.7f}")
        assert abs(loss_f - lr_) <= lr_tol * max(1.0, abs(lr_)), (step, loss_f, lr_)
    tr.check()
    want = {k: v.detach().cpu() for k, v in ref.state_dict().items()}
    assert_post_adam(tr.model.state_dict(), want, hists, cfg.D)


_MODULE_CASES = [(kind, L, dropout, loss) for kind in KINDS for L in (20, 50) for dropout in (0.0, 0.5)
                 for loss in ("token_softmax", "gbce") if not (loss == "gbce" and kind == "SRFRN")]


@pytest.mark.parametrize("i", range(len(_MODULE_CASES)), ids=lambda i: "-".join(str(x) for x in _MODULE_CASES[i]))
def test_step_matches_module_path(i):
    """two graph steps against the module path on the same negatives and dropout seed words; K in {1, 5, 65}, log_q given
    or not and hit removal on or off cycle through the cases (every value of each with both objectives)"""
    from tests.gpu_util import random_sd
    kind, L, dropout, loss = _MODULE_CASES[i]
    K, with_lq, remove = (1, 5, 65)[i % 3], bool((i // 2) % 2), bool((i // 4 + i) % 2)
    cfg = _kind_cfg(kind, L, dropout)
    sd = random_sd(cfg, 21)
    B = 16
    beta = 0.6 if loss == "gbce" else 1.0
    tr = _trainer(cfg, sd, B, loss, K, gbce_beta=beta, remove_accidental_hits=remove)
    batches = [_batch(cfg, B, 40 + s) for s in range(2)]
    negs = [_negatives(cfg, b[2], K, 9 + s) for s, b in enumerate(batches)]
    if not with_lq:
        negs = [(n, None) for n, _ in negs]
    _module_steps(cfg, sd, tr, batches, negs, loss, beta, remove)


def test_the_module_cases_cover_every_k_log_q_and_hit_removal():
    seen = {(loss, "K", (1, 5, 65)[i % 3]) for i, (_, _, _, loss) in enumerate(_MODULE_CASES)}
    seen |= {(loss, "lq", bool((i // 2) % 2)) for i, (_, _, _, loss) in enumerate(_MODULE_CASES)}
    seen |= {(loss, "rm", bool((i // 4 + i) % 2)) for i, (_, _, _, loss) in enumerate(_MODULE_CASES)}
    for loss in ("token_softmax", "gbce"):
        assert {(loss, "K", k) for k in (1, 5, 65)} | {(loss, w, v) for w in ("lq", "rm") for v in (False, True)} <= seen


def _oracle_step(cfg, sd, batch, neg, log_q, objective, beta, l2=0.0):
    """fp64: O.forward + the materialised loss (mean over targets) [+ l2 * sum ||p||] -> (loss, grads, stepped sd)"""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    seq, rsq, pos = (t.cpu() for t in batch[:3])
    h, _, _ = O.forward(cfg, leaves, seq, rsq)
    ce = _torch_loss(h, O.item_table(cfg, leaves), pos, neg.cpu(), None if log_q is None else log_q.cpu().double(), objective, beta)
    ce.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).clone() for k, v in leaves.items()}
    grads[O.key_item(cfg)][0].zero_()                           # padding_idx rows, as O.grads_of
    total = float(ce)
    if l2:                                                      # as O.grads_of: l2's term reaches the padding rows too
        for k, v in leaves.items():
            nrm = torch.norm(v.detach())
            total += l2 * float(nrm)
            if float(nrm) > 0.0:
                grads[k] = grads[k] + l2 * v.detach() / nrm
    sd_step = {k: v.detach().clone() for k, v in leaves.items()}
    O.Adam(sd_step, lr=1e-3, betas=(0.9, 0.98)).step(sd_step, grads)
    return total, grads, sd_step


@pytest.mark.parametrize("loss, kind, l2", [("token_softmax", "SASRec", 0.0), ("gbce", "SASRec", 0.0), ("token_softmax", "SRFU_B", 0.0),
                                            ("gbce", "SRFU_B", 0.0), ("token_softmax", "SASRec", 1e-3)])
def test_one_step_against_fp64_oracle(loss, kind, l2):
    import srfrd_amd
    from tests.gpu_util import random_sd
    cfg = _kind_cfg(kind, 20)
    sd = random_sd(cfg, 8)
    B, K = 8, 24
    beta = srfrd_amd.gbce_beta(cfg.item_number, K, 0.75) if loss == "gbce" else 1.0
    tr = _trainer(cfg, sd, B, loss, K, gbce_beta=beta, l2_emb=l2)
    batch = _batch(cfg, B, 5)
    neg, log_q = _negatives(cfg, batch[2], K, 3)
    got = float(_step(tr, batch, neg, log_q))
    want, grads, sd_step = _oracle_step(cfg, sd, batch, neg, log_q if loss == "token_softmax" else None, OBJECTIVE[loss], beta, l2)
    print(f"fused {got:.7f} oracle {want:.7f}")
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    assert_post_adam(tr.model.state_dict(), sd_step, [{k: g.float() for k, g in grads.items()}], cfg.D)


def _grads_of_moment(tr, m_before):
    """the mean gradient the last step handed to Adam, from its first moment: m = 0.9 m_before + 0.1 g"""
    g = ((tr.m - 0.9 * m_before) / 0.1).detach().cpu()
    names = {id(p): k for k, p in tr.model.named_parameters()}
    return {names[id(p)]: g[o:o + p.numel()].view(p.shape).clone() for p, o in tr.model._slots}


@pytest.mark.parametrize("kind", ["SASRec", "SRFU_B"])
def test_gbce_k1_beta1_is_the_bce_step(kind):
    """loss="gbce", K = 1, beta = 1, no hit removal, on the batch's own negative plane: two steps beside FusedTrainer(
    loss="bce") on the same batches - the step the reference-generated fixtures pin"""
    from tests.gpu_util import random_sd
    cfg = _kind_cfg(kind, 20, 0.5)
    sd = random_sd(cfg, 12)
    B = 8
    tok = _trainer(cfg, sd, B, "gbce", 1, gbce_beta=1.0, remove_accidental_hits=False)
    bce = _trainer(cfg, sd, B, "bce", 1)
    hists = []
    for s in range(2):
        batch = _batch(cfg, B, 60 + s)
        assert bool((batch[4][batch[2] != 0] != 0).all())           # every target has its negative: no unused slot
        m0 = bce.m.clone()
        lt = float(_step(tok, batch, batch[4].unsqueeze(-1).contiguous()))
        lb = float(bce.step(None, *batch))
        hists.append(_grads_of_moment(bce, m0))
        print(f"step {s}: gbce {lt:.7f} bce {lb:.7f}")
        assert abs(lt - lb) <= 1e-5 * max(1.0, abs(lb)), (s, lt, lb)
    want = {k: v.detach().cpu() for k, v in bce.model.state_dict().items()}
    assert_post_adam(tok.model.state_dict(), want, hists, cfg.D)


def _bits(tr):
    torch.cuda.synchronize()
    return tr.flat.detach().clone(), tr.m.detach().clone(), tr.v.detach().clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_graph_equals_eager_resume_and_foreign_states(loss):
    import srfrd_amd
    from tests.gpu_util import random_sd
    cfg = _kind_cfg("SRFU_B", 50, dropout=0.5)
    sd = random_sd(cfg, 3)
    B, K = 16, 5
    batches = [_batch(cfg, B, 70 + i) for i in range(4)]
    negs = [_negatives(cfg, b[2], K, 30 + i) for i, b in enumerate(batches)]

    def trainer(use_graph=True, model_sd=sd, **kw):
        kw = dict(dict(gbce_beta=0.7), **kw)
        return _trainer(cfg, model_sd, B, loss, K, use_graph=use_graph, **kw)

    # graph = eager, and two independent runs agree, with `deterministic` either way: flat parameters and both moments
    g, e, g2, gd = trainer(True), trainer(False), trainer(True, deterministic=True), trainer(True, deterministic=True)
    for i in range(3):
        ls = [float(_step(t, batches[i], *negs[i])) for t in (g, e, g2, gd)]
        assert math.isfinite(ls[0]) and ls[0] == ls[1] == ls[2] == ls[3], (i, ls)
        for other in (e, g2, gd):
            assert _same(_bits(g), _bits(other)), i
    # four uninterrupted steps = two, state_dict, a fresh trainer, load_state_dict, two more
    _step(g, batches[3], *negs[3])
    b = trainer(True)
    for i in range(2):
        _step(b, batches[i], *negs[i])
    opt_sd, model_sd = b.state_dict(), {k: v.detach().cpu().clone() for k, v in b.model.state_dict().items()}
    assert opt_sd["srfrd"]["loss"] == {"kind": loss, "num_negatives": K, "gbce_beta": 0.7, "logq_correction": True,
                                       "remove_accidental_hits": True}
    c = trainer(True, model_sd)
    c.load_state_dict(opt_sd)
    for i in range(2, 4):
        lc = float(_step(c, batches[i], *negs[i]))
    assert lc == float(g.loss)
    assert _same(_bits(c), _bits(g))
    # a state saved under another loss, another K or another beta is refused
    from tests.gpu_util import build_model
    sampled = srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), B, 50, loss="sampled_softmax", num_negatives=K)
    with pytest.raises(ValueError, match="loss"):
        trainer(True).load_state_dict(sampled.state_dict())
    with pytest.raises(ValueError, match="loss"):
        sampled.load_state_dict(opt_sd)
    with pytest.raises(ValueError, match="loss"):
        trainer(True, gbce_beta=0.2).load_state_dict(opt_sd)
    with pytest.raises(ValueError, match="loss"):
        _trainer(cfg, sd, B, loss, 65).load_state_dict(opt_sd)


@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_spin_up_leaves_the_training_trajectory_untouched(loss):
    """FusedTrainer.spin_up() on the step of two graphs around the eager key sort: 7 replays of a filled slot (ids, negatives
    and log-Q) inside the snapshot, then three steps - losses, parameters and both moments bit for bit those of a run without
    it.  400 items, L 50 (the ragged pair), B 16, K 3, dropout 0.5."""
    from tests.gpu_util import random_sd
    cfg = O.Cfg("SRFU_B", 400, 50, 50, n_labels=3, dropout=0.5)
    sd = random_sd(cfg, 21)
    B, K = 16, 3
    batches = [_batch(cfg, B, 80 + i) for i in range(3)]
    negs = [_negatives(cfg, b[2], K, 50 + i) for i, b in enumerate(batches)]
    outs = []
    for spin in (False, True):
        tr = _trainer(cfg, sd, B, loss, K, gbce_beta=0.7, seed=77)
        if spin:
            tr.ids_ring[0].copy_(torch.stack(batches[2]))
            tr.neg_ring[0].copy_(negs[2][0])
            tr.log_q_ring[0].copy_(negs[2][1])
            tr.spin_up(7)
            assert tr.captured and tr.graph_form == "split" and tr.steps_done == 0
        losses = [float(_step(tr, b, *n)) for b, n in zip(batches, negs)]
        assert all(math.isfinite(x) for x in losses)
        outs.append((losses, _bits(tr)))
    assert outs[0][0] == outs[1][0]
    assert _same(outs[0][1], outs[1][1])


@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_batch_without_targets_behaves_as_bce(loss):
    from tests.gpu_util import random_sd
    cfg = _kind_cfg("SASRec", 20)
    sd = random_sd(cfg, 4)
    B, K = 8, 7
    batch = list(_batch(cfg, B, 9))
    batch[2] = torch.zeros_like(batch[2])                          # no position has a target
    neg = torch.randint(0, cfg.item_number + 1, (B, 20, K), device="cuda")
    out = []
    for kind in ("bce", loss):
        tr = _trainer(cfg, sd, B, kind, K if kind != "bce" else 1)
        lo = _step(tr, batch, neg) if kind != "bce" else tr.step(None, *batch)
        torch.cuda.synchronize()
        out.append((lo.clone(), tr.flat.clone(), tr.m.clone(), tr.v.clone()))
    (lb, fb, mb, vb), (lc, fc, mc, vc) = out
    assert bool(torch.isnan(lb).all()) == bool(torch.isnan(lc).all())
    for x, y in ((fb, fc), (mb, mc), (vb, vc)):
        torch.testing.assert_close(x, y, rtol=0.0, atol=0.0, equal_nan=True)


@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_positions_without_a_participating_slot(loss):
    """every position's K slots are all 0 (even rows) or all accidental hits (odd rows), hit removal on: the module path's
    result; under the softmax the loss is 0 and nothing moves"""
    from tests.gpu_util import random_sd
    cfg = _kind_cfg("SASRec", 20)
    sd = random_sd(cfg, 4)
    B, K = 8, 7
    batch = _batch(cfg, B, 11)
    neg = batch[2].unsqueeze(-1).repeat(1, 1, K)
    neg[0::2] = 0
    neg = neg.contiguous()
    tr = _trainer(cfg, sd, B, loss, K, gbce_beta=0.8)
    before = _bits(tr)[0]
    _module_steps(cfg, sd, tr, [batch], [(neg, None)], loss, 0.8, True)
    if loss == "token_softmax":
        assert float(tr.loss) == 0.0
        assert torch.equal(before, _bits(tr)[0]) and float(tr.m.abs().max()) == 0.0 and float(tr.v.abs().max()) == 0.0
    else:
        assert float(tr.loss) > 0.0 and not torch.equal(before, _bits(tr)[0])


def test_duplicate_heavy_batch():
    """an 8-item catalog, K = 65, B 16, L 20, no hit removal: 21 440 list rows over 8 items, every item's run through ten or
    more segments of the reduction; against the module path"""
    from tests.gpu_util import random_sd
    cfg = O.Cfg("SASRec", 8, 20, 50)
    sd = random_sd(cfg, 2)
    B, K = 16, 65
    batch = _batch(cfg, B, 31, min_len=20)
    neg = torch.randint(1, 9, (B, 20, K), generator=torch.Generator().manual_seed(5)).cuda()
    keys = R.step_keys(batch[0].cpu().numpy(), batch[2].cpu().numpy(), neg.cpu().numpy(), 8, False)
    assert keys.shape[0] == 21_440
    sk = np.sort(keys)
    for item in range(1, 9):
        at = np.nonzero(sk == item)[0]
        assert at[-1] // R.SEG - at[0] // R.SEG + 1 >= 10, (item, at.size)
    R.audit_indices(keys, B * 20, 1 + K, B * 20, 8, 50, R.ws_floats(keys.shape[0], 50))
    for loss in ("token_softmax", "gbce"):
        tr = _trainer(cfg, sd, B, loss, K, remove_accidental_hits=False)
        _module_steps(cfg, sd, tr, [batch], [(neg, None)], loss, 1.0, False)


def _interactions(n_items=300, n_users=40, seed=4):
    import srfrd_amd
    rng = np.random.RandomState(seed)
    u, it = [], []
    for user in range(1, n_users + 1):
        n = int(rng.randint(3, 45))
        u += [user] * n
        it += list(rng.randint(1, n_items + 1, n))
    it[0] = n_items                                             # itemnum is the largest id seen
    return srfrd_amd.partition(np.array(u), np.array(it), rng.rand(len(u)) < 0.3)


def test_ring_fed_by_the_device_sampler():
    """slots = 2: DeviceSampler(num_negatives=5) fills ids_ring / neg_ring / log_q_ring in place and step_slot steps; the bits
    of a second trainer handed the same tensors through step(); an out-of-range negative id makes check() raise"""
    import srfrd_amd
    from tests.gpu_util import random_sd
    cfg = _kind_cfg("SASRec", 20, 0.5)
    sd = random_sd(cfg, 6)
    B, K = 16, 5
    ring = _trainer(cfg, sd, B, "token_softmax", K, slots=2)
    plain = _trainer(cfg, sd, B, "token_softmax", K)
    assert ring.neg_ring.shape == (2, B, 20, K) and ring.neg_ring.dtype == torch.int64
    assert ring.log_q_ring.shape == (2, B, 20, K) and ring.log_q_ring.dtype == torch.float32
    sampler = srfrd_amd.DeviceSampler(_interactions(), B, 20, seed=5, num_negatives=K, model=ring)
    for i in range(4):
        s = i % 2
        sampler.next_batch(packed=True, out=ring.ids_ring[s], neg_out=ring.neg_ring[s], log_q_out=ring.log_q_ring[s])
        assert sampler.negatives.data_ptr() == ring.neg_ring[s].data_ptr()
        ids, neg, lq = ring.ids_ring[s].clone(), ring.neg_ring[s].clone(), ring.log_q_ring[s].clone()
        assert int(neg.max()) >= 1
        lr_ = float(ring.step_slot(s))
        assert torch.equal(ring.negatives, neg) and torch.equal(ring.log_q, lq)
        lp = float(plain.step(None, ids[0], ids[1], ids[2], ids[3], neg, ids[5], log_q=lq))
        assert math.isfinite(lr_) and lr_ == lp, (i, lr_, lp)
        assert _same(_bits(ring), _bits(plain)), i
    plain.check()
    bad = neg.clone()
    bad[3, 7, 2] = cfg.item_number + 1
    plain.step(None, ids[0], ids[1], ids[2], ids[3], bad, ids[5], log_q=lq)
    with pytest.raises(IndexError, match="item id outside"):
        plain.check()
    plain.check()                                               # (the word is cleared by the raise)
    bad[3, 7, 2] = -1
    plain.step(None, ids[0], ids[1], ids[2], ids[3], bad, ids[5])
    with pytest.raises(IndexError, match="item id outside"):
        plain.check()


def test_c2_size_graph_step():
    """C2: 50 k items, B 512, L 50, K = 64, graph mode: a finite loss and the bits of the eager step.  1 689 600 keys: above
    2^20, where torch.sort is the one-sweep radix sort whose memsets must not be captured - the shape at
    which a step with the sort inside its graph faulted"""
    import srfrd_amd
    B, L, n, K = 512, 50, 50_000, 64
    assert (B, L, K, n) in R.TRAINER_SHAPES
    torch.manual_seed(0)
    m0 = srfrd_amd.SASRec(n, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m0.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    batch = srfrd_amd.synthetic_batch(n, L, B, seed=1, device="cuda")[1:]
    neg, log_q = srfrd_amd.sample_token_negatives(n, batch[2], K, generator=torch.Generator("cuda").manual_seed(2))
    trs = []
    for use_graph in (True, False):
        m = srfrd_amd.SASRec(n, L, 50, 0.0, 2, 1, "cuda")
        m.load_state_dict(sd)
        trs.append(srfrd_amd.FusedTrainer(m.to("cuda").train(), B, L, loss="token_softmax", num_negatives=K, use_graph=use_graph))
    g, e = trs
    lg, le = float(_step(g, batch, neg, log_q)), float(_step(e, batch, neg, log_q))
    assert math.isfinite(lg) and lg == le, (lg, le)
    assert _same(_bits(g), _bits(e))
    g.check()
