"""-m gpu: FusedTrainer(loss="sampled_softmax" | "softmax") and the device-side shared-negative sampler.

The sampler (srfrd_shared_negatives) is restated in numpy, integer for integer (tests/loss_refs.py, ref_negatives): its ids
must agree bit for bit, its log-Q output with log(K q) in fp64.  The trainer's step is held against the module-level loop on
the same negatives and dropout masks (model(...) -> model.sampled_softmax_loss -> backward -> srfrd_amd.Adam), against the fp64
oracle with a materialised softmax, and against itself: graph replay = eager, and a resumed run = the uninterrupted one, bit
for bit."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.helpers import assert_post_adam
from tests.loss_refs import M32, ref_negatives, sxent_mean_loss, xent_mean_loss
from tests.test_gpu_sxent import KINDS, _kind_cfg

pytestmark = pytest.mark.gpu


def _state(seed_word, dev="cuda"):
    st = torch.zeros(32, dtype=torch.int32)
    st[2] = int(np.array([seed_word], dtype=np.uint32).view(np.int32)[0])
    return st.to(dev)


def _draw(state, n_items, K, tab=None):
    from srfrd_amd import _lib
    from srfrd_amd._lib import check, ptr
    ids = torch.empty(K, device="cuda", dtype=torch.int64)
    lq = torch.empty(K, device="cuda", dtype=torch.float32)
    prob, idx, ilq = tab if tab is not None else (None, None, None)
    check(_lib.lib().srfrd_shared_negatives(ptr(state), n_items, K, ptr(prob), ptr(idx), ptr(ilq), ptr(ids), ptr(lq),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "srfrd_shared_negatives")
    return ids, lq


def _table(n_items, K, seed=0, zeros=False):
    """a skewed popularity distribution -> (q fp64, device (alias_prob, alias_idx, item_log_q), host (prob, alias))"""
    from srfrd_amd.sampler import alias_table, negative_q
    rs = np.random.RandomState(seed + n_items)
    counts = np.r_[0.0, rs.pareto(1.0, n_items) + 0.01]
    if zeros and n_items > 2:
        counts[1 + rs.choice(n_items, n_items // 2, replace=False)] = 0.0
    q = negative_q(n_items, torch.from_numpy(counts), 0.8)
    prob, alias = alias_table(q)
    with np.errstate(divide="ignore"):
        ilq = np.r_[0.0, np.log(K * q)].astype(np.float32)
    dev = (torch.from_numpy(prob).cuda(), torch.from_numpy(alias).cuda(), torch.from_numpy(ilq).cuda())
    return q, dev, (prob, alias)


SEEDS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xDEADBEEF, M32)


@pytest.mark.parametrize("n_items", [1, 2, 300, 50_000])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 4096])
def test_sampler_matches_numpy_restatement(n_items, K):
    tab_q, tab_dev, (prob, alias) = _table(n_items, K, zeros=True)
    for seed in SEEDS:
        st = _state(seed)
        ids, lq = _draw(st, n_items, K)
        ref = ref_negatives(seed, n_items, K)
        assert np.array_equal(ids.cpu().numpy(), ref), (seed, n_items, K)
        assert bool((lq == np.float32(math.log(K / n_items))).all())
        ids, lq = _draw(st, n_items, K, tab_dev)
        ref = ref_negatives(seed, n_items, K, prob, alias)
        assert np.array_equal(ids.cpu().numpy(), ref), (seed, n_items, K, "alias")
        assert ids.min() >= 1 and ids.max() <= n_items
        want = np.log(K * tab_q[ref - 1])                            # fp64
        assert np.all(np.isfinite(want))                             # (no zero-weight item is ever drawn)
        assert np.abs(lq.cpu().numpy().astype(np.float64) - want).max() <= 1e-6 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("popularity", [False, True])
def test_sampler_distribution_chi_square(popularity):
    """2000 consecutive seed words x K = 1024 draws over 300 items against q: a fixed chi-square bound (the seeds are fixed,
    so the statistic is one number, not a random one).  299 degrees of freedom: mean 299, sd 24.5; bound 299 + 6 sd."""
    n, K, steps = 300, 1024, 2000
    if popularity:
        q, tab, _ = _table(n, K)
    else:
        q, tab = np.full(n, 1.0 / n), None
    out = torch.empty(steps, K, device="cuda", dtype=torch.int64)
    st = _state(12345)
    for s in range(steps):
        st[2].fill_(12345 + s)
        out[s] = _draw(st, n, K, tab)[0]
    counts = torch.bincount(out.view(-1) - 1, minlength=n).cpu().numpy().astype(np.float64)
    expect = q * steps * K
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    assert chi2 < 299 + 6 * math.sqrt(2 * 299), chi2
    # and the draws of consecutive steps are not the same negatives
    assert not torch.equal(out[0], out[1])


# ------------------------------------------------------------------------------------------------ the train step
def _batch(cfg, B, seed, min_len=1):
    import srfrd_amd
    return srfrd_amd.synthetic_batch(cfg.item_number, cfg.max_len, B, seed=seed, device="cuda", min_len=min_len)[1:]


def _seed_word(tr):
    return int(tr.state[2].item()) & M32


@pytest.mark.parametrize("dropout", [0.0, 0.5])
@pytest.mark.parametrize("L", [20, 50])
@pytest.mark.parametrize("kind", KINDS)
def test_sampled_step_matches_module_path(kind, L, dropout):
    """two FusedTrainer(loss="sampled_softmax") steps (graph) against the module-level loop on the negatives the trainer
    drew and the dropout masks of its seed words; L = 50 runs the ragged encoder pair"""
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _kind_cfg(kind, L, dropout)
    sd = random_sd(cfg, 21)
    B, K = 16, 256
    fused = build_model(cfg, sd).train()
    tr = srfrd_amd.FusedTrainer(fused, B, L, loss="sampled_softmax", num_negatives=K)
    ref = build_model(cfg, sd).train()
    opt = srfrd_amd.Adam(list(ref.parameters()), lr=1e-3, betas=(0.9, 0.98))
    hists = []
    for step in range(2):
        batch = _batch(cfg, B, 40 + step)
        seed = _seed_word(tr)
        loss_f = float(tr.step(None, *batch))
        neg, log_q = tr.negatives, tr.log_q
        assert neg.min() >= 1 and neg.max() <= cfg.item_number
        ref._next_seed = lambda s=seed: s
        opt.zero_grad()
        hidden, _, _ = ref(None, batch[0], batch[1])
        loss_r = ref.sampled_softmax_loss(hidden, batch[2], neg, log_q)
        loss_r.backward()
        params = dict(ref.named_parameters())
        hists.append({k: (params[k].grad if params[k].grad is not None else torch.zeros_like(params[k])).detach().cpu().clone()
                      for k in ref.state_dict()})
        opt.step()
        lr_ = float(loss_r.detach())
        assert abs(loss_f - lr_) <= 1e-5 * max(1.0, abs(lr_)), (step, loss_f, lr_)
    want = {k: v.detach().cpu() for k, v in ref.state_dict().items()}
    assert_post_adam(fused.state_dict(), want, hists, cfg.D)


def _oracle_step(cfg, sd, batch, loss, neg=None, log_q=None, l2=0.0):
    """fp64: O.forward + materialised softmax CE (mean over targets) [+ l2 * sum ||p||] -> (loss, grads, stepped sd)"""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    seq, rsq, pos = (t.cpu() for t in batch[:3])
    h, _, _ = O.forward(cfg, leaves, seq, rsq)
    E = O.item_table(cfg, leaves)
    ce = sxent_mean_loss(h, E, pos, neg, log_q, True) if loss == "sampled_softmax" else xent_mean_loss(h, E, pos)
    ce.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).clone() for k, v in leaves.items()}
    grads[O.key_item(cfg)][0].zero_()                           # padding_idx rows, as O.grads_of
    if cfg.kind in ("SRFR", "SRFRN"):
        grads[O.key_side(cfg)][0].zero_()
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


@pytest.mark.parametrize("loss, kind, l2", [("softmax", "SASRec", 0.0), ("softmax", "SRFRN", 0.0),
                                            ("sampled_softmax", "SASRec", 0.0), ("sampled_softmax", "SRFU_B", 0.0),
                                            ("sampled_softmax", "SRFR", 1e-3), ("softmax", "SASRec", 1e-3)])
def test_one_step_against_fp64_oracle(loss, kind, l2):
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _kind_cfg(kind, 20)
    sd = random_sd(cfg, 8)
    B = 8
    model = build_model(cfg, sd).train()
    counts = torch.arange(cfg.item_number + 1.0) ** 0.5
    kw = dict(num_negatives=512, neg_counts=counts, neg_alpha=0.75) if loss == "sampled_softmax" else {}
    tr = srfrd_amd.FusedTrainer(model, B, 20, loss=loss, l2_emb=l2, **kw)
    batch = _batch(cfg, B, 5)
    got = float(tr.step(None, *batch))
    neg, log_q = (tr.negatives.cpu(), tr.log_q.cpu().double()) if loss == "sampled_softmax" else (None, None)
    want, grads, sd_step = _oracle_step(cfg, sd, batch, loss, neg, log_q, l2)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    assert_post_adam(model.state_dict(), sd_step, [{k: g.float() for k, g in grads.items()}], cfg.D)


def _flat_bits(tr):
    torch.cuda.synchronize()
    return tr.flat.detach().clone()


@pytest.mark.parametrize("loss, det", [("sampled_softmax", False), ("softmax", True)])
def test_graph_equals_eager_and_resume_is_bitwise(loss, det):
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _kind_cfg("SRFRN", 50, dropout=0.5)
    sd = random_sd(cfg, 3)
    B, K = 32, 300
    batches = [_batch(cfg, B, 70 + i) for i in range(4)]

    def trainer(use_graph, model_sd=sd):
        m = build_model(cfg, model_sd).train()
        return srfrd_amd.FusedTrainer(m, B, 50, loss=loss, num_negatives=K, deterministic=det, use_graph=use_graph,
                                      neg_counts=torch.arange(cfg.item_number + 1.0) if loss == "sampled_softmax" else None)

    g, e, g2 = trainer(True), trainer(False), trainer(True)
    for i in range(3):
        lg, le, lg2 = (float(t.step(None, *batches[i])) for t in (g, e, g2))
        assert math.isfinite(lg) and lg == le == lg2, (i, lg, le, lg2)
        if loss == "sampled_softmax":
            assert torch.equal(g.negatives, e.negatives) and torch.equal(g.log_q, e.log_q)
            assert torch.equal(g.negatives, g2.negatives)
        assert torch.equal(_flat_bits(g), _flat_bits(e)), i
        assert torch.equal(_flat_bits(g), _flat_bits(g2)), i

    # four uninterrupted steps = two, state_dict, a fresh trainer, load_state_dict, two more
    a = trainer(True)
    drawn_a = []
    for i in range(4):
        a.step(None, *batches[i])
        drawn_a.append(a.negatives)
    b = trainer(True)
    for i in range(2):
        b.step(None, *batches[i])
    opt_sd, model_sd = b.state_dict(), {k: v.detach().cpu().clone() for k, v in b.model.state_dict().items()}
    c = trainer(True, model_sd)
    c.load_state_dict(opt_sd)
    for i in range(2, 4):
        lc = float(c.step(None, *batches[i]))
        if loss == "sampled_softmax":
            assert torch.equal(c.negatives, drawn_a[i]), i
    assert lc == float(a.loss)
    assert torch.equal(_flat_bits(c), _flat_bits(a))
    ma, va = a._moments_full()
    mc, vc = c._moments_full()
    assert torch.equal(ma, mc) and torch.equal(va, vc)
    # a resume under another loss configuration is refused
    other = srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), B, 50, loss="bce" if loss != "bce" else "softmax")
    with pytest.raises(ValueError, match="loss"):
        other.load_state_dict(opt_sd)


@pytest.mark.parametrize("loss, kw", [("sampled_softmax", dict(num_negatives=64)), ("softmax", dict(deterministic=True))])
def test_spin_up_leaves_the_training_trajectory_untouched(loss, kw):
    """FusedTrainer.spin_up() under the catalog losses: 7 replays of a filled slot inside the snapshot, then three steps -
    losses, parameters, both moments and (sampled: the state word the device sampler draws from is restored) the negatives
    of every step bit for bit those of a run without it.  400 items, L 50 (the ragged pair), B 16, dropout 0.5."""
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = O.Cfg("SRFRN", 400, 50, 45, d_fake=5, dropout=0.5)
    sd = random_sd(cfg, 21)
    B = 16
    batches = [_batch(cfg, B, 80 + i) for i in range(3)]
    outs = []
    for spin in (False, True):
        tr = srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), B, 50, loss=loss, seed=77, **kw)
        if spin:
            tr.ids_ring[0].copy_(torch.stack(batches[2]))
            tr.spin_up(7)
            assert tr.captured and tr.graph_form == "one" and tr.steps_done == 0
        losses, drawn = [], []
        for b in batches:
            losses.append(float(tr.step(None, *b)))
            drawn.append(tr.negatives)
        assert all(math.isfinite(x) for x in losses)
        torch.cuda.synchronize()
        outs.append((losses, drawn, (tr.flat.detach().clone(), tr.m.detach().clone(), tr.v.detach().clone())))
    assert outs[0][0] == outs[1][0]
    assert all(torch.equal(x, y) for x, y in zip(outs[0][2], outs[1][2]))
    if loss == "sampled_softmax":
        assert all(torch.equal(x, y) for x, y in zip(outs[0][1], outs[1][1]))
        assert not torch.equal(outs[0][1][0], outs[0][1][1])           # (every step draws its own)


@pytest.mark.parametrize("loss", ["sampled_softmax", "softmax"])
def test_batch_without_targets_behaves_as_bce(loss):
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _kind_cfg("SASRec", 20)
    sd = random_sd(cfg, 4)
    B = 8
    batch = list(_batch(cfg, B, 9))
    batch[2] = torch.zeros_like(batch[2])                          # no position has a target
    out = []
    for kind in ("bce", loss):
        m = build_model(cfg, sd).train()
        tr = srfrd_amd.FusedTrainer(m, B, 20, loss=kind, num_negatives=64)
        lo = tr.step(None, *batch)
        torch.cuda.synchronize()
        out.append((lo.clone(), tr.flat.clone(), tr.m.clone(), tr.v.clone()))
    (lb, fb, mb, vb), (lc, fc, mc, vc) = out
    assert bool(torch.isnan(lb).all()) == bool(torch.isnan(lc).all())
    for x, y in ((fb, fc), (mb, mc), (vb, vc)):
        torch.testing.assert_close(x, y, rtol=0.0, atol=0.0, equal_nan=True)


def test_step_accepts_no_negative_ids():
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _kind_cfg("SRFRN", 20)
    sd = random_sd(cfg, 6)
    batch = _batch(cfg, 8, 2)
    losses = []
    for negs in ("given", "none", "zeros"):
        tr = srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), 8, 20, loss="sampled_softmax", num_negatives=128)
        b = list(batch)
        if negs == "none":
            b[4] = b[5] = None
        elif negs == "zeros":
            b[4], b[5] = torch.zeros_like(b[4]), torch.zeros_like(b[5])
        losses.append(float(tr.step(None, *b)))
        tr.check()                                                  # an all-zero negative plane is a valid batch
    assert losses[0] == losses[1] == losses[2]


def test_c2_size_graph_step():
    """C2: 50 k items, B 512, L 50, K 1024, graph mode: step 1 = eager, a finite loss, and 20 steps on one batch lower it"""
    import srfrd_amd
    B, L, n, K = 512, 50, 50_000, 1024
    torch.manual_seed(0)
    m0 = srfrd_amd.SASRec(n, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m0.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
    batch = srfrd_amd.synthetic_batch(n, L, B, seed=1, device="cuda")[1:]
    trs = []
    for use_graph in (True, False):
        m = srfrd_amd.SASRec(n, L, 50, 0.0, 2, 1, "cuda")
        m.load_state_dict(sd)
        trs.append(srfrd_amd.FusedTrainer(m.to("cuda").train(), B, L, loss="sampled_softmax", num_negatives=K,
                                          use_graph=use_graph))
    g, e = trs
    l1 = float(g.step(None, *batch))
    assert l1 == float(e.step(None, *batch)) and math.isfinite(l1)
    assert torch.equal(_flat_bits(g), _flat_bits(e))
    losses = [l1] + [float(g.step(None, *batch)) for _ in range(19)]
    assert all(math.isfinite(x) for x in losses)
    assert np.mean(losses[-3:]) < losses[0] - 0.1, losses
