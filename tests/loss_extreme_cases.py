"""Inputs that put the loss heads' rescaling under load (tests/test_gpu_loss_extreme.py): max |logit| about 200, where exp()
of a logit overflows fp32, with planted tokens whose maximum sits at a chosen candidate.  Every builder returns plain CPU
tensors and a `plan` naming the planted tokens; the check_* functions assert from the fp64 logits that each planted situation
really occurs, so the inputs cannot drift into something milder unnoticed (tests/test_loss_width_cover.py runs the checks
without a GPU).

A token is planted by h_t = c E[j] with c = 200 / |E[j]|^2: its logit against j is 200, against any other row i it is
200 cos(i, j) |E[i]| / |E[j]|, and the planted rows of the table are lengthened by 1.5 so that this stays well below 200."""
import math

import torch

B, L = 5, 13                    # 65 positions: one past the 64-token tile
T = B * L
BIG = 200.0
FAKE_FILL = 1e3                 # the fake slice of `hidden` (d_out > d_item): must never reach a logit
EXTREME_WIDTHS = [(50, 0), (45, 5), (64, 0), (17, 0)]      # (d_item, d_fake): KS 13 / 12 / 16 / 5


def tneg_case_args(d_item, d_fake, objective):
    """(d_item, d_fake, seed) of the tneg case a width runs under an objective: gbce is refused for SRFRN, so there the same
    width runs as plain SASRec"""
    seed = d_item + 7 * d_fake
    if objective == "gbce" and d_fake:
        return d_item + d_fake, 0, seed
    return d_item, d_fake, seed


def _base(d_item, d_fake, n_items, seed, planted_ids):
    g = torch.Generator().manual_seed(seed)
    E = torch.randn(n_items + 1, d_item, generator=g) * 0.5
    E[0] = 0.0
    for j in planted_ids:
        E[j] *= 1.5
    h = torch.randn(T, d_item + d_fake, generator=g)
    y = torch.randint(1, n_items + 1, (T,), generator=g)
    y[torch.rand(T, generator=g) < 0.3] = 0
    y[2 * L:3 * L] = 0                                   # a row of the batch without any target
    return g, E, h, y


def _finish(h, d_item, scale_to, logits_of, planted):
    """scale the unplanted rows so that their largest |logit| is scale_to; fill the fake slice"""
    free = torch.ones(T, dtype=torch.bool)
    free[list(planted)] = False
    big = float(logits_of(h.double())[free].abs().max())
    h[free, :d_item] *= scale_to / big
    if h.shape[1] > d_item:
        h[:, d_item:] = FAKE_FILL * (1.0 + 0.1 * h[:, d_item:])
    return h


def _plant(h, t, E, j, d_item, logit=BIG):
    e = E[j].double()
    h[t, :d_item] = (logit / float(e @ e) * e).float()


def _live(y, skip=()):
    """positions outside the empty row, in order; the planted tokens are taken from here and given targets"""
    return [t for t in range(T) if not (2 * L <= t < 3 * L) and t not in skip]


# ------------------------------------------------------------------------------------------------ full catalog
XENT_ITEMS = 257        # rows 0..257: five 64-row chunks, the last of two rows; 65 tokens are 2 token tiles, so the forward
#                         takes min(chunks, 64) = 5 candidate splits (xent_splits): every chunk is a split of its own


def xent_case(d_item, d_fake=0, seed=0):
    n = XENT_ITEMS
    #        argmax, target
    pairs = [(1, 200), (63, 64), (64, 65), (65, 64), (n, 1), (130, 130)]
    g, E, h, y = _base(d_item, d_fake, n, seed, [a for a, _ in pairs])
    slots = _live(y)[:len(pairs) + 1]
    plan = {"argmax": {}, "zero": slots[-1]}
    for t, (a, tg) in zip(slots, pairs):
        _plant(h, t, E, a, d_item)
        y[t] = tg
        plan["argmax"][t] = a
    h[plan["zero"], :d_item] = 0.0
    y[plan["zero"]] = 5
    h = _finish(h, d_item, 180.0, lambda hh: hh[:, :d_item] @ E.double().T, slots)
    h[plan["zero"], :d_item] = 0.0
    return dict(h=h.view(B, L, -1), E=E, y=y.view(B, L), plan=plan, n_items=n)


def check_xent_case(c):
    E, y, plan = c["E"].double(), c["y"].view(-1), c["plan"]
    d = E.shape[1]
    s = c["h"].view(T, -1).double()[:, :d] @ E.T
    s = s[:, 1:]                                          # column i: item i + 1
    lse = torch.logsumexp(s, 1)
    live = y != 0
    assert 150.0 < float(s[live].abs().max()) < 260.0
    other_split = 0
    for t, a in plan["argmax"].items():
        assert int(s[t].argmax()) + 1 == a, (t, a)
        tg = int(y[t])
        loss = float(lse[t] - s[t, tg - 1])
        if tg == a:                                       # the target is the maximum by a wide gap
            assert float(s[t, a - 1] - s[t].topk(2).values[1]) > 50.0 and loss < 1e-9
        else:                                             # the target is far below the maximum
            assert loss > 50.0
            other_split += (a // 64) != (tg // 64)
    assert other_split >= 3
    assert {1, 64, 65, c["n_items"]} <= set(plan["argmax"].values())
    z = plan["zero"]
    assert abs(float(lse[z] - s[z, int(y[z]) - 1]) - math.log(c["n_items"])) < 1e-12


# ------------------------------------------------------------------------------------------------ shared negatives
SXENT_ITEMS, SXENT_K = 300, 130     # slots 0..129: three 64-slot chunks, the last of two slots; three candidate splits
SXENT_LQ_SLOT = 7                   # the slot whose log_q = -30 makes it the maximum of the small-logit token


def sxent_case(d_item, d_fake=0, seed=0):
    n, K = SXENT_ITEMS, SXENT_K
    max_slots = [0, 63, 64, K - 1]
    ids = [11, 12, 13, 14]                               # the items planted at those slots
    g, E, h, y = _base(d_item, d_fake, n, seed, ids + [150])
    y[y <= 20] = 0                                        # ids 1..20 are reserved for the planted slots
    neg = torch.randint(21, n + 1, (K,), generator=g)
    neg[1::5] = 0                                         # unused slots
    neg[2::7] = neg[5]                                    # duplicates
    tg = y[y != 0]
    neg[3::6] = tg[torch.randint(0, tg.numel(), (len(range(3, K, 6)),), generator=g)]      # accidental hits
    neg[SXENT_LQ_SLOT] = 15
    for sl, j in zip(max_slots, ids):
        neg[sl] = j
    log_q = torch.rand(K, generator=g) * 50.0 - 25.0
    log_q[max_slots] = 0.0
    log_q[SXENT_LQ_SLOT] = -30.0
    log_q[9], log_q[70] = 30.0, -20.0
    slots = _live(y)[:len(ids) + 3]
    plan = {"argmax_slot": {}, "target_max": slots[4], "lq_only": slots[5], "zero": slots[6]}
    for t, sl, j in zip(slots, max_slots, ids):
        _plant(h, t, E, j, d_item)
        y[t] = 250
        plan["argmax_slot"][t] = sl
    _plant(h, plan["target_max"], E, 150, d_item)
    y[plan["target_max"]] = 150
    neg[neg == 150] = 151
    y[plan["lq_only"]] = 260
    y[plan["zero"]] = 270
    h = _finish(h, d_item, 180.0, lambda hh: hh[:, :d_item] @ E.double()[torch.cat([neg, y.clamp(min=0)])].T, slots)
    h[plan["zero"], :d_item] = 0.0
    h[plan["lq_only"], :d_item] *= 2.0 / float((h[plan["lq_only"], :d_item].double() @ E.double().T).abs().max())
    return dict(h=h.view(B, L, -1), E=E, y=y.view(B, L), neg=neg, log_q=log_q, plan=plan, n_items=n)


def check_sxent_case(c):
    from tests.loss_refs import sxent_logits_ref
    E, y, neg, plan = c["E"].double(), c["y"], c["neg"], c["plan"]
    h = c["h"].double()
    pos = (y.view(-1) != 0).nonzero().view(-1).tolist()
    row = {t: i for i, t in enumerate(pos)}               # position -> row of the token list
    tok, sp, sn = sxent_logits_ref(h, E, y, neg, None, True)
    _, _, snq = sxent_logits_ref(h, E, y, neg, c["log_q"].double(), True)
    big = max(float(sp.abs().max()), float(sn[sn.isfinite()].abs().max()))
    assert 150.0 < big < 260.0
    assert float(c["log_q"].min()) == -30.0 and float(c["log_q"].max()) == 30.0
    assert bool((neg == 0).any()) and neg.unique().numel() < neg.numel()
    assert bool((neg[None, :] == y.view(-1)[tok][:, None]).any())              # accidental hits
    for t, sl in plan["argmax_slot"].items():
        for s_ in (sn, snq):                              # the planted slot is the maximum, the target far below it
            assert int(s_[row[t]].argmax()) == sl and float(s_[row[t], sl] - sp[row[t]]) > 50.0, (t, sl)
    assert {0, 63, 64, SXENT_K - 1} == set(plan["argmax_slot"].values())
    r = row[plan["target_max"]]
    assert float(sp[r] - snq[r].max()) > 50.0 and float(sp[r]) > 150.0
    r = row[plan["lq_only"]]                              # the maximum only because of log_q
    assert int(snq[r].argmax()) == SXENT_LQ_SLOT and float(snq[r].max()) > float(sp[r]) + 20.0
    assert int(sn[r].argmax()) != SXENT_LQ_SLOT
    r = row[plan["zero"]]
    n_part = int(sn[r].isfinite().sum())
    assert abs(float(torch.logsumexp(torch.cat([sp[r:r + 1], sn[r]]), 0) - sp[r]) - math.log(1 + n_part)) < 1e-12


def sxent_hits_case(d_item, d_fake=0, seed=0):
    """every participating slot holds item 40: the tokens whose target is 40 lose every negative to hit removal, their
    neighbours (target 41) none"""
    g, E, h, y = _base(d_item, d_fake, 100, seed, [40])
    neg = torch.tensor([40, 0, 40, 40])
    log_q = torch.tensor([30.0, 0.0, -30.0, 3.0])
    live = _live(y)
    for i, t in enumerate(live):
        y[t] = 40 if i % 2 == 0 else 41
    planted = [t for t in range(T) if t not in live]      # (the scale is taken over the tokens alone)
    h = _finish(h, d_item, 180.0, lambda hh: hh[:, :d_item] @ E.double()[[40, 41]].T, planted)
    return dict(h=h.view(B, L, -1), E=E, y=y.view(B, L), neg=neg, log_q=log_q, n_items=100)


# ------------------------------------------------------------------------------------------------ K negatives per position
TNEG_ITEMS, TNEG_K = 300, 65        # slot 0 is the target, slot 1 + k negative k, walked in steps of 16 slots
TNEG_MAX_AT = (0, 14, 15, 16, 63, 64)   # negatives planted as the maximum: first, both sides of a step seam, last
TNEG_LQ_AT = 5


def tneg_case(d_item, d_fake=0, seed=0):
    n, K = TNEG_ITEMS, TNEG_K
    ids = list(range(1, 1 + len(TNEG_MAX_AT)))
    g, E, h, y = _base(d_item, d_fake, n, seed, ids + [150, 160, 170])
    y[y <= 20] = 0
    neg = torch.randint(21, n + 1, (T, K), generator=g)
    neg[torch.rand(T, K, generator=g) < 0.2] = 0                                   # unused slots
    hit = torch.rand(T, K, generator=g) < 0.1                                      # accidental hits
    neg = torch.where(hit, y[:, None].expand(-1, K), neg)
    neg[:, 2] = neg[:, 0]                                                          # duplicates inside a position
    neg[neg == 150] = 151
    log_q = torch.rand(T, K, generator=g) * 60.0 - 30.0
    slots = _live(y)[:len(ids) + 7]
    plan = {"argmax_neg": {}}
    for t, k, j in zip(slots, TNEG_MAX_AT, ids):
        _plant(h, t, E, j, d_item)
        y[t] = 250
        neg[t, k] = j
        log_q[t, k] = 0.0
        plan["argmax_neg"][t] = k
    names = ("target_max", "target_min", "neg_min", "lq_only", "zero", "all_removed", "none_removed")
    plan.update(dict(zip(names, slots[len(ids):])))
    t = plan["target_max"]
    _plant(h, t, E, 150, d_item)
    y[t] = 150
    t = plan["target_min"]                                # s+ = -200
    _plant(h, t, E, 160, d_item, -BIG)
    y[t] = 160
    t = plan["neg_min"]                                   # a negative at -200
    _plant(h, t, E, 170, d_item, -BIG)
    y[t] = 255
    neg[t, 3] = 170
    t = plan["lq_only"]
    y[t] = 260
    neg[t, TNEG_LQ_AT] = 30
    log_q[t] = log_q[t].clamp(min=-5.0)
    log_q[t, TNEG_LQ_AT] = -30.0
    y[plan["zero"]] = 270
    t = plan["all_removed"]
    y[t] = 280
    neg[t] = torch.where(torch.arange(K) % 2 == 0, 280, 0)
    t = plan["none_removed"]
    y[t] = 281
    neg[t] = torch.randint(21, 250, (K,), generator=g)
    log_q[slots[1], 40] = 30.0

    def logits_of(hh):
        Ed = E.double()
        return torch.cat([(hh[:, :d_item] * Ed[y]).sum(1, keepdim=True), torch.einsum("td,tkd->tk", hh[:, :d_item], Ed[neg])], 1)

    h = _finish(h, d_item, 180.0, logits_of, slots)
    h[plan["zero"], :d_item] = 0.0
    t = plan["lq_only"]
    h[t, :d_item] *= 2.0 / float(logits_of(h.double())[t].abs().max())
    return dict(h=h.view(B, L, -1), E=E, y=y.view(B, L), neg=neg.view(B, L, K), log_q=log_q.view(B, L, K), plan=plan,
                n_items=n)


def tneg_logits(c, with_log_q):
    """fp64 (s+ (T,), negative logits (T, K) minus log_q if asked, participation mask (T, K) under hit removal)"""
    E, y, neg = c["E"].double(), c["y"].view(-1), c["neg"].view(T, -1)
    d = E.shape[1]
    H = c["h"].view(T, -1).double()[:, :d]
    sp = (H * E[y]).sum(1)
    sn = torch.einsum("td,tkd->tk", H, E[neg])
    if with_log_q:
        sn = sn - c["log_q"].view(T, -1).double()
    part = (neg != 0) & (neg != y[:, None]) & (y != 0)[:, None]
    return sp, sn, part


def check_tneg_case(c):
    plan, y = c["plan"], c["y"].view(-1)
    sp, sn, part = tneg_logits(c, False)
    _, snq, _ = tneg_logits(c, True)
    live = y != 0
    assert 150.0 < max(float(sp[live].abs().max()), float(sn[part].abs().max())) < 260.0
    assert float(c["log_q"].min()) == -30.0 and float(c["log_q"].max()) == 30.0
    ninf = -float("inf")
    for t, k in plan["argmax_neg"].items():
        for s_ in (sn, snq):
            m = s_[t].masked_fill(~part[t], ninf)
            assert int(m.argmax()) == k and float(m[k] - sp[t]) > 50.0, (t, k)
    t = plan["target_max"]
    assert float(sp[t]) > 150.0 and float(sp[t] - snq[t].masked_fill(~part[t], ninf).max()) > 50.0
    t = plan["target_min"]                                # gbce: a positive near -200
    assert float(sp[t]) < -150.0
    t = plan["neg_min"]
    assert bool(part[t, 3]) and float(sn[t, 3]) < -150.0
    assert float(sn[part].max()) > 150.0                  # gbce: negatives near +200 (the planted maxima)
    t = plan["lq_only"]
    m, mq = sn[t].masked_fill(~part[t], ninf), snq[t].masked_fill(~part[t], ninf)
    assert int(mq.argmax()) == TNEG_LQ_AT and float(mq.max()) > float(sp[t]) + 20.0 and int(m.argmax()) != TNEG_LQ_AT
    t = plan["zero"]
    assert float(c["h"].view(T, -1)[t, :c["E"].shape[1]].abs().max()) == 0.0 and int(part[t].sum()) > 0
    a, b = plan["all_removed"], plan["none_removed"]
    assert b == a + 1 and int(part[a].sum()) == 0 and bool((c["neg"].view(T, -1)[a] != 0).any()) and bool(part[b].all())
