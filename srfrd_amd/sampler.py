"""Synthetic batches in the reference sampler's layout (reference utils.py:21-57, ``sample_function_fr``).

One batch is the 7-tuple ``(user, seq, rsq, pos, prs, neg, nrs)``: ``user`` (B,), the rest int64 (B, L),
LEFT-padded with 0; ``pos[t] = seq[t+1]`` with the held-out next item in the last column; ``neg[t]`` is a random
item outside the user's own items wherever ``pos[t] != 0``; ``rsq / prs`` hold 1 (fake) / 2 (real) / 0 (pad) and
``nrs`` is 1 wherever set (reference utils.py:52 draws ``randint(1, 2)``).

The generator is counter-seeded (seed, batch index, rank) so every data-parallel rank can regenerate its own shard,
and it runs on the target device so the timed loop never waits for a host sampler.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def synthetic_batch(n_items: int, max_len: int, batch: int, *, seed: int = 1, index: int = 0, rank: int = 0,
                    device="cpu", fake_prob: float = 0.3, n_users: int | None = None, min_len: int = 2,
                    packed: bool = False):
    """Uniform item ids over [1, n_items], lengths ~ U[min_len, max_len] (SURVEY 8d workload definition)."""
    g = torch.Generator(device="cpu")
    g.manual_seed((seed * 1_000_003 + index) * 1009 + rank)
    B, L = batch, max_len
    lens = torch.randint(min(min_len, L), L + 1, (B,), generator=g)
    items = torch.randint(1, n_items + 1, (B, L + 1), generator=g)          # L inputs + the final target
    revs = torch.where(torch.rand(B, L + 1, generator=g) < fake_prob, 1, 2)
    negs = torch.randint(1, n_items + 1, (B, L), generator=g)
    col = torch.arange(L).unsqueeze(0)
    valid = col >= (L - lens).unsqueeze(1)                                   # left padding
    seq = torch.where(valid, items[:, :L], 0)
    rsq = torch.where(valid, revs[:, :L], 0)
    pos = torch.where(valid, items[:, 1:], 0)
    prs = torch.where(valid, revs[:, 1:], 0)
    # negatives must avoid the user's own items (utils.py:14-19 random_neq): resample collisions a few rounds
    own = torch.cat([seq, pos[:, -1:]], dim=1)
    for _ in range(8):
        clash = (negs.unsqueeze(2) == own.unsqueeze(1)).any(dim=2)
        if not bool(clash.any()):
            break
        negs = torch.where(clash, torch.randint(1, n_items + 1, (B, L), generator=g), negs)
    neg = torch.where(valid, negs, 0)
    nrs = valid.to(torch.int64)
    user = torch.randint(1, (n_users or B) + 1, (B,), generator=g)
    if packed:
        return user.to(device), torch.stack([seq, rsq, pos, prs, neg, nrs]).to(device=device, dtype=torch.int64)
    return tuple(t.to(device=device, dtype=torch.int64) for t in (user, seq, rsq, pos, prs, neg, nrs))


def sample_negatives(n_items: int, num: int, counts=None, alpha: float = 1.0, generator=None, device="cuda"):
    """Shared negatives for ``model.sampled_softmax_loss``: ``num`` item ids drawn with replacement from 1..n_items, uniformly
    or with probability q_j proportional to ``counts[j] ** alpha`` (``counts`` indexed by item id, shape (n_items + 1,);
    entry 0, the padding id, is ignored).  Returns ``(ids, log_q)``: ids int64 (num,) and ``log_q = log(num * q_ids)`` float32
    (num,), the log-Q correction under which the sampled sum of exps estimates the full partition function.  Drawn with
    torch on ``device`` (``generator``, if given, must live there)."""
    if n_items < 1 or num < 1:
        raise ValueError(f"n_items and num must be positive (got {n_items}, {num})")
    if counts is None:
        ids = torch.randint(1, n_items + 1, (num,), generator=generator, device=device)
        log_q = torch.full((num,), math.log(num / n_items), device=device, dtype=torch.float32)
        return ids, log_q
    c = torch.as_tensor(counts, device=device, dtype=torch.float64)
    if tuple(c.shape) != (n_items + 1,):
        raise ValueError(f"counts must have shape ({n_items + 1},) (indexed by item id), got {tuple(c.shape)}")
    w = c[1:].clamp_min(0) ** alpha
    total = w.sum()
    if not bool(total > 0):
        raise ValueError("counts ** alpha has no positive weight")
    q = w / total
    ids = torch.multinomial(q, num, replacement=True, generator=generator) + 1
    log_q = torch.log(num * q[ids - 1]).to(torch.float32)
    return ids, log_q


def sample_token_negatives(n_items: int, positive_ids, num: int, counts=None, alpha: float = 1.0, generator=None):
    """Per-position negatives for ``model.token_negatives_loss``: for every position of ``positive_ids`` (B, L) with a target,
    ``num`` item ids drawn with replacement from 1..n_items, uniformly or with probability q_j proportional to
    ``counts[j] ** alpha`` (``counts`` as in ``sample_negatives``); id 0 in every slot of a position without a target.
    Returns ``(negative_ids (B, L, num) int64, log_q (B, L, num) float32)`` with ``log_q = log(num * q_ids)`` (0 in the
    id-0 slots).  Drawn with torch on the device of ``positive_ids`` (``generator``, if given, must live there).  The draws
    do not avoid the user's history: accidental hits on the position's own target are dropped by the loss.  For negatives
    outside the user's history as the reference samples them, reproducible from (seed, batch index) and drawn by one
    kernel launch without an allocation, use ``DeviceSampler(..., num_negatives=num)`` (``sampler.negatives`` /
    ``sampler.log_q``, or ``sampler.token_negatives`` for a batch that came from elsewhere)."""
    pos = torch.as_tensor(positive_ids)
    if pos.dim() != 2:
        raise ValueError(f"positive_ids must be (batch, seq_len) (got shape {tuple(pos.shape)})")
    if n_items < 1 or num < 1:
        raise ValueError(f"n_items and num must be positive (got {n_items}, {num})")
    dev = pos.device
    B, L = pos.shape
    if counts is None:
        ids = torch.randint(1, n_items + 1, (B, L, num), generator=generator, device=dev)
        log_q = torch.full((B, L, num), math.log(num / n_items), device=dev, dtype=torch.float32)
    else:
        q = torch.as_tensor(negative_q(n_items, counts, alpha), device=dev)
        ids = torch.multinomial(q, B * L * num, replacement=True, generator=generator).view(B, L, num) + 1
        log_q = torch.log(num * q[ids - 1]).to(torch.float32)
    live = (pos != 0).unsqueeze(-1)
    return torch.where(live, ids, torch.zeros_like(ids)), torch.where(live, log_q, torch.zeros_like(log_q))


def gbce_beta(n_items: int, num_negatives: int, t: float) -> float:
    """gSASRec's beta for ``token_negatives_loss(objective="gbce")``: with the sampling rate ``alpha = K / (n_items - 1)``,
    ``beta = alpha * (t * (1 - 1 / alpha) + 1 / alpha)``; the calibration t = 0 gives 1.0 (plain BCE), t = 1 gives alpha (the
    fully calibrated loss)."""
    if not 0.0 <= t <= 1.0:
        raise ValueError(f"t must lie in [0, 1] (got {t})")
    if not 1 <= num_negatives <= n_items - 1:
        raise ValueError(f"num_negatives must lie in [1, n_items - 1] (got {num_negatives} for {n_items} items)")
    a = num_negatives / (n_items - 1)
    return a * (t * (1.0 - 1.0 / a) + 1.0 / a)


def negative_q(n_items: int, counts, alpha: float = 1.0):
    """The sampling distribution of ``sample_negatives`` as fp64 numpy (n_items,): q[i] for item id i + 1, proportional to
    ``counts[i + 1] ** alpha`` (entry 0, the padding id, ignored; negative counts taken as 0)."""
    c = np.asarray(torch.as_tensor(counts).detach().cpu().to(torch.float64))
    if c.shape != (n_items + 1,):
        raise ValueError(f"counts must have shape ({n_items + 1},) (indexed by item id), got {tuple(c.shape)}")
    w = np.maximum(c[1:], 0.0) ** float(alpha)
    total = w.sum()
    if not total > 0 or not np.isfinite(total):
        raise ValueError("counts ** alpha has no positive (finite) weight")
    return w / total


def history_log_keep(data, q=None):
    """float32 (usernum + 1,): ``log(1 - sum of q over the DISTINCT training items of user u)``, the log of the mass that
    rejecting u's history leaves of the sampling distribution ``q`` (fp64 (itemnum,), ``q[i]`` for item id i + 1, as
    ``negative_q`` returns it); ``q=None`` is the uniform distribution: ``log(1 - distinct / itemnum)``.  Computed in fp64.
    Subtracted from ``log(K q)`` it gives the log-Q correction of negatives drawn outside the history
    (``DeviceSampler(num_negatives=K)``).  A user whose history carries all the mass gets ``-inf``: every slot of such a
    user comes out 0, so the value is never read at a kept slot."""
    n_users, n_items = data.usernum + 1, data.itemnum
    owner = np.repeat(np.arange(n_users, dtype=np.int64), data.train_len())
    its = np.asarray(data.train_items[: owner.size], dtype=np.int64)
    ok = (its >= 1) & (its <= n_items)
    pairs = np.unique(owner[ok] * (n_items + 1) + its[ok])            # one entry per (user, distinct item)
    pu, pi = pairs // (n_items + 1), pairs % (n_items + 1)
    if q is None:
        keep = 1.0 - np.bincount(pu, minlength=n_users).astype(np.float64) / n_items
        full = np.bincount(pu, minlength=n_users) >= n_items
    else:
        q = np.asarray(q, dtype=np.float64)
        if q.shape != (n_items,):
            raise ValueError(f"q must have shape ({n_items},) (q[i] for item id i + 1), got {q.shape}")
        keep = 1.0 - np.bincount(pu, weights=q[pi - 1], minlength=n_users)
        # all the mass: every item of positive weight is in the history (the fp64 sum may miss 1 by a rounding)
        full = np.bincount(pu, weights=(q[pi - 1] > 0).astype(np.float64), minlength=n_users) >= np.count_nonzero(q > 0)
    keep = np.where(full, 0.0, np.maximum(keep, 0.0))
    with np.errstate(divide="ignore"):
        return np.log(keep).astype(np.float32)


def alias_table(q):
    """Walker / Vose alias table of the distribution q (n,) (fp64, summing to 1): (alias_prob float32 (n,), alias_idx int32
    (n,)).  Drawing bucket b uniformly, then keeping b with probability alias_prob[b] and otherwise taking alias_idx[b],
    gives b' with probability q[b'].  Built in fp64; only the stored probabilities are rounded to fp32."""
    q = np.asarray(q, dtype=np.float64)
    n = q.size
    p = q * n
    prob = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int32)
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if p[i] >= 1.0]
    while small and large:
        s, g = small.pop(), large.pop()
        prob[s], alias[s] = p[s], g
        p[g] = (p[g] + p[s]) - 1.0
        (small if p[g] < 1.0 else large).append(g)
    # what is left has p == 1 up to rounding: kept with probability 1 (prob and alias already say so)
    return prob.astype(np.float32), alias


def eval_candidates(n_items: int, seq: torch.Tensor, target: torch.Tensor, n_neg: int = 100, *, seed: int = 7):
    """(B, 1 + n_neg) candidates per user: the true next item followed by sampled negatives that are neither 0 nor
    in the user's history (reference utils.py:576-583)."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    seq_c, tgt = seq.cpu(), target.cpu().view(-1, 1)
    B = seq_c.shape[0]
    negs = torch.randint(1, n_items + 1, (B, n_neg), generator=g)
    for _ in range(8):
        clash = (negs.unsqueeze(2) == seq_c.unsqueeze(1)).any(dim=2)
        if not bool(clash.any()):
            break
        negs = torch.where(clash, torch.randint(1, n_items + 1, (B, n_neg), generator=g), negs)
    return torch.cat([tgt, negs], dim=1).to(device=seq.device, dtype=torch.int64)
