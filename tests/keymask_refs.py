"""The key-padding mask's reference (no GPU): ``srfrd_layout.flags & SRFRD_LAYOUT_MASK_PAD_KEYS`` (include/srfrd_hip.h).

``masked()`` is a context manager that swaps ``oracle.srfrd_oracle.encoder_block`` for ``masked_encoder_block`` - the oracle's
block with the LEADING pads of every sequence taken out of its attention keys - and puts the oracle's own back.  ``O.forward``
looks the block up on every call, so everything that goes through it follows inside the context: ``grad_refs.build_ref``,
``fwd_refs.build_ref``, ``relu_margin``, ``O.grads_of``, ``O.predict``.  The ``lru_cache``d ``grad_refs.reference`` /
``fwd_refs.reference`` must never be called inside it (an entry built under the swap would stay for the unmasked suites): the
masked references live in this file's own caches, ``grad_reference`` / ``fwd_reference``.

Semantics, as the header states them: t0(b) = the index of the first non-zero input id (L: none).  A live query row r >= t0 has
P[r, j] = softmax over t0 <= j <= r, keys j < t0 an exact 0 and no part in the row maximum; an id 0 at a position >= t0 stays a
key; a pad query row r < t0 keeps its causal keys (finite values, masked to zero behind the FFN, no gradient).

Cases, weights, metric, bounds and clamp lists are grad_refs' and fwd_refs', unchanged.  Batches too, but for KEYMASK_SEEDS.
"""
import contextlib
import math

import torch

from oracle import srfrd_oracle as O
from tests import fwd_refs as F
from tests import grad_refs as G

_ORACLE_BLOCK = O.encoder_block


def leading_pads(keep):
    """keep (B, L, 1), the oracle's pad mask -> (B,) index of each sequence's first live position, L where it has none"""
    live = keep.reshape(keep.shape[0], keep.shape[1]) != 0
    L = live.shape[1]
    idx = torch.arange(L).expand_as(live)
    return torch.where(live, idx, torch.full_like(idx, L)).min(dim=1).values


def gone_keys(keep):
    """(B, 1, L, L) bool: [b, 0, r, j] <=> key j is a leading pad of sequence b and query r is not (j < t0 <= r)"""
    L = keep.shape[1]
    t0 = leading_pads(keep).view(-1, 1, 1, 1)
    j = torch.arange(L).view(1, 1, 1, L)
    r = torch.arange(L).view(1, 1, L, 1)
    return (j < t0) & (r >= t0)


def masked_encoder_block(cfg, sd, i, x, keep, m_attn=None, m_f1=None, m_f2=None, taps=None):
    """O.encoder_block, operation for operation, with the leading pads masked out of the keys; fills the same taps"""
    B, L, D = x.shape
    H = cfg.num_heads
    dh = D // H
    pre = f"attention_layers.{i}."
    W, bias = sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"]
    qn = O.layer_norm(x, sd[f"attention_layernorms.{i}.weight"], sd[f"attention_layernorms.{i}.bias"])
    q = qn @ W[:D].T + bias[:D]
    k = x @ W[D:2 * D].T + bias[D:2 * D]
    v = x @ W[2 * D:].T + bias[2 * D:]
    q = q * math.sqrt(1.0 / dh)
    qh = q.view(B, L, H, dh).transpose(1, 2)
    kh = k.view(B, L, H, dh).transpose(1, 2)
    vh = v.view(B, L, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool))
    s = s.masked_fill(~causal | gone_keys(keep), float("-inf"))
    p = torch.softmax(s, dim=-1)
    if taps is not None:
        taps[f"qn{i}"], taps[f"q{i}"], taps[f"k{i}"], taps[f"v{i}"], taps[f"p{i}"] = qn, q, k, v, p
    if m_attn is not None:
        p = p * (m_attn if m_attn.dim() == 4 else m_attn.unsqueeze(1))
    o = (p @ vh).transpose(1, 2).reshape(B, L, D)
    o = o @ sd[pre + "out_proj.weight"].T + sd[pre + "out_proj.bias"]
    h1 = qn + o
    h2 = O.layer_norm(h1, sd[f"forward_layernorms.{i}.weight"], sd[f"forward_layernorms.{i}.bias"])
    fp = f"forward_layers.{i}."
    a1 = h2 @ sd[fp + "conv1.weight"].squeeze(-1).T + sd[fp + "conv1.bias"]
    if m_f1 is not None:
        a1 = a1 * m_f1
    r = torch.relu(a1)
    a2 = r @ sd[fp + "conv2.weight"].squeeze(-1).T + sd[fp + "conv2.bias"]
    if m_f2 is not None:
        a2 = a2 * m_f2
    y = (a2 + h2) * keep
    if taps is not None:
        taps[f"o{i}"], taps[f"h1{i}"], taps[f"h2{i}"], taps[f"y{i}"] = o, h1, h2, y
    return y


@contextlib.contextmanager
def masked():
    """inside: the oracle masks the leading pads out of the attention keys"""
    before = O.encoder_block
    O.encoder_block = masked_encoder_block
    try:
        yield
    finally:
        O.encoder_block = before


# (case id, mode) -> batch seed where the job's own (grad_refs.SEEDS; fwd_refs.seed_of) is not admissible under the masked
# reference: chosen by the suites' rule under the swap - grad_refs.scan_seeds / pick_seed for "autograd" and "fused" (ReLU
# margin >= 2 * RELU_MARGIN and 64 e32 <= SEARCH_HEADROOM * CAP), fwd_refs.scan_seeds / pick_seed for "eval", "last" and
# "train" - by ``pick`` below.  The clamp lists are grad_refs.OVER_CAP and fwd_refs.FWD_OVER_CAP as they stand: a clamped job
# needs the ReLU margin alone.  Scanned over 12 seeds, then 48, then 200 (t3 fused, h.3 autograd; and the depth-8 fused steps of
# t0 and t2, clamped jobs with 19 batches of 200 that keep the margin: the one whose e32 is smallest, 3.1e-6 and 3.8e-6).
KEYMASK_SEEDS = {
    ("b", "autograd"): 20, ("b", "fused"): 54, ("c", "fused"): 53, ("d", "fused"): 52, ("d", "train"): 52,
    ("e", "fused"): 50, ("f", "autograd"): 22, ("h", "autograd"): 10, ("h", "fused"): 62, ("j", "train"): 57,
    ("k", "autograd"): 12, ("k", "fused"): 74, ("l", "autograd"): 18, ("l", "fused"): 55, ("n", "train"): 57,
    ("o", "autograd"): 15, ("o", "fused"): 72, ("p", "autograd"): 20, ("p", "fused"): 54, ("s", "eval"): 7,
    ("t0", "autograd"): 6, ("t0", "fused"): 52, ("t0", "eval"): 13, ("t1", "fused"): 66, ("t2", "autograd"): 22,
    ("t2", "fused"): 89, ("t3", "fused"): 136, ("u0", "fused"): 51, ("u2", "fused"): 63, ("g.1", "fused"): 51,
    ("i.1", "fused"): 51, ("k.1", "autograd"): 13, ("k.1", "fused"): 70, ("t2.1", "autograd"): 9, ("a.3", "fused"): 67,
    ("b.3", "autograd"): 31, ("c.3", "fused"): 93, ("d.3", "fused"): 84, ("g.3", "fused"): 91, ("h.3", "autograd"): 62,
    ("h.3", "fused"): 80, ("i.3", "fused"): 91, ("j.3", "autograd"): 15, ("j.3", "fused"): 82, ("k.3", "autograd"): 39,
    ("n.3", "autograd"): 15, ("n.3", "fused"): 82, ("p.3", "autograd"): 31, ("q.3", "fused"): 67, ("s.3", "autograd"): 6,
    ("s.3", "fused"): 53, ("t0.3", "autograd"): 8, ("t0.3", "fused"): 56, ("t0.3", "train"): 52, ("t2.3", "autograd"): 19,
    ("t2.3", "fused"): 58, ("t0.8", "autograd"): 22, ("t0.8", "fused"): 187, ("t2.8", "autograd"): 18, ("t2.8", "fused"): 175,
    ("t2.8", "eval"): 48, ("g.8", "autograd"): 50, ("l.8", "autograd"): 40, ("l.8", "fused"): 65,
    ("d.8", "autograd"): 10, ("d.8", "eval"): 64,
}
GRAD_MODES = ("autograd", "fused")


def grad_seed(cid, mode):
    return KEYMASK_SEEDS.get((cid, mode), G.SEEDS[cid, mode])


def fwd_seed(cid, mode):
    return KEYMASK_SEEDS.get((cid, mode), F.seed_of(cid, mode))


_GRAD, _FWD = {}, {}


def grad_reference_at(cid, mode, seed, l2=0.0):
    key = (cid, mode, seed, l2)
    if key not in _GRAD:
        with masked():
            _GRAD[key] = G.build_ref(G.BY_ID[cid], mode, seed, l2)
    return _GRAD[key]


def grad_reference(cid, mode, l2=0.0):
    """grad_refs.reference under the mask: the Ref of one case and mode, shared by every test of the process; read-only"""
    return grad_reference_at(cid, mode, grad_seed(cid, mode), l2)


def fwd_reference_at(cid, mode, seed):
    key = (cid, mode, seed)
    if key not in _FWD:
        with masked():
            _FWD[key] = F.build_ref(G.BY_ID[cid], mode, seed)
    return _FWD[key]


def fwd_reference(cid, mode):
    """fwd_refs.reference under the mask"""
    return fwd_reference_at(cid, mode, fwd_seed(cid, mode))


def fused_step_reference(cid):
    """the masked train-mode FwdRef on the batch of the masked fused step: its fp64 loss is that step's loss"""
    return fwd_reference_at(cid, "train", grad_seed(cid, "fused"))


def pick(cid, mode, count=12):
    """-> (seed, found) for one job under the mask, on THIS machine's CPU: the job's present seed where it meets the suites'
    search rule, else the rule's pick among `count` seeds from the suite's first one on"""
    with masked():
        if mode in GRAD_MODES:
            ref = G.build_ref(G.BY_ID[cid], mode, G.SEEDS[cid, mode])
            if ref.margin >= 2 * G.RELU_MARGIN and (ref.clamp or G.FACTOR * max(ref.e32.values()) <= G.SEARCH_HEADROOM * G.CAP):
                return G.SEEDS[cid, mode], True
            return G.pick_seed([G.scan_seeds((cid, mode, count))])
        ref = F.build_ref(G.BY_ID[cid], mode, F.seed_of(cid, mode))
        if ref.clamp or F.FACTOR_FWD * F.worst_e32(ref) <= G.SEARCH_HEADROOM * F.CAP_FWD:
            return F.seed_of(cid, mode), True
        return F.pick_seed([F.scan_seeds((cid, mode, count))])


# ---------------------------------------------------------------------------------------------------------------------------
# the window property: a masked model's live rows do not depend on how much padding precedes the history
# ---------------------------------------------------------------------------------------------------------------------------
WINDOW_HISTORIES = (1, 2, 3, 5, 11, 16, 17, 19, 20)      # items per user, at the short window 20
WINDOW_KINDS = ("SASRec", "SRFRN")
WINDOW_I = G.I


def window_cfg(kind, L):
    return O.Cfg(kind, WINDOW_I, L, 50 if kind == "SASRec" else 45, d_fake=0 if kind == "SASRec" else 5)


def window_weights(kind, long, short, sd_seed=G.SD_SEED):
    """(cfg, sd) of a model at max_len `long` and of one at `short` that holds the LAST `short` rows of its position table and
    every other tensor as it is"""
    from tests.gpu_util import random_sd
    cl, cs = window_cfg(kind, long), window_cfg(kind, short)
    sdl = random_sd(cl, sd_seed)
    sds = {k: v.clone() for k, v in sdl.items()}
    sds[O.key_pos(cs)] = sdl[O.key_pos(cl)][long - short:].clone()
    return (cl, sdl), (cs, sds)


def window_batch(long, short, seed=5):
    """(seq, rsq) at the long window and their last `short` columns: one user per entry of WINDOW_HISTORIES scaled to the
    short window (n * short / 20 items), left-padded"""
    g = torch.Generator().manual_seed(seed)
    ns = [n * short // 20 for n in WINDOW_HISTORIES]
    seq = torch.randint(1, WINDOW_I + 1, (len(ns), long), generator=g)
    rsq = torch.randint(1, 3, (len(ns), long), generator=g)
    for b, n in enumerate(ns):
        seq[b, :long - n] = 0
        rsq[b, :long - n] = 0
    return (seq, rsq), (seq[:, long - short:].contiguous(), rsq[:, long - short:].contiguous()), ns


def window_difference(h_long, h_short, ns):
    """max |difference| over the live rows of every user (hidden (B, L, d) at each window)"""
    worst = 0.0
    for b, n in enumerate(ns):
        worst = max(worst, float((h_long[b, -n:].double() - h_short[b, -n:].double()).abs().max()))
    return worst
