"""What the loss-head tests share (tests/test_gpu_xent.py, test_gpu_sxent.py, test_gpu_tneg.py, test_gpu_loss_widths.py,
test_gpu_loss_extreme.py, test_gpu_ce_trainer.py, test_gpu_token_trainer.py, grad_refs.py): the fp64 references over
materialised logits, the differentiable mean losses the train-step oracles apply to a hidden state, the inf-norm error measure,
the numpy restatement of the shared-negative sampler, and a Python restatement of the two run-time kernel choices of the heads
(with_ks in srfrd_xent_common.h, with_shape in srfrd_tneg.hip).  Plain torch and numpy: everything here runs on the CPU as
well, except head_model."""
import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------ kernel choice, restated
def xent_ks(d_item):
    """the KS instantiation with_ks picks for the six streaming kernels of the two softmax losses"""
    return (d_item + 3) // 4


def tneg_shape(d_item, table_addr=0):
    """(VEC, NJ) with_shape picks for tneg_fwd_kernel / tneg_bwd_kernel from the row width and the table's byte address"""
    if d_item % 4 == 0 and table_addr % 16 == 0:
        return 4, 1
    if d_item % 2 == 0 and table_addr % 8 == 0:
        return (2, 1) if d_item <= 32 else (2, 2)
    return 1, min((d_item + 15) // 16, 4)


TNEG_SHAPES = {(4, 1), (2, 1), (2, 2), (1, 1), (1, 2), (1, 3), (1, 4)}


# ------------------------------------------------------------------------------------------------ what the width tests run
WIDTHS = list(range(1, 65))
REQUIRED_WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 51, 52, 53, 63, 64)     # a thinned list keeps these
FAKE_CASES = [(d, f) for d in (3, 4, 26, 27, 45, 59, 63) for f in (1, 5) if d + f <= 64]
ALIGN_WIDTHS = (16, 32, 48, 64)
ALIGN_OFFSETS = (0, 1, 2)       # floats past a 16-byte boundary


# ------------------------------------------------------------------------------------------------ models and calls
def head_model(d_item, d_fake, n_items, L, table=None):
    """SASRec, or SRFRN (d_out = d_item + d_fake) when d_fake > 0, on the GPU; the item table N(0, 0.5) or a copy of `table`"""
    import srfrd_amd
    if d_fake:
        m = srfrd_amd.SRFRN(n_items, L, d_item, d_fake, 0.0, 2, 1, "cuda").to("cuda")
    else:
        m = srfrd_amd.SASRec(n_items, L, d_item, 0.0, 2, 1, "cuda").to("cuda")
    with torch.no_grad():
        if table is None:
            head_table(m).normal_(0, 0.5)
        else:
            head_table(m).copy_(table)
    return m


def head_table(m):
    return m.item_emb.weight if hasattr(m, "item_emb") else m.embedding_layer.item_embed.weight


def run_head(m, call, h):
    """call(hidden) -> loss; -> (loss, d_hidden, table gradient)"""
    table = head_table(m)
    table.grad = None
    hh = h.detach().clone().requires_grad_(True)
    loss = call(hh)
    loss.backward(torch.ones_like(loss))
    return loss.detach(), hh.grad, table.grad.clone()


# ------------------------------------------------------------------------------------------------ input generators
def shared_negatives(K, n_items, y, seed):
    """ids in 0..n_items with id-0 slots, duplicates and accidental hits (targets of the batch)"""
    g = torch.Generator().manual_seed(seed)
    neg = torch.randint(1, n_items + 1, (K,), generator=g)
    if K >= 4:
        neg[1::5] = 0                                   # unused slots
        neg[2::7] = neg[0]                              # duplicates
        tg = y[y != 0].view(-1).cpu()
        if tg.numel():
            neg[3::6] = tg[torch.randint(0, tg.numel(), (len(range(3, K, 6)),), generator=g)]   # accidental hits
    return neg


def make_inputs(B, L, K, n_items, seed, empty_rows=(2,), zero_frac=0.3):
    """(targets (B, L), negatives (B, L, K)) on the CPU with id-0 slots, duplicate ids inside one position, accidental hits,
    rows of the batch without any target, every tenth token with all slots unused and every tenth (offset 1) with every
    slot unused or the target's own id: those tokens have no participating slot (under hit removal, for the second kind)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, n_items + 1, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < zero_frac] = 0
    for b in empty_rows:
        y[b] = 0
    neg = torch.randint(1, n_items + 1, (B, L, K), generator=g)
    neg[torch.rand(B, L, K, generator=g) < 0.2] = 0                                  # unused slots
    hit = torch.rand(B, L, K, generator=g) < 0.15                                    # accidental hits
    neg = torch.where(hit, y.unsqueeze(-1).expand_as(neg), neg)
    if K >= 3:
        neg[..., 2] = neg[..., 0]                                                    # duplicates inside a position
    flat, yy = neg.view(-1, K), y.view(-1)
    live = (yy != 0).nonzero().view(-1)
    flat[live[0::10]] = 0
    mix = live[1::10]
    flat[mix] = torch.where(torch.rand(mix.numel(), K, generator=g) < 0.5, yy[mix].unsqueeze(1).expand(-1, K),
                            torch.zeros(mix.numel(), K, dtype=torch.int64))
    return y, neg


# ------------------------------------------------------------------------------------------------ error measure
def rel(a, b, abs_norm=0.0):
    """||a - b||_inf / ||b||_inf; abs_norm: the inf-norm of the same quantity summed over the absolute values of its terms,
    which floors the scale at 10 % of itself where the terms cancel (tests/test_gpu_sxent.py says why)"""
    scale = max(float(b.abs().max()), 0.1 * abs_norm)
    if scale == 0.0:
        return float(a.abs().max())
    return float((a.double() - b.double()).abs().max()) / scale


# ------------------------------------------------------------------------------------------------ full-catalog softmax
def xent_ref(h, E, y, reduction):
    """fp64 reference: loss and (d_hidden, dE) by autograd over materialised logits"""
    h64 = h.detach().double().requires_grad_(True)
    E64 = E.detach().double().requires_grad_(True)
    d = E.shape[1]
    logits = h64[..., :d] @ E64.T
    n = E.shape[0] - 1
    loss = F.cross_entropy(logits[..., 1:].reshape(-1, n), (y - 1).reshape(-1), ignore_index=-1, reduction=reduction)
    if reduction == "none":
        loss = loss.view(y.shape)
    loss.backward(torch.ones_like(loss))
    return loss.detach(), h64.grad, E64.grad


# ------------------------------------------------------------------------------------------------ shared negatives
def sxent_logits_ref(h64, E64, y, neg, log_q, remove):
    """-> (token mask, s+ (T,), masked negative logits (T, K)) in the dtype of h64 / E64"""
    d = E64.shape[1]
    hs = h64[..., :d].reshape(-1, d)
    yy = y.reshape(-1)
    tok = yy != 0
    H, t = hs[tok], yy[tok]
    sp = (H * E64[t]).sum(1)
    sn = H @ E64[neg].T
    if log_q is not None:
        sn = sn - log_q.to(sn.dtype)
    mask = (neg == 0).unsqueeze(0).expand_as(sn)
    if remove:
        mask = mask | (neg.unsqueeze(0) == t.unsqueeze(1))
    return tok, sp, sn.masked_fill(mask, -float("inf"))


def reduce_tokens(lt, tok, shape, reduction):
    if reduction == "mean":
        return lt.mean()
    if reduction == "sum":
        return lt.sum()
    full = torch.zeros(tok.numel(), dtype=lt.dtype, device=lt.device)
    return full.index_put((tok.nonzero().view(-1),), lt).view(shape)


def sxent_ref(h, E, y, neg, log_q, remove, reduction, with_abs=False):
    """fp64 reference: loss and (d_hidden, dE) by autograd over materialised logits; with_abs: also the inf-norms of the
    two gradients summed over the absolute values of their terms"""
    h64 = h.detach().double().requires_grad_(True)
    E64 = E.detach().double().requires_grad_(True)
    tok, sp, sn = sxent_logits_ref(h64, E64, y, neg, log_q, remove)
    lse = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1)
    loss = reduce_tokens(lse - sp, tok, y.shape, reduction)
    loss.backward(torch.ones_like(loss))
    gh = h64.grad if h64.grad is not None else torch.zeros_like(h64)
    ge = E64.grad if E64.grad is not None else torch.zeros_like(E64)
    if not with_abs:
        return loss.detach(), gh, ge
    with torch.no_grad():
        c = 1.0 / max(int(tok.sum()), 1) if reduction == "mean" else 1.0
        d = E.shape[1]
        H = h64.detach()[..., :d].reshape(-1, d)[tok].abs()
        Ea = E64.detach().abs()
        P = torch.exp(sn.detach() - lse.detach().unsqueeze(1)) * c
        gp = (torch.exp(sp.detach() - lse.detach()) - 1.0).abs() * c
        t = y.reshape(-1)[tok]
        ah = P @ Ea[neg] + gp.unsqueeze(1) * Ea[t]
        ae = torch.zeros_like(Ea).index_add_(0, neg, P.T @ H).index_add_(0, t, gp.unsqueeze(1) * H)
    return loss.detach(), gh, ge, float(ah.max()) if ah.numel() else 0.0, float(ae.max())


# ------------------------------------------------------------------------------------------------ K negatives per position
def tneg_ref(h, E, y, neg, log_q=None, remove=True, reduction="mean", objective="softmax", beta=1.0, with_abs=False, chunk=2048):
    """fp64 reference over materialised logits, in token chunks: loss and (d_hidden, dE) by autograd; with_abs: also the
    inf-norms of the two gradients summed over the absolute values of their terms"""
    d, K = E.shape[1], neg.shape[-1]
    h64 = h.detach().double().requires_grad_(True)
    E64 = E.detach().double().requires_grad_(True)
    yy = y.reshape(-1)
    idx = (yy != 0).nonzero().view(-1)
    n_tok = idx.numel()
    c = 1.0 / n_tok if (reduction == "mean" and n_tok) else 1.0
    hs, N_all = h64.view(-1, h64.shape[-1]), neg.reshape(-1, K)
    lq_all = None if log_q is None else log_q.reshape(-1, K).double()
    losses, ah = [], 0.0
    ae = torch.zeros(E.shape, dtype=torch.float64, device=E.device)
    for i0 in range(0, n_tok, chunk):
        ii = idx[i0:i0 + chunk]
        H, t, N = hs[ii, :d], yy[ii], N_all[ii]
        sp = (H * E64[t]).sum(1)
        sn = torch.einsum("td,tkd->tk", H, E64[N])
        mask = N == 0
        if remove:
            mask = mask | (N == t.unsqueeze(1))
        if objective == "softmax":
            if lq_all is not None:
                sn = sn - lq_all[ii]
            sn = sn.masked_fill(mask, -float("inf"))
            lse = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1)
            lt = lse - sp
        else:
            lt = beta * F.softplus(-sp) + F.softplus(sn).masked_fill(mask, 0.0).sum(1)
        (lt.sum() * c).backward()
        losses.append(lt.detach())
        if with_abs:
            with torch.no_grad():
                if objective == "softmax":
                    P, gp = torch.exp(sn - lse.unsqueeze(1)) * c, (torch.exp(sp - lse) - 1.0).abs() * c
                else:
                    P, gp = torch.sigmoid(sn).masked_fill(mask, 0.0) * c, beta * torch.sigmoid(-sp) * c
                Ha, Ea = H.abs(), E64.abs()
                ah = max(ah, float((torch.einsum("tk,tkd->td", P, Ea[N]) + gp.unsqueeze(1) * Ea[t]).max()))
                ae.index_add_(0, N.reshape(-1), (P.unsqueeze(2) * Ha.unsqueeze(1)).reshape(-1, d))
                ae.index_add_(0, t, gp.unsqueeze(1) * Ha)
    lt = torch.cat(losses) if losses else torch.zeros(0, dtype=torch.float64, device=h.device)
    if reduction == "mean":
        loss = lt.mean()
    elif reduction == "sum":
        loss = lt.sum()
    else:
        loss = torch.zeros(yy.numel(), dtype=torch.float64, device=h.device).index_put((idx,), lt).view(y.shape)
    gh = h64.grad if h64.grad is not None else torch.zeros_like(h64)
    ge = E64.grad if E64.grad is not None else torch.zeros_like(E64)
    if with_abs:
        return loss, gh, ge, ah, float(ae.max())
    return loss, gh, ge


def tneg_mean_loss(hidden, E, pos, neg, log_q, objective, beta, remove=True):
    """the materialised loss in the dtype of its inputs (mean reduction), differentiable"""
    d, K = E.shape[1], neg.shape[-1]
    tok = pos.reshape(-1) != 0
    H, t, N = hidden[..., :d].reshape(-1, d)[tok], pos.reshape(-1)[tok], neg.reshape(-1, K)[tok]
    sp = (H * E[t]).sum(1)
    sn = torch.einsum("td,tkd->tk", H, E[N])
    mask = N == 0
    if remove:
        mask = mask | (N == t.unsqueeze(1))
    if objective == "softmax":
        if log_q is not None:
            sn = sn - log_q.reshape(-1, K)[tok].to(sn.dtype)
        sn = sn.masked_fill(mask, -float("inf"))
        return (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()
    sp_ = torch.nn.functional.softplus
    return (beta * sp_(-sp) + sp_(sn).masked_fill(mask, 0.0).sum(1)).mean()


def sxent_mean_loss(h, E, pos, neg, log_q, remove=True):
    """the materialised sampled softmax over the K shared negatives, mean over the targets, differentiable"""
    _, sp, sn = sxent_logits_ref(h, E, pos, neg, log_q, remove)
    return (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()


def xent_mean_loss(h, E, pos):
    """the materialised full-catalog softmax (items 1 .. n), mean over the targets, differentiable"""
    d = E.shape[1]
    y = pos.reshape(-1)
    hs = h[..., :d].reshape(-1, d)[y != 0]
    return F.cross_entropy(hs @ E[1:].T, y[y != 0] - 1)


# ------------------------------------------------------------------------------------------------ the shared-negative sampler
M32 = 0xFFFFFFFF
SITE_NEG = 0x4E470001           # srfrd_rng.h


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def ref_negatives(seed_word, n_items, K, prob=None, alias=None):
    """ids (K,) int64 that srfrd_shared_negatives draws for the step seed word `seed_word` (state[2]): numpy, integer for
    integer"""
    base = fmix32((int(seed_word) + SITE_NEG * 0x9E3779B9) & M32)
    j = np.arange(K, dtype=np.uint64)
    h1 = fmix32(base ^ j)
    b = (h1 * np.uint64(n_items)) >> np.uint64(32)
    if prob is not None:
        h2 = fmix32(base ^ (j | np.uint64(0x80000000)))
        u = (h2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        b = np.where(u < prob[b.astype(np.int64)], b, alias[b.astype(np.int64)].astype(np.uint64))
    return b.astype(np.int64) + 1


def tneg_token_loss(h, E, y, neg, log_q, remove, objective, beta):
    """the materialised per-token loss (B, L) in the dtype of h / E (fp32 torch: what plain torch arithmetic errs by)"""
    d, K = E.shape[1], neg.shape[-1]
    H, t, N = h[..., :d].reshape(-1, d), y.reshape(-1), neg.reshape(-1, K)
    sp = (H * E[t]).sum(1)
    sn = torch.einsum("td,tkd->tk", H, E[N])
    mask = (N == 0) | (t == 0).unsqueeze(1)
    if remove:
        mask = mask | (N == t.unsqueeze(1))
    if objective == "softmax":
        if log_q is not None:
            sn = sn - log_q.reshape(-1, K).to(sn.dtype)
        lt = torch.logsumexp(torch.cat([sp.unsqueeze(1), sn.masked_fill(mask, -float("inf"))], 1), 1) - sp
    else:
        lt = beta * F.softplus(-sp) + F.softplus(sn).masked_fill(mask, 0.0).sum(1)
    return (lt * (t != 0)).view(y.shape)
