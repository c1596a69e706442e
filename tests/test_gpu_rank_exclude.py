"""-m gpu: full-catalog ranking with per-user exclusion sets (srfrd_logits_topk_excl) and exact target ranks
(srfrd_target_rank) on every kernel route, against the GPU's own scores in fp64 with the excluded entries removed."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (kind, item width, bf16 shadow, SRFRD_TOPK_FP32): the 16-wide fp32 path (three bf16 planes), the fp32 stream (forced, and
# hidden 64 > 52), the bf16 shadow (even and odd width), SRFRN with its user-label channel
ROUTES = [("SASRec", 50, False, False), ("SRFR", 45, False, False), ("SASRec", 50, False, True), ("SASRec", 64, False, False),
          ("SASRec", 50, True, False), ("SASRec", 51, True, False), ("SRFRN", 45, False, False)]


def _model(kind, width, bf16, I, L, seed=3):
    import srfrd_amd
    torch.manual_seed(seed)
    if kind == "SASRec":
        m = srfrd_amd.SASRec(I, L, width, 0.0, 2, 1, "cuda")
    else:
        m = getattr(srfrd_amd, kind)(I, L, width, 5, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    with torch.no_grad():
        m._item_param().mul_(6.0)
    if bf16:
        m.use_bf16_table()
    return m


def _batch(I, L, B, seed):
    import srfrd_amd
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=seed, device="cuda")
    return seq, rsq


def _scores(m, seq, rsq, I):
    """(B, I + 1) fp64 scores of every item (the predict kernel: one fp32 dot product per (user, item)).  The tests of this
    file trust these; _check_predict_chain holds them to the host's fp64 scores of the same hidden states, and
    tests/test_gpu_rank_widths.py pins predict_logits itself at every width."""
    with torch.no_grad():
        s = m.predict(None, seq, rsq, torch.arange(I + 1, device="cuda")).double().reshape(seq.shape[0], I + 1)
    _check_predict_chain(m, seq, rsq, s)
    return s


def _check_predict_chain(m, seq, rsq, s):
    """the predict-derived scores agree with scores64 of tests/rank_refs.py (fp64 on the host from the encoder's last hidden
    state and the table the kernels read) within that file's value bound, 4 max(E32, 2^-23) A"""
    from tests import rank_refs as R
    with torch.no_grad():
        ids = m._prep(seq, rsq, None, None, None, None)
        hidden = m._launch_fwd_last(ids[0], ids[1]).cpu()
        rows, d = m.layout.n_items + 1, m.layout.d_item
        if m.bf16_table:
            table = ((m._table16.cpu().to(torch.int32) & 0xFFFF) << 16).view(torch.float32).reshape(rows, d)
        else:
            table = m._item_param().detach().cpu()
        side = None
        if m._kind == "SRFRN":
            side = (m.embedding_layer.fake_embed.weight.detach().cpu(), m.user_labels(ids[1]).cpu().clamp(0, 2))
    ref = R.Ref(hidden, table, side)
    assert (np.abs(s.cpu().numpy() - ref.s) <= ref.eps * ref.A).all()


def _mask(scores, rows, exclude_pad=True):
    s = scores.clone()
    for b, r in enumerate(rows):
        r = torch.as_tensor(r, dtype=torch.int64)
        r = r[(r >= 0) & (r < s.shape[1])]
        s[b, r.cuda()] = -float("inf")
    if exclude_pad:
        s[:, 0] = -float("inf")
    return s


def _check_topk(idx, val, ref, k):
    tv, ti = torch.topk(ref, k + 1, dim=1)
    fin = torch.isfinite(tv[:, :k])
    assert torch.equal(torch.isfinite(val), fin)
    assert float((val.double()[fin] - tv[:, :k][fin]).abs().max()) < 1e-4
    safe = ((tv[:, :-1] - tv[:, 1:]).abs() > 1e-5).all(dim=1)        # users whose order fp32 rounding cannot change
    assert int(safe.sum()) > idx.shape[0] // 2
    assert torch.equal(idx[safe], ti[safe][:, :k])


def _rows(seq, I, B, gen, extra):
    """per user: the input window, the current top items (so the mask matters), and noise - 0, duplicates, unsorted ids,
    ids outside the catalog"""
    rows = []
    for b in range(B):
        r = seq[b].cpu()
        r = r[r != 0].tolist() + extra[b].tolist() + [0, -5, I + 7, 10 * I]
        r += r[:3]
        r += torch.randint(1, I + 1, (20,), generator=gen).tolist()
        rows.append(torch.tensor(r)[torch.randperm(len(r), generator=gen)])
    return rows


@pytest.mark.parametrize("kind,width,bf16,fp32", ROUTES)
def test_topk_with_exclusion_matches_fp64_on_every_route(kind, width, bf16, fp32, monkeypatch):
    if fp32:
        monkeypatch.setenv("SRFRD_TOPK_FP32", "1")
    I, L, B, k = 20_000, 20, 40, 10
    m = _model(kind, width, bf16, I, L)
    seq, rsq = _batch(I, L, B, 5)
    i0, _ = m.topk(None, seq, rsq, k=k)
    gen = torch.Generator().manual_seed(1)
    rows = _rows(seq, I, B, gen, i0[:, :3].cpu())
    idx, val = m.topk(None, seq, rsq, k=k, exclude=rows)
    _check_topk(idx, val, _mask(_scores(m, seq, rsq, I), rows), k)
    assert not (idx == i0[:, :1]).any()                               # every user's old winner is gone
    # "input": the ids of each user's window
    idx, val = m.topk(None, seq, rsq, k=k, exclude="input")
    _check_topk(idx, val, _mask(_scores(m, seq, rsq, I), [s[s != 0].cpu() for s in seq]), k)


@pytest.mark.parametrize("kind,width,bf16,fp32", [ROUTES[0], ROUTES[2], ROUTES[4]])
def test_exhaustive_fallback_masks_too(kind, width, bf16, fp32, monkeypatch):
    """mass ties overflow the candidate lists and arm the exhaustive path: it must mask the same items"""
    if fp32:
        monkeypatch.setenv("SRFRD_TOPK_FP32", "1")
    I, L, B, k = 6000, 20, 24, 10
    m = _model(kind, width, False, I, L)
    with torch.no_grad():
        m._item_param()[1:5001] = m._item_param()[7:8]            # 5000 bit-identical rows: > 2048 candidates tie
    if bf16:
        m.use_bf16_table()
    seq, rsq = _batch(I, L, B, 6)
    rows = [torch.tensor([7, 1, 2, 3, 4000, 4999] + list(range(100 + b, 200 + b))) for b in range(B)]
    idx, val = m.topk(None, seq, rsq, k=k, exclude=rows)
    ref = _mask(_scores(m, seq, rsq, I), rows)
    for b in range(B):
        # stable order over the masked scores: value desc, id asc (exact ties among the identical rows)
        s = ref[b].cpu().numpy()
        order = np.lexsort((np.arange(s.size), -s))[:k]
        tied = np.isclose(s[order], s[order[0]], rtol=0, atol=1e-5).all()
        if tied:
            assert idx[b].tolist() == order.tolist()
    assert not any(set(idx[b].tolist()) & set(rows[b].tolist()) for b in range(B))


def test_exclusion_edge_cases():
    from srfrd_amd import _lib
    I, L, B, k = 3000, 20, 6, 10
    m = _model("SASRec", 50, False, I, L)
    seq, rsq = _batch(I, L, B, 7)
    ref = _scores(m, seq, rsq, I)
    everything = torch.arange(0, I + 1)
    keep = torch.tensor([17, 1200, 2999, 3000, 256])
    rows = [torch.tensor([], dtype=torch.int64),                                   # empty
            torch.tensor([0, 0, 5, 5, 5, -1, I + 1, 2 ** 31 - 1, 9, 1]),            # 0, duplicates, out of range, unsorted
            everything[~torch.isin(everything, keep)].flip(0),                      # all but 5 items: 5 trailing -1 / -inf
            torch.randint(1, I + 1, (_lib.EXCL_CAP,)),                               # a row at the cap (with duplicates)
            torch.tensor([], dtype=torch.int64),
            torch.arange(1, 300)]
    idx, val = m.topk(None, seq, rsq, k=k, exclude=rows)
    masked = _mask(ref, rows)
    tv, ti = torch.topk(masked, k, dim=1)
    assert idx[2, 5:].tolist() == [-1] * 5 and bool(torch.isneginf(val[2, 5:]).all())
    assert sorted(idx[2, :5].tolist()) == sorted(keep.tolist())
    for b in (0, 1, 3, 4, 5):
        assert set(idx[b].tolist()) == set(ti[b].tolist()) or float((val[b].double() - tv[b]).abs().max()) < 1e-4
        assert not (set(idx[b].tolist()) & set(rows[b].tolist()) - {0})
    # the empty rows equal the unmasked ranking
    i0, v0 = m.topk(None, seq, rsq, k=k)
    assert torch.equal(idx[0], i0[0]) and torch.equal(idx[4], i0[4])
    # one id over the cap: SRFRD_E_UNSUPPORTED, not a wrong answer
    rows[3] = torch.randint(1, I + 1, (_lib.EXCL_CAP + 1,))
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        m.topk(None, seq, rsq, k=k, exclude=rows)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        m.target_rank(None, seq, rsq, torch.ones(B, dtype=torch.int64), exclude=rows)


@pytest.mark.parametrize("bf16", [False, True])
def test_mask_equals_removal(bf16):
    """exclude=None and all-empty sets are bit-equal to the existing topk; excluding a set equals ranking a table whose
    excluded rows were moved past a reduced item_hi (ids mapped back)"""
    import srfrd_amd
    I, L, B, k = 9000, 20, 33, 10
    m = _model("SASRec", 50, bf16, I, L)
    seq, _ = _batch(I, L, B, 8)
    i0, v0 = m.topk(None, seq, None, k=k)
    i1, v1 = m.topk(None, seq, None, k=k, exclude=None)
    i2, v2 = m.topk(None, seq, None, k=k, exclude=[torch.tensor([], dtype=torch.int64)] * B)
    assert torch.equal(i0, i1) and torch.equal(v0, v1) and torch.equal(i0, i2) and torch.equal(v0, v2)
    gen = torch.Generator().manual_seed(4)
    S = torch.unique(torch.cat([i0[:, :4].cpu().reshape(-1), torch.randint(1, I + 1, (300,), generator=gen)]))
    ix, vx = m.topk(None, seq, None, k=k, exclude=[S] * B)
    rest = torch.tensor([i for i in range(I + 1) if i not in set(S.tolist())])
    perm = torch.cat([rest, S])                                         # new row j holds old row perm[j]
    m2 = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda").cuda().eval()
    sd = {kk: v.clone() for kk, v in m.state_dict().items()}
    sd["item_emb.weight"] = sd["item_emb.weight"][perm.cuda()]
    m2.load_state_dict(sd)
    if bf16:
        m2.use_bf16_table()
    seq2 = torch.argsort(perm.cuda())[seq]                              # the same windows in new ids
    ir, vr = m2.topk(None, seq2, None, k=k, item_range=(0, rest.numel()))
    assert torch.equal(vx, vr)
    assert torch.equal(ix, perm.cuda()[ir])


@pytest.mark.parametrize("kind,width,bf16,fp32", ROUTES)
def test_target_rank_counts(kind, width, bf16, fp32, monkeypatch):
    if fp32:
        monkeypatch.setenv("SRFRD_TOPK_FP32", "1")
    I, L, B, k = 20_000, 20, 40, 10
    m = _model(kind, width, bf16, I, L)
    seq, rsq = _batch(I, L, B, 9)
    i0, _ = m.topk(None, seq, rsq, k=k, exclude="input")
    t = i0[:, 3].clone()                                               # some targets inside the top k ...
    t[::3] = torch.randint(1, I + 1, (t[::3].numel(),), device="cuda")  # ... and some anywhere
    rank = m.target_rank(None, seq, rsq, t, exclude="input")
    assert rank.dtype == torch.int32 and rank.shape == (B,)
    ref = _mask(_scores(m, seq, rsq, I), [s[s != 0].cpu() for s in seq])
    st = _scores(m, seq, rsq, I).gather(1, t[:, None]).double()
    others = ref.clone()
    others.scatter_(1, t[:, None], -float("inf"))
    want = (others > st).sum(1)
    clear = ((others - st).abs() > 1e-5).all(dim=1)
    assert int(clear.sum()) > B // 2
    assert torch.equal(rank.long()[clear], want[clear])
    # consistency with top-k: where the list has no ties, the target sits at its rank
    iv, vv = m.topk(None, seq, rsq, k=k, exclude="input")
    for b in range(B):
        r = int(rank[b])
        vals = vv[b].tolist()
        if r < k and len(set(vals)) == k:
            assert int(iv[b, r]) == int(t[b])
    # the target is ranked even inside its own exclusion set
    own = [torch.cat([s[s != 0].cpu(), t[b:b + 1].cpu()]) for b, s in enumerate(seq)]
    assert torch.equal(m.target_rank(None, seq, rsq, t, exclude=own), rank)


@pytest.mark.parametrize("kind,width,bf16,fp32", [ROUTES[0], ROUTES[2], ROUTES[4], ROUTES[6]])
def test_duplicates_of_the_target_tie(kind, width, bf16, fp32, monkeypatch):
    """bit-identical copies of the target's row in other chunks and other lanes score exactly s_t and are never counted"""
    if fp32:
        monkeypatch.setenv("SRFRD_TOPK_FP32", "1")
    I, L, B = 20_000, 20, 40
    m = _model(kind, width, False, I, L)
    tgt = 777
    dups = [5, 300, 301, 778, 1023, 2047, 2500, 13_001, 19_999]
    with torch.no_grad():
        m._item_param()[dups] = m._item_param()[tgt].clone()
    if bf16:
        m.use_bf16_table()
    seq, rsq = _batch(I, L, B, 10)
    t = torch.full((B,), tgt, dtype=torch.int64, device="cuda")
    r_plain = m.target_rank(None, seq, rsq, t)
    r_without = m.target_rank(None, seq, rsq, t, exclude=[torch.tensor(dups)] * B)
    assert torch.equal(r_plain, r_without)
    # and the copies as targets rank the same
    for d in (5, 2047, 19_999):
        assert torch.equal(m.target_rank(None, seq, rsq, torch.full_like(t, d)), r_plain)


@pytest.mark.parametrize("n_shards", [3, 8])
@pytest.mark.parametrize("bf16", [False, True])
def test_shards_equal_unsharded(n_shards, bf16):
    import srfrd_amd
    I, L, B, k = 12_000, 20, 37, 10
    m = _model("SASRec", 50, bf16, I, L)
    seq, _ = _batch(I, L, B, 11)
    gen = torch.Generator().manual_seed(2)
    rows = [torch.randint(0, I + 1, (int(n),), generator=gen) for n in torch.randint(0, 400, (B,), generator=gen)]
    wi, wv = m.topk(None, seq, None, k=k, exclude=rows)
    t = torch.randint(1, I + 1, (B,), device="cuda")
    wr = m.target_rank(None, seq, None, t, exclude=rows)
    r = srfrd_amd.ShardedRanker(m, n_shards=n_shards)
    si, sv = r.topk(None, seq, None, k=k, exclude=rows)
    assert torch.equal(si, wi) and torch.equal(sv, wv)
    assert torch.equal(r.target_rank(None, seq, None, t, exclude=rows), wr)


def test_full_catalog_evaluation_matches_fp64():
    """evaluation(full_catalog=True): the held-out item ranked against every item outside set(train[u]) | {0}"""
    import srfrd_amd
    from srfrd_amd.dataset import InteractionData, eval_inputs
    rng = np.random.RandomState(0)
    U, I, L = 300, 4000, 20
    lens = rng.randint(1, 60, U + 1)
    lens[0] = 0
    ptr_ = np.zeros(U + 2, np.int64)
    np.cumsum(lens, out=ptr_[1:U + 2])
    items = rng.randint(1, I + 1, int(ptr_[-1])).astype(np.int32)
    reviews = rng.randint(1, 3, items.size).astype(np.int32)
    test_item = rng.randint(1, I + 1, U + 1).astype(np.int32)
    test_item[0] = 0
    data = InteractionData(U, I, ptr_, items, reviews, test_item, rng.randint(1, 3, U + 1).astype(np.int32))
    m = _model("SRFR", 45, False, I, L)
    ndcg, hr = srfrd_amd.evaluation(m, data, L, full_catalog=True, k=10, batch=128)
    uid, seq, rsq, _ = eval_inputs(data, L, 0, 0)
    seq, rsq = seq.cuda(), rsq.cuda()
    sc = _scores(m, seq, rsq, I)
    rated = [items[ptr_[u]:ptr_[u + 1]] for u in uid.tolist()]
    ref = _mask(sc, [torch.from_numpy(r.astype(np.int64)) for r in rated])
    t = torch.from_numpy(test_item[uid.numpy()].astype(np.int64)).cuda()
    st = sc.gather(1, t[:, None])
    ref.scatter_(1, t[:, None], -float("inf"))
    want = (ref > st).sum(1)
    clear = ((ref - st).abs() > 1e-5).all(dim=1)
    assert float(clear.double().mean()) > 0.9
    ndcg_u = torch.where(want < 10, 1.0 / torch.log2(want.double() + 2.0), torch.zeros_like(want, dtype=torch.float64))
    lo_n = float(ndcg_u[clear].sum()) / want.numel()
    # near-tie users are bounded: they contribute between 0 and their best case
    hi_n = lo_n + float((~clear).sum()) / want.numel()
    assert lo_n - 1e-12 <= ndcg <= hi_n + 1e-12
    hit_lo = float((want[clear] < 10).sum()) / want.numel()
    assert hit_lo - 1e-12 <= hr <= hit_lo + float((~clear).sum()) / want.numel() + 1e-12
    if bool(clear.all()):
        assert abs(ndcg - float(ndcg_u.mean())) < 1e-12 and abs(hr - float((want < 10).double().mean())) < 1e-12
    out = srfrd_amd.evaluation(m, data, L, full_catalog=True, k=10, batch=128, with_labels=True)
    assert out[0] == ndcg and out[1] == hr and len(out) == 6
    # per user: the evaluation's rank equals the fp64 count wherever no score is within 1e-5 of the target's
    got = torch.tensor([out[2][int(u)][0] for u in uid.tolist()], device="cuda")
    assert torch.equal(got[clear], want[clear])
