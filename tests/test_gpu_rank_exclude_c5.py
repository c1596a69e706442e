"""-m gpu: C5 geometry (1M items, seq_len 200, B = 512) with 200 excluded ids per user, fp32 table and bf16 shadow:
masked top-10 and target ranks against fp64 scores on the GPU with the excluded entries removed (property check, in
the style of test_c5_size_one_million_items_property)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bf16", [False, True])
def test_c5_exclusion_property(bf16):
    import srfrd_amd
    torch.manual_seed(1)
    I, L, B, k, X = 1_000_000, 200, 512, 10, 200
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    with torch.no_grad():
        m.item_emb.weight.mul_(30.0)
    if bf16:
        m.use_bf16_table()
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=4, device="cuda")
    i0, _ = m.topk(None, seq, None, k=k)
    excl = torch.randint(1, I + 1, (B, X), device="cuda")
    excl[:, :5] = i0[:, :5]                                            # the current winners must go
    ptr_ = torch.arange(0, B * X + 1, X, device="cuda", dtype=torch.int64)
    items = excl.reshape(-1).to(torch.int32)
    idx, val = m.topk(None, seq, None, k=k, exclude=(ptr_, items))
    t = i0[:, 7].clone()
    rank = m.target_rank(None, seq, None, t, exclude=(ptr_, items))
    with torch.no_grad():
        h = m(None, seq, None)[0][:, -1].double()
        table = m.item_emb.weight.to(torch.bfloat16).double() if bf16 else m.item_emb.weight.double()
        scores = h @ table.T
        st = scores.gather(1, t[:, None])
        scores[:, 0] = -float("inf")
        scores.scatter_(1, excl, -float("inf"))
        tv, ti = torch.topk(scores, k + 1, dim=1)
        assert float((val.double() - tv[:, :k]).abs().max()) < 1e-4
        safe = ((tv[:, :-1] - tv[:, 1:]).abs() > 1e-5).all(dim=1)
        assert int(safe.sum()) > B // 2
        assert torch.equal(idx[safe], ti[safe][:, :k])
        scores.scatter_(1, t[:, None], -float("inf"))
        want = (scores > st).sum(1)
        clear = ((scores - st).abs() > 1e-5).all(dim=1)
        assert int(clear.sum()) > B // 2
        assert torch.equal(rank.long()[clear], want[clear])
