"""-m gpu: the six library ops of the loss heads (torch.ops.srfrd.{xent,sxent,tneg}_{fwd,bwd}) against the model methods
(full_catalog_loss, sampled_softmax_loss, token_negatives_loss).  Both go through srfrd_amd/loss_heads.py, the ops under
torch.library's registered autograd and the methods under their own autograd function, so every comparison is bitwise.
B, L, K and n_items are pairwise distinct, and SRFRN has d_out != d_item: a swapped argument cannot pass."""
import pytest
import torch

from tests.loss_refs import head_model, head_table, make_inputs, run_head, shared_negatives

pytestmark = pytest.mark.gpu

B, L, K, N_ITEMS = 4, 20, 9, 500
CASES = [(head, kind) for head in ("xent", "sxent", "tneg-softmax", "tneg-gbce") for kind in ("SASRec", "SRFRN")
         if (head, kind) != ("tneg-gbce", "SRFRN")]                      # gBCE refuses SRFRN


@pytest.mark.parametrize("head, kind", CASES)
def test_library_ops_match_the_method(head, kind):
    from srfrd_amd import ops
    torch.manual_seed(6)
    m = head_model(*((50, 0) if kind == "SASRec" else (45, 5)), N_ITEMS, L)
    table, key = head_table(m), ops.register_model(m)
    h = torch.randn(B, L, m.layout.d_out, device="cuda") * 0.5
    y, neg = make_inputs(B, L, K, N_ITEMS, 2, empty_rows=())
    assert bool((y == 0).any()) and bool((y != 0).any())
    if head == "xent":
        def method(hh, red):
            return m.full_catalog_loss(hh, y, red)

        def op(hh):
            return torch.ops.srfrd.xent_fwd(hh, y, table, key)
    elif head == "sxent":
        neg = shared_negatives(K, N_ITEMS, y, 2).cuda()
        log_q = (torch.randn(K) * 2.0).cuda()

        def method(hh, red):
            return m.sampled_softmax_loss(hh, y, neg, log_q, True, red)

        def op(hh):
            return torch.ops.srfrd.sxent_fwd(hh, y, neg, log_q, table, True, key)
    else:
        objective = head.split("-")[1]
        code = {"softmax": 0, "gbce": 1}[objective]
        neg = neg.cuda()
        log_q = (torch.randn(B, L, K) * 2.0).cuda() if objective == "softmax" else None

        def method(hh, red):
            return m.token_negatives_loss(hh, y, neg, objective, log_q, 0.6, True, red)

        def op(hh):
            return torch.ops.srfrd.tneg_fwd(hh, y, neg, log_q, table, code, 0.6, True, key)
    y = y.cuda()
    want = {red: run_head(m, lambda hh: method(hh, red), h) for red in ("sum", "none", "mean")}
    table.grad = None
    hh = h.clone().requires_grad_(True)
    tl, lse, stats = op(hh)
    tl.sum().backward()
    assert torch.equal(stats[0], want["sum"][0])
    assert torch.equal(stats[1], (y != 0).sum().to(torch.float32))
    assert torch.equal(tl.detach(), want["none"][0])
    assert torch.equal(want["mean"][0], stats[0] / stats[1])
    for red in ("sum", "none"):                         # d token loss = 1 everywhere, as tl.sum() gives
        assert torch.equal(hh.grad, want[red][1]) and torch.equal(table.grad, want[red][2]), red
