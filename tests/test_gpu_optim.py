"""-m gpu: srfrd_amd.Adam - torch.optim.Adam's update (reference trainer.py:390) as one launch over the model's flat parameter
vector, for the module-level drop-in loop (trainer.py:29-41 unchanged but for the optimizer's constructor)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(kind="SASRec"):
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(400, 50, 50, 0.0, 2, 1, "cuda") if kind == "SASRec" else srfrd_amd.SRFRN(400, 50, 45, 5, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _close(sd1, sd2, D=50):
    """same gradients up to float-atomic order in the item table => same Adam steps, except where a gradient is rounding
    noise and its SIGN decides the step (tests/helpers.drop_kbias; a handful of near-zero table elements)"""
    from tests.helpers import drop_kbias
    for k in sd1:
        d = (drop_kbias(k, sd1[k].cpu(), D) - drop_kbias(k, sd2[k].cpu(), D)).abs()
        assert float(d.mean()) < 5e-7 and float((d > 2e-5).float().mean()) < 2e-3 and float(d.max()) < 1e-2, (k, float(d.max()), float(d.mean()))


def _step(m, opt, batch):
    u, seq, rsq, pos, prs, neg, nrs = batch
    h, pl, nl = m(u, seq, rsq, pos, prs, neg, nrs)
    idx = torch.where(pos != 0)
    crit = torch.nn.BCEWithLogitsLoss()
    loss = crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_flat_adam_equals_torch_adam_and_exchanges_state(kind):
    import srfrd_amd
    m1 = _model(kind)
    m2 = copy.deepcopy(m1)
    o1 = srfrd_amd.Adam(m1.parameters(), lr=1e-3, betas=(0.9, 0.98))
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, betas=(0.9, 0.98))
    batches = [srfrd_amd.synthetic_batch(400, 50, 24, seed=3, index=i, device="cuda") for i in range(4)]
    for i in range(3):
        l1, l2 = _step(m1, o1, batches[i]), _step(m2, o2, batches[i])
        assert abs(l1 - l2) < 1e-5
    assert o1._gbuf is None                        # every step took the one in-place launch (no gradient gather)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    _close(sd1, sd2)
    # state in torch.optim.Adam's own format, both directions
    s1, s2 = o1.state_dict(), o2.state_dict()
    assert s1["param_groups"][0]["params"] == s2["param_groups"][0]["params"]
    for i in s2["state"]:
        assert float(s1["state"][i]["step"]) == float(s2["state"][i]["step"]) == 3.0
        assert float((s1["state"][i]["exp_avg"] - s2["state"][i]["exp_avg"]).abs().max()) < 1e-5
        assert float((s1["state"][i]["exp_avg_sq"] - s2["state"][i]["exp_avg_sq"]).abs().max()) < 1e-7
    o3 = srfrd_amd.Adam(m2.parameters(), lr=1e-3, betas=(0.9, 0.98))
    o3.load_state_dict(s2)                         # torch's state into the flat optimizer: the fourth step continues it
    o2b = torch.optim.Adam(m1.parameters(), lr=1e-3, betas=(0.9, 0.98))
    o2b.load_state_dict(s1)                        # ... and the flat optimizer's state into torch's
    l1, l2 = _step(m1, o2b, batches[3]), _step(m2, o3, batches[3])
    assert abs(l1 - l2) < 1e-5
    _close(m1.state_dict(), m2.state_dict())


def test_flat_adam_takes_gradients_that_are_not_views_of_one_vector():
    """two backward calls accumulate into .grad (torch then owns separate tensors): the optimizer gathers them"""
    import srfrd_amd
    m1 = _model()
    m2 = copy.deepcopy(m1)
    o1 = srfrd_amd.Adam(m1.parameters(), lr=1e-3, betas=(0.9, 0.98))
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, betas=(0.9, 0.98))
    b = [srfrd_amd.synthetic_batch(400, 50, 16, seed=5, index=i, device="cuda") for i in range(2)]
    for m, o in ((m1, o1), (m2, o2)):
        o.zero_grad()
        for u, seq, rsq, pos, prs, neg, nrs in b:
            h, pl, nl = m(u, seq, rsq, pos, prs, neg, nrs)
            (pl.sum() * 1e-3 - nl.sum() * 1e-3).backward()
        o.step()
    _close(m1.state_dict(), m2.state_dict())


def test_replaced_parameters_and_submodules_are_picked_up_by_the_next_forward():
    """forward() resolves its parameter slots through cached module paths (srfrd_amd/modules.py:_current_slots): a parameter
    object or a whole submodule replaced between two calls must be what the next call computes with - checked against a fresh
    model loaded from the modified model's state_dict (bit-equal outputs), and training must go on from there."""
    import srfrd_amd
    m = _model().eval()
    batch = srfrd_amd.synthetic_batch(400, 50, 32, seed=5, device="cuda")
    u, seq, rsq, pos, prs, neg, nrs = batch
    with torch.no_grad():
        h0 = m(u, seq, rsq, pos, prs, neg, nrs)[0].clone()
        # (a) a new Parameter object in place of an old one
        m.last_layernorm.weight = torch.nn.Parameter(torch.full((50,), 1.5, device="cuda"))
        # (b) a whole submodule replaced
        ln = torch.nn.LayerNorm(50, eps=1e-8).cuda()
        ln.weight.data.uniform_(0.5, 1.5)
        m.attention_layernorms[1] = ln
        # (c) in-place edits of an existing parameter
        m.pos_emb.weight.data.mul_(0.5)
        h1 = m(u, seq, rsq, pos, prs, neg, nrs)[0].clone()
    assert float((h1 - h0).abs().max()) > 1e-3
    ref = _model().eval()
    ref.load_state_dict(m.state_dict())
    with torch.no_grad():
        h2 = ref(u, seq, rsq, pos, prs, neg, nrs)[0]
    assert torch.equal(h1, h2)
    # every parameter is a view of the (re-built) flat vector again, and the optimizer steps the new objects
    m.train()
    opt = srfrd_amd.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.98))
    before = m.last_layernorm.weight.detach().clone()
    _step(m, opt, batch)
    assert float((m.last_layernorm.weight.detach() - before).abs().max()) > 0
    base = m.flat_parameters().data_ptr()
    assert all(base <= p.data_ptr() < base + 4 * m.flat_parameters().numel() for p in m.parameters())


@pytest.mark.parametrize("frozen", ["item_emb.weight", "attention_layers.1.in_proj_weight", "last_layernorm.bias"])
def test_filtered_parameter_list_leaves_frozen_tensors_alone(frozen):
    """Adam([p for p in m.parameters() if p.requires_grad]): the backward still writes every gradient into the one flat
    gradient vector, but a tensor left out of the list must neither move nor get state - as with torch.optim.Adam.  The last
    one, last_layernorm.bias, starts 2 elements into a float4 at the end of the vector."""
    import srfrd_amd
    m1 = _model()
    m2 = copy.deepcopy(m1)
    for m in (m1, m2):
        dict(m.named_parameters())[frozen].requires_grad_(False)
    o1 = srfrd_amd.Adam([p for p in m1.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98))
    o2 = torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3, betas=(0.9, 0.98))
    before = dict(m1.named_parameters())[frozen].detach().clone()
    batches = [srfrd_amd.synthetic_batch(400, 50, 24, seed=4, index=i, device="cuda") for i in range(2)]
    for b in batches:
        assert abs(_step(m1, o1, b) - _step(m2, o2, b)) < 1e-5
    assert torch.equal(dict(m1.named_parameters())[frozen].detach(), before)
    s1, s2 = o1.state_dict(), o2.state_dict()
    assert sorted(s1["state"]) == sorted(s2["state"]) and len(s1["state"]) == len(list(m1.parameters())) - 1
    _close(m1.state_dict(), m2.state_dict())


def test_listed_parameter_without_gradient_keeps_value_and_moments():
    """a listed parameter whose .grad is None is skipped, however large its (loaded) moments - torch.optim.Adam's rule"""
    import srfrd_amd
    m1 = _model()
    m2 = copy.deepcopy(m1)
    o1 = srfrd_amd.Adam(m1.parameters(), lr=1e-3, betas=(0.9, 0.98))
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, betas=(0.9, 0.98))
    batches = [srfrd_amd.synthetic_batch(400, 50, 24, seed=6, index=i, device="cuda") for i in range(2)]
    _step(m2, o2, batches[0])
    _step(m1, o1, batches[0])
    o1.load_state_dict(o2.state_dict())                # non-zero moments for every parameter
    names = [k for k, _ in m1.named_parameters()]
    j = names.index("last_layernorm.weight")
    p1, p2 = dict(m1.named_parameters())["last_layernorm.weight"], dict(m2.named_parameters())["last_layernorm.weight"]
    with torch.no_grad():
        p1.copy_(p2)
    m_before = o1.state_dict()["state"][j]["exp_avg"].clone()
    v_before = o1.state_dict()["state"][j]["exp_avg_sq"].clone()
    assert float(m_before.abs().max()) > 0
    w_before = p1.detach().clone()
    for m, o in ((m1, o1), (m2, o2)):
        u, seq, rsq, pos, prs, neg, nrs = batches[1]
        h, pl, nl = m(u, seq, rsq, pos, prs, neg, nrs)
        o.zero_grad()
        (pl.sum() * 1e-3 - nl.sum() * 1e-3).backward()
        dict(m.named_parameters())["last_layernorm.weight"].grad = None
        o.step()
    assert torch.equal(p1.detach(), w_before) and torch.equal(p2.detach(), w_before)
    s1, s2 = o1.state_dict(), o2.state_dict()
    assert torch.equal(s1["state"][j]["exp_avg"], m_before) and torch.equal(s1["state"][j]["exp_avg_sq"], v_before)
    _close(m1.state_dict(), m2.state_dict())
    # torch's per-parameter step counts: the skipped parameter is one behind, in both state dicts, and the next step corrects
    # its bias with its own count (a second launch); the states still move between the two optimizers
    assert sorted(s1["state"]) == sorted(s2["state"])
    for i in s2["state"]:
        assert float(s1["state"][i]["step"]) == float(s2["state"][i]["step"]) == (1.0 if i == j else 2.0)
    o1.load_state_dict(s2)
    o2.load_state_dict(s1)
    assert abs(_step(m1, o1, batches[0]) - _step(m2, o2, batches[0])) < 1e-5
    _close(m1.state_dict(), m2.state_dict())
    s1, s2 = o1.state_dict(), o2.state_dict()
    for i in s2["state"]:
        assert float(s1["state"][i]["step"]) == float(s2["state"][i]["step"]) == (2.0 if i == j else 3.0)
        assert float((s1["state"][i]["exp_avg"] - s2["state"][i]["exp_avg"]).abs().max()) < 1e-5


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_load_state_dict_before_the_first_forward(kind):
    """the usual resume order - build the model and the optimizer, load both state dicts, then train - continues torch's run"""
    import srfrd_amd
    m2 = _model(kind)
    o2 = torch.optim.Adam(m2.parameters(), lr=1e-3, betas=(0.9, 0.98))
    batches = [srfrd_amd.synthetic_batch(400, 50, 24, seed=3, index=i, device="cuda") for i in range(4)]
    for i in range(3):
        _step(m2, o2, batches[i])
    torch.manual_seed(1)
    m3 = (srfrd_amd.SASRec(400, 50, 50, 0.0, 2, 1, "cuda") if kind == "SASRec"
          else srfrd_amd.SRFRN(400, 50, 45, 5, 0.0, 2, 1, "cuda")).cuda().train()
    o3 = srfrd_amd.Adam(m3.parameters(), lr=1e-3, betas=(0.9, 0.98))
    m3.load_state_dict(m2.state_dict())
    o3.load_state_dict(o2.state_dict())                # before any forward of m3
    s3 = o3.state_dict()
    assert float(s3["state"][0]["step"]) == 3.0
    l3, l2 = _step(m3, o3, batches[3]), _step(m2, o2, batches[3])
    assert abs(l3 - l2) < 1e-5
    _close(m3.state_dict(), m2.state_dict())
    s3, s2 = o3.state_dict(), o2.state_dict()
    for i in s2["state"]:
        assert float(s3["state"][i]["step"]) == float(s2["state"][i]["step"]) == 4.0
        assert float((s3["state"][i]["exp_avg"] - s2["state"][i]["exp_avg"]).abs().max()) < 1e-5
