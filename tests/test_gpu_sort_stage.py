"""-m gpu: the step program with an eager key sort (srfrd_amd.trainer.step_program(eager_sort=True)) computes, bit for bit, what
the step with the sort inside its one graph and the step without graphs compute.

Tiny shapes run the eager-sort program by building the trainer with trainer.SORT_CAPTURE_LIMIT patched to 0 (a key list of a
few hundred entries); the last three tests run it where it is needed, at the smallest shapes whose list exceeds the limit -
where no tree may capture the sort."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"sasrec50": ("SASRec", 300, 50, 8), "srfrn20": ("SRFRN", 300, 20, 4)}      # kind, items, L, B
TRAINERS = {
    "deterministic": dict(deterministic=True),
    "lazy": dict(lazy_table=True),
    "lazy-cosine": dict(lazy_table=True, lr_schedule="cosine", warmup_steps=2, total_steps=10, final_lr_ratio=0.1),
    "softmax-deterministic": dict(loss="softmax", deterministic=True),
    "sampled-softmax": dict(loss="sampled_softmax", num_negatives=16),
    "token-softmax": dict(loss="token_softmax", num_negatives=5),          # the control: its sort is eager at every size
}
N_BATCHES = 5
_shared = {}


def _new_model(kind, items, L, dropout):
    import srfrd_amd
    if kind == "SRFRN":
        return srfrd_amd.SRFRN(items, L, 45, 5, dropout, 2, 1, "cuda")
    return srfrd_amd.SASRec(items, L, 50, dropout, 2, 1, "cuda")


def _weights(kind, items, L):
    torch.manual_seed(0)
    m = _new_model(kind, items, L, 0.5)
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def _inputs(shape):
    """the shape's initial weights, batches and per-position negatives: made once, read by every test of the shape"""
    if shape not in _shared:
        import srfrd_amd
        kind, items, L, B = SHAPES[shape]
        batches = [srfrd_amd.synthetic_batch(items, L, B, seed=11 + i, device="cuda")[1:] for i in range(N_BATCHES)]
        negs = [srfrd_amd.sample_token_negatives(items, b[2], 5, generator=torch.Generator("cuda").manual_seed(40 + i))
                for i, b in enumerate(batches)]
        _shared[shape] = (_weights(kind, items, L), batches, negs)
    return _shared[shape]


def _trainer(shape_cfg, sd, limit=None, **kw):
    """a trainer in train mode at dropout 0.5 from the weights ``sd``; ``limit``: SORT_CAPTURE_LIMIT while it is built"""
    import srfrd_amd
    from srfrd_amd import trainer
    kind, items, L, B = shape_cfg
    m = _new_model(kind, items, L, 0.5)
    m.load_state_dict(sd)
    with pytest.MonkeyPatch.context() as mp:
        if limit is not None:
            mp.setattr(trainer, "SORT_CAPTURE_LIMIT", limit)
        return srfrd_amd.FusedTrainer(m.to("cuda").train(), B, L, **kw)


def _step(tr, batch, neg):
    if tr.token:
        return tr.step(None, batch[0], batch[1], batch[2], batch[3], neg[0], batch[5], log_q=neg[1])
    return tr.step(None, *batch)


def _fill_slot(tr, slot, batch, neg):
    """what step() leaves in slot 0, into ``slot``"""
    for k, t in enumerate(batch):
        tr.ids_ring[slot][k].copy_(t)
    if tr.token:
        tr.ids_ring[slot][4:].zero_()
        tr.neg_ring[slot].copy_(neg[0])
        tr.log_q_ring[slot].copy_(neg[1])


def _bits(tr):
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (tr.flat, tr.m, tr.v, tr.state)]


def _assert_same(trs, where):
    losses = [float(t.loss) for t in trs]
    assert math.isfinite(losses[0]) and all(x == losses[0] for x in losses), (where, losses)
    ref = _bits(trs[0])
    for t in trs[1:]:
        for name, a, b in zip(("flat", "m", "v", "state"), ref, _bits(t)):
            assert torch.equal(a, b), (where, name)


def _sort_stages(tr):
    return [kind for kind, _, calls in tr._program if "_sort_keys" in calls]


@pytest.mark.parametrize("name", list(TRAINERS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_eager_sort_program_equals_the_captured_sort_and_the_eager_step(shape, name):
    sd, batches, negs = _inputs(shape)
    kw = TRAINERS[name]
    token = kw.get("loss") == "token_softmax"
    cap = _trainer(SHAPES[shape], sd, slots=2, **kw)
    eag = _trainer(SHAPES[shape], sd, limit=0, slots=2, **kw)
    plain = _trainer(SHAPES[shape], sd, use_graph=False, **kw)
    trs = (cap, eag, plain)
    assert cap.n_keys == eag.n_keys == cap.keys.numel() > 0
    assert _sort_stages(eag) == ["eager"] and len(eag._program) == 3
    assert _sort_stages(cap) == (["eager"] if token else [])
    for i in range(3):
        for t in trs:
            _step(t, batches[i], negs[i])
        _assert_same(trs, f"step {i}")
        if i == 0:
            assert cap.graph_form == ("split" if token else "one") and len(cap._graphs[0]) == (3 if token else 1)
            assert eag.graph_form == "split" and len(eag._graphs[0]) == 3 and plain.graph_form is None
            before = _bits(eag)
            eag.spin_up(5)                          # five replays of the two graphs and the sort between them, all put back
            assert all(torch.equal(a, b) for a, b in zip(before, _bits(eag)))
        if i == 1:
            # a state_dict round trip drops the graphs: the next step re-captures the split form and continues
            eag.load_state_dict(eag.state_dict())
            assert not eag.captured
    assert eag.captured and eag.graph_form == "split" and eag.graph_capture_error is None
    # the input ring: slot 1, then slot 0, against the same batches through step()
    _fill_slot(eag, 1, batches[3], negs[3])
    _fill_slot(eag, 0, batches[4], negs[4])
    eag.step_slot(1)
    _step(cap, batches[3], negs[3])
    _assert_same((cap, eag), "slot 1")
    eag.step_slot(0)
    _step(cap, batches[4], negs[4])
    _assert_same((cap, eag), "slot 0")
    for t in (cap, plain):
        t.check()


def test_an_unsorted_trainer_has_no_key_list_and_stays_one_graph():
    sd, batches, negs = _inputs("sasrec50")
    for kw in (dict(), dict(loss="softmax")):
        tr = _trainer(SHAPES["sasrec50"], sd, limit=0, **kw)
        assert tr.n_keys == 0 and tr.keys is None and tr.skeys is None and tr.order is None
        assert len(tr._program) == 1 and _sort_stages(tr) == []


# ---- the real thing: the smallest lists above the limit ---------------------------------------------------------------------------
def _over_limit(B, **kw):
    """SASRec 50, 2000 items (long runs per item), L = 50: one step of the graph form against the step without graphs"""
    import srfrd_amd
    from srfrd_amd.trainer import SORT_CAPTURE_LIMIT
    cfg = ("SASRec", 2000, 50, B)
    sd = _weights(*cfg[:3])
    batch = srfrd_amd.synthetic_batch(2000, 50, B, seed=1, device="cuda")[1:]
    g, e = _trainer(cfg, sd, **kw), _trainer(cfg, sd, use_graph=False, **kw)
    # before the first step: the list is over the limit, and the program sorts it in an eager stage between two graphs
    assert g.n_keys > SORT_CAPTURE_LIMIT
    assert [(kind, calls) for kind, _, calls in g._program][1] == ("eager", ("_sort_keys",)) and _sort_stages(g) == ["eager"]
    assert g.use_graph and [kind for kind, _, _ in g._program] == ["graph", "eager", "graph"]
    lg, le = float(g.step(None, *batch)), float(e.step(None, *batch))
    assert g.captured and g.graph_form == "split"
    assert math.isfinite(lg) and lg == le, (lg, le)
    for name, a, b in zip(("flat", "m", "v"), _bits(g), _bits(e)):
        assert torch.equal(a, b), name
    g.check()
    return g


def test_over_limit_deterministic():
    assert _over_limit(7000, deterministic=True).n_keys == 1_050_000


def test_over_limit_lazy_table():
    assert _over_limit(7000, lazy_table=True).n_keys == 1_050_000


def test_over_limit_sampled_softmax():
    assert _over_limit(10_500, loss="sampled_softmax", num_negatives=64).n_keys == 1_050_064
