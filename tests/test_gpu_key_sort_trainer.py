"""-m gpu: ``FusedTrainer(key_sort="device")`` against ``key_sort="torch"``, in bits.

A stable sort has one correct output, so the two trainers - same weights, same seed, same batches - must agree bit for bit after
every step: parameters, both moments, the loss, and the sorted key list itself.  Token losses at K 1 / 5 / 65 with and without
graphs (one graph per step under "device", two around the eager sort under "torch"), the sampled softmax, the deterministic and
the lazy BCE step on the generic kernels and on the train kernel, a batch with an invalid id, checkpoints moving both ways, and
one C2-size token step (1 689 600 keys) as one captured graph.  There is no tolerance in this file."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

ITEMS = 300
_shared = {}


def _new_model(items, L, dropout=0.5):
    import srfrd_amd
    return srfrd_amd.SASRec(items, L, 50, dropout, 2, 1, "cuda")


def _weights(items, L):
    if (items, L) not in _shared:
        torch.manual_seed(0)
        m = _new_model(items, L)
        for _, p in m.named_parameters():
            if p.dim() >= 2:
                torch.nn.init.xavier_normal_(p.data)
        _shared[items, L] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return _shared[items, L]


def _trainer(items, B, L, sd=None, **kw):
    import srfrd_amd
    m = _new_model(items, L)
    m.load_state_dict(_weights(items, L) if sd is None else sd)
    return srfrd_amd.FusedTrainer(m.to("cuda").train(), B, L, **kw)


def _batches(items, B, L, K=0, n=3, seed=11):
    """-> [(batch planes, (negatives, log_q) or None)]"""
    import srfrd_amd
    out = []
    for i in range(n):
        b = srfrd_amd.synthetic_batch(items, L, B, seed=seed + i, device="cuda")[1:]
        neg = srfrd_amd.sample_token_negatives(items, b[2], K, generator=torch.Generator("cuda").manual_seed(40 + i)) if K else None
        out.append((b, neg))
    return out


def _step(tr, batch, neg):
    if tr.token:
        return tr.step(None, batch[0], batch[1], batch[2], batch[3], neg[0], batch[5], log_q=neg[1])
    return tr.step(None, *batch)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.is_floating_point() else t


def _assert_same(a, b, where, rows=None):
    """parameters, moments, loss and the sorted key list of two trainers, as bit patterns (``rows``: these table rows alone)"""
    torch.cuda.synchronize()
    assert math.isfinite(float(a.loss))
    pairs = [("loss", a.loss, b.loss), ("skeys", a.skeys, b.skeys), ("order", a.order, b.order)]
    for name in ("flat", "m", "v"):
        x, y = getattr(a, name), getattr(b, name)
        if rows is not None:
            d = a.lay.d_item
            x, y = x[:a.lay.n_table].view(-1, d)[rows], y[:b.lay.n_table].view(-1, d)[rows]
        pairs.append((name, x, y))
    if rows is None:
        pairs.append(("state", a.state, b.state))
    for name, x, y in pairs:
        bad = (_bits(x) != _bits(y)).reshape(-1)
        assert not bool(bad.any()), f"{where}: {name}: {int(bad.sum())} of {x.numel()} elements differ, first at " \
                                    f"{bad.nonzero().flatten()[:8].tolist()}"


def _pair(items, B, L, use_graph=True, **kw):
    dev = _trainer(items, B, L, use_graph=use_graph, key_sort="device", **kw)
    ref = _trainer(items, B, L, use_graph=use_graph, key_sort="torch", **kw)
    assert dev.sort_ws is not None and ref.sort_ws is None and dev.n_keys == ref.n_keys > 0
    assert dev.sort_ws.data_ptr() % 16 == 0
    return dev, ref


def _three_steps(dev, ref, batches, where):
    for i, (b, neg) in enumerate(batches):
        _step(dev, b, neg)
        _step(ref, b, neg)
        _assert_same(dev, ref, f"{where} step {i}")
    dev.check()
    ref.check()


# ---- the token losses: one graph instead of two -----------------------------------------------------------------------------------
TOKEN_SHAPES = {"K1": (4, 20, 1), "K5": (4, 20, 5), "K65": (4, 20, 65), "L50-K5": (4, 50, 5)}       # B, L, K


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("shape", list(TOKEN_SHAPES))
@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_token_step_same_bits_and_one_graph(loss, shape, use_graph):
    B, L, K = TOKEN_SHAPES[shape]
    dev, ref = _pair(ITEMS, B, L, use_graph, loss=loss, num_negatives=K, gbce_beta=0.7)
    assert dev.n_keys == B * L * (2 + K)
    assert len(dev._program) == 1 and dev._program[0][:2] == ("graph", True) and "_sort_keys" in dev._program[0][2]
    assert [kind for kind, _, _ in ref._program] == ["graph", "eager", "graph"]
    _three_steps(dev, ref, _batches(ITEMS, B, L, K), f"{loss} {shape}")
    if use_graph:
        assert dev.graph_form == "one" and ref.graph_form == "split" and dev.graph_capture_error is None
    else:
        assert dev.graph_form is None and ref.graph_form is None and not dev.captured


# ---- the other sorted steps -------------------------------------------------------------------------------------------------------
OTHERS = {
    "sampled-softmax-K16": (8, 50, dict(loss="sampled_softmax", num_negatives=16)),
    "bce-deterministic": (8, 50, dict(deterministic=True)),
    "bce-lazy-L8-generic": (5, 8, dict(lazy_table=True)),
    "bce-lazy-L50-train-kernel": (5, 50, dict(lazy_table=True)),
}


@pytest.mark.parametrize("name", list(OTHERS))
def test_other_sorted_steps_same_bits(name):
    from srfrd_amd import _lib
    B, L, kw = OTHERS[name]
    dev, ref = _pair(ITEMS, B, L, True, **kw)
    if "lazy" in name:       # L 8 runs the generic forward and backward, L 50 the one-launch train kernel
        has_train = bool(_lib.encoder_plan_train(dev.lay, B, L, dev._train_mode, _lib.env_switches())[0])
        assert has_train == (L == 50)
    assert dev._program == ref._program and len(dev._program) == 1
    _three_steps(dev, ref, _batches(ITEMS, B, L), name)
    assert dev.graph_form == ref.graph_form == "one"


def test_an_unsorted_trainer_accepts_the_option_and_changes_nothing():
    dev = _trainer(ITEMS, 4, 20, key_sort="device")
    ref = _trainer(ITEMS, 4, 20)
    assert dev.n_keys == 0 and dev.sort_ws is None and dev.keys is None and dev._program == ref._program
    # one step: its table gradient is scattered by float atomics (no run repeats another's bits), the loss and the dense
    # parameters' step are reproducible
    (b, _), = _batches(ITEMS, 4, 20, n=1)
    dev.step(None, *b)
    ref.step(None, *b)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev.loss), _bits(ref.loss))
    for name in ("flat", "m", "v"):
        assert torch.equal(_bits(getattr(dev, name)[dev.n_tab:]), _bits(getattr(ref, name)[ref.n_tab:])), name


def test_an_invalid_id_is_recorded_by_both_and_the_valid_rows_agree():
    B, L = 8, 50
    dev, ref = _pair(ITEMS, B, L, True, deterministic=True)
    (b, _), = _batches(ITEMS, B, L, n=1)
    b = [t.clone() for t in b]
    assert int(b[4][3, L - 1]) != 0
    b[4][3, L - 1] = ITEMS + 1                         # a negative id one above the table
    for tr in (dev, ref):
        tr.step(None, *b)
    valid = torch.unique(torch.cat([b[0].reshape(-1), b[2].reshape(-1), b[4].reshape(-1)]))
    valid = valid[(valid >= 1) & (valid <= ITEMS)]
    _assert_same(dev, ref, "invalid id", rows=valid)
    assert int(dev.skeys[-1]) == ITEMS + 1 and int(ref.skeys[-1]) == ITEMS + 1
    for tr in (dev, ref):
        with pytest.raises(IndexError, match="item id outside"):
            tr.check()


def test_checkpoints_move_between_the_two_sorts():
    B, L, K = 4, 20, 5
    kw = dict(loss="token_softmax", num_negatives=K)
    dev, ref = _pair(ITEMS, B, L, True, **kw)
    batches = _batches(ITEMS, B, L, K, n=4)
    for b, neg in batches[:2]:
        _step(dev, b, neg)
        _step(ref, b, neg)
    assert "key_sort" not in str(dev.state_dict()["srfrd"]) and dev.state_dict()["srfrd"] == ref.state_dict()["srfrd"]
    # device -> torch, and torch -> device
    to_ref = _trainer(ITEMS, B, L, sd=dev.model.state_dict(), key_sort="torch", **kw)
    to_ref.load_state_dict(dev.state_dict())
    to_dev = _trainer(ITEMS, B, L, sd=ref.model.state_dict(), key_sort="device", **kw)
    to_dev.load_state_dict(ref.state_dict())
    for i, (b, neg) in enumerate(batches[2:]):
        for tr in (dev, ref, to_ref, to_dev):
            _step(tr, b, neg)
        for other, name in ((ref, "torch"), (to_ref, "device -> torch"), (to_dev, "torch -> device")):
            _assert_same(dev, other, f"{name}, step {2 + i}")
    assert to_dev.graph_form == "one" and to_ref.graph_form == "split"


# ---- the shape whose captured rocprim sort faulted --------------------------------------------------------------------------------
def test_c2_size_token_step_is_one_captured_graph():
    """B 512, L 50, K 64: 1 689 600 keys.  Under "device" the step is one graph that holds kernel nodes only; "torch" runs
    without graphs (its sort over the limit is never captured)."""
    from srfrd_amd.trainer import SORT_CAPTURE_LIMIT
    from tests import skew_cases as S
    items, B, L, K = 50_000, 512, 50, 64
    kw = dict(loss="token_softmax", num_negatives=K)
    dev = _trainer(items, B, L, use_graph=True, key_sort="device", **kw)
    ref = _trainer(items, B, L, use_graph=False, key_sort="torch", **kw)
    assert dev.n_keys == 1_689_600 > SORT_CAPTURE_LIMIT
    # before anything is captured: one stage, and a sort that takes the device branch
    assert len(dev._program) == 1 and dev._program[0][0] == "graph" and not dev.captured
    assert dev.key_sort == "device" and dev.sort_ws is not None and ref.sort_ws is None
    with S.use("product") as rec:
        for i, (b, neg) in enumerate(_batches(items, B, L, K, n=2)):
            _step(dev, b, neg)
            _step(ref, b, neg)
            _assert_same(dev, ref, f"C2 step {i}")
    assert "srfrd_sort_keys" in rec.called
    assert dev.captured and dev.graph_form == "one" and len(dev._graphs[0]) == 1
