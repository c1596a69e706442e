"""-m gpu: the key-padding mask (``model.use_key_padding_mask()``, ``srfrd_layout.flags & SRFRD_LAYOUT_MASK_PAD_KEYS``) on every
encoder kernel family, against the masked fp64 oracle of tests/keymask_refs.py.

  forward     every case of grad_refs.ALL_CASES in every mode of fwd_refs.MODES (eval, last + predict, train with dropout 0.5),
              metric and bound fwd_refs', the planned kernel name asserted before each launch (the flag moves no plan);
  gradients   ``p.grad`` of the autograd path and the first fused step read from the Adam moments, both scatter modes, for
              every case; grad_refs.TRAIN_KERNEL_IDS also as two launches; metric and bound grad_refs';
  neutrality  one case per distinct set of planned kernel names on a batch WITHOUT pads: flag on and flag off give the same
              bits - outputs, checkpoints, and the fused step's loss, parameters and moments;
  window      a model at max_len 50 against one at 20 that holds its last 20 position rows (SASRec, SRFRN: the ragged family
              against the first-generation one), 100 against 50 and 200 against 100 (the row-owner forward): with the flag the
              live rows agree inside the sum of the two forwards' bounds, without it they differ by 0.1 of a row's size and more;
  edges       an all-pad row beside live ones, t0 = L - 1, an interior zero, and a pad key whose score is about +200 against
              real scores near 0 - a masked key left in the row maximum gives 0 / 0 there;
  trainer     the captured graph and the eager step give the same bits with the flag on; a flag changed behind a trainer's
              back makes its next step raise.

The shapes are the suites' own (I = 300, B of a few to 17 sequences).
"""
import pytest
import torch

from oracle import srfrd_oracle as O
from tests import fwd_refs as F
from tests import grad_refs as G
from tests import keymask_refs as K
from tests import test_gpu_bf16_families as FAM
from tests import test_gpu_fwd_fp64 as W

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", G.ALL_CASES, ids=G.case_ids())
scatter = pytest.mark.parametrize("det", [True, False], ids=["deterministic", "atomics"])


def _model(cfg, sd, switch, setenv, on=True):
    model = W._model(cfg, sd, switch, setenv)
    assert not model.key_padding_mask and model.layout.flags == 0
    assert model.use_key_padding_mask(on) is model and model.key_padding_mask == on
    return model


# ---------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------
def run_forward(c, mode, setenv):
    """-> {output: fwd_refs.figures} of one mode's launch with the flag on, against the masked reference"""
    from tests.gpu_util import cuda
    ref = K.fwd_reference(c.id, mode)
    F.assert_admissible(ref, f"case {c.id} {mode} masked")
    model = _model(ref.cfg, ref.sd, c.switch, setenv)
    W._assert_plan(model, c.B, c.L, mode, c.switch, F.plan_name(c, mode))
    if mode == "eval":
        return F.compare(W._eval(model, ref), ref)
    if mode == "last":
        return F.compare(W._last(model, ref), ref)
    assert ref.cfg.dropout == 0.5 and ref.train
    model.train()
    model._next_seed = lambda: ref.seed
    seq, rsq, pos, prs, neg, nrs = cuda(*ref.batch)
    W._poison((c.B, c.L, ref.cfg.d_out), (c.B, c.L), (c.B, c.L))
    h, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    assert h.requires_grad
    figs = F.compare({"hidden": h, "pos_logits": pl, "neg_logits": nl}, ref)
    F.assert_loss_holds(FAM._bce(pl.detach(), nl.detach(), pos), ref, f"case {c.id} train masked")
    return figs


@pytest.mark.parametrize("mode", F.MODES)
@cases
def test_forward_meets_the_masked_fp64_oracle(c, mode, monkeypatch):
    F.assert_holds(run_forward(c, mode, monkeypatch.setenv), f"keymask fwd case {c.id} {mode}")


# ---------------------------------------------------------------------------------------------------------------------------
# 2. gradients
# ---------------------------------------------------------------------------------------------------------------------------
def run_autograd(c, setenv):
    from tests.gpu_util import cuda
    ref = K.grad_reference(c.id, "autograd")
    G.assert_admissible(ref, f"case {c.id} autograd masked")
    model = _model(ref.cfg, ref.sd, c.switch, setenv).train()
    FAM._assert_plan(c, model, "autograd", c.autograd)
    seq, rsq, pos, prs, neg, nrs = cuda(*ref.batch)
    _, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    FAM._bce(pl, nl, pos).backward()
    return G.compare({k: p.grad for k, p in model.named_parameters()}, ref)


def run_fused(c, det, setenv, train_launch=True):
    import srfrd_amd
    from srfrd_amd import _lib
    from tests.gpu_util import cuda
    ref = K.grad_reference(c.id, "fused")
    G.assert_admissible(ref, f"case {c.id} fused masked")
    model = _model(ref.cfg, ref.sd, c.switch, setenv).train()
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=det)
    tr.train_launch = train_launch
    FAM._assert_plan(c, model, "fused", c.fused, scratch=tr.n_scratch)
    if c.id in G.TRAIN_KERNEL_IDS:
        assert _lib.encoder_plan_train(tr.lay, c.B, c.L, tr._train_mode, _lib.env_switches())[0].startswith(
            "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here"
    loss = tr.step(None, *cuda(*ref.batch))
    assert bool(torch.isfinite(loss).all())
    F.assert_loss_holds(loss.detach().cpu(), K.fused_step_reference(c.id), f"case {c.id} fused masked det={det}")
    g, g2 = G.fused_gradients(tr, model)
    return G.compare(g, ref), G.compare(g2, ref, squares=True)


@cases
def test_autograd_gradients_meet_the_masked_fp64_oracle(c, monkeypatch):
    G.assert_holds(run_autograd(c, monkeypatch.setenv), f"keymask grad case {c.id} autograd")


@scatter
@cases
def test_fused_step_gradients_meet_the_masked_fp64_oracle(c, det, monkeypatch):
    figs, figs2 = run_fused(c, det, monkeypatch.setenv)
    G.assert_holds(figs, f"keymask grad case {c.id} fused det={det}")
    G.assert_holds(figs2, f"keymask grad case {c.id} fused det={det} second moment")


@scatter
@pytest.mark.parametrize("cid", G.TRAIN_KERNEL_IDS)
def test_two_launch_step_gradients_meet_the_masked_fp64_oracle(cid, det, monkeypatch):
    figs, figs2 = run_fused(G.BY_ID[cid], det, monkeypatch.setenv, train_launch=False)
    G.assert_holds(figs, f"keymask grad case {cid} two-launch det={det}")
    G.assert_holds(figs2, f"keymask grad case {cid} two-launch det={det} second moment")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. neutrality: nothing to mask, nothing changes
# ---------------------------------------------------------------------------------------------------------------------------
def _names(c):
    return (c.eval_fwd, c.last_fwd, c.autograd, c.fused)


def _distinct(cases_):
    seen, out = set(), []
    for c in cases_:
        if _names(c) not in seen:
            seen.add(_names(c))
            out.append(c)
    return out


NEUTRAL = _distinct(G.DEPTH2_CASES)


def _full_batch(c, seed=3):
    g = torch.Generator().manual_seed(seed)
    seq, pos, neg = (torch.randint(1, G.I + 1, (c.B, c.L), generator=g) for _ in range(3))
    return G._reviews(g, seq, pos, neg)


@pytest.mark.parametrize("c", NEUTRAL, ids=G.case_ids(NEUTRAL))
def test_a_batch_without_pads_gives_the_same_bits_with_the_flag(c, monkeypatch):
    import srfrd_amd
    from tests.gpu_util import cuda
    batch = cuda(*_full_batch(c))
    assert bool((batch[0] != 0).all())
    sd = G.weights(c.id)
    got = {}
    for on in (False, True):
        out = {}
        cfg = G.cfg_of(c, "fused")
        model = _model(cfg, sd, c.switch, monkeypatch.setenv, on)
        FAM._assert_plan(c, model, "eval", (c.eval_fwd, None))
        with torch.no_grad():
            ids = model._prep(*batch)
            out.update({f"eval.{k}": v for k, v in model._launch_fwd(*ids, 0.0, 0, False).items() if v is not None})
            out["last"] = model._launch_fwd_last(ids[0], ids[1])
            # (the ragged forward leaves the checkpoint floats no backward reads unwritten - probability columns 56 .. 62, and
            # column 63 of a sequence without pads: the launch's buffers start from zeros here, so that every float compares)
            with monkeypatch.context() as mp:
                mp.setattr(torch, "empty", torch.zeros)
                out.update({f"ckpt.{k}": v for k, v in model._launch_fwd(*ids, 0.5, O.step_seed(G.BASE, 1), True).items()})
        model.train()
        tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=True)
        FAM._assert_plan(c, model, "fused", c.fused, scratch=tr.n_scratch)
        out["step.loss"] = tr.step(None, *batch).clone()
        out["step.flat"], out["step.m"], out["step.v"] = model._flat.clone(), tr.m.clone(), tr.v.clone()
        torch.cuda.synchronize()
        got[on] = out
    assert set(got[True]) == set(got[False]) and len(got[True]) >= 14
    for k in got[True]:
        assert bool(torch.isfinite(got[True][k]).all()), k
        assert torch.equal(got[True][k], got[False][k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the window property across kernel families
# ---------------------------------------------------------------------------------------------------------------------------
WINDOWS = [(50, 20), (100, 50), (200, 100)]


def _hidden(cfg, sd, ids, on):
    from tests.gpu_util import build_model, cuda
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}).use_key_padding_mask(on).eval()
    with torch.no_grad():
        return model(None, *cuda(*ids))[0].cpu()


def _live_rows(h, ns):
    return torch.cat([h[b, -n:] for b, n in enumerate(ns)])


def _row_difference(a, b, ref_rows):
    """fwd_refs' metric of a - b: each row's largest |difference| over the size of the reference's row"""
    return F.row_errors_inf((a.double() - b.double()) + ref_rows, ref_rows)


@pytest.mark.parametrize("long,short", WINDOWS)
@pytest.mark.parametrize("kind", K.WINDOW_KINDS)
def test_live_rows_do_not_depend_on_the_window(kind, long, short):
    (cl, sdl), (cs, sds) = K.window_weights(kind, long, short)
    ids_l, ids_s, ns = K.window_batch(long, short)
    bounds, x64 = [], None
    with K.masked(), torch.no_grad():
        for cfg, sd, ids in ((cl, sdl, ids_l), (cs, sds, ids_s)):
            h64 = O.forward(cfg, {k: v.double() for k, v in sd.items()}, *ids)[0]
            h32 = G._one_thread(lambda: O.forward(cfg, sd, *ids)[0])
            bounds.append(F.bound(F.row_errors_inf(h32, h64)))
            x64 = h64 if x64 is None else x64
    limit = sum(bounds)
    ref_rows = _live_rows(x64, ns)                                    # the rows' own size: the long window's fp64 reference
    masked, plain = (_row_difference(_live_rows(_hidden(cl, sdl, ids_l, on), ns), _live_rows(_hidden(cs, sds, ids_s, on), ns),
                                     ref_rows) for on in (True, False))
    print(f"keymask window {kind} {long}/{short}: masked {masked:.2e} of {limit:.2e}, unmasked {plain:.2e}")
    assert max(bounds) <= F.CAP_FWD                                   # (both forwards admissible: fwd_refs' condition)
    assert masked <= limit
    assert plain >= 0.1


# ---------------------------------------------------------------------------------------------------------------------------
# 5. edges
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_SWITCHES = [None, "SRFRD_NO_RAGGED", "SRFRD_ROWS_ALWAYS", "SRFRD_GENERIC", "SRFRD_RAGGED_FULL_ROWS"]
EDGE_L = 50


def _edge_batch():
    """row 0 all pad, row 1 a single item (t0 = L - 1), row 2 three pads and an interior zero, row 3 full, row 4 all pad"""
    g = torch.Generator().manual_seed(21)
    seq, pos, neg = (torch.randint(1, G.I + 1, (5, EDGE_L), generator=g) for _ in range(3))
    for b, t0 in enumerate((EDGE_L, EDGE_L - 1, 3, 0, EDGE_L)):
        for x in (seq, pos, neg):
            x[b, :t0] = 0
    seq[2, 27] = 0
    return G._reviews(g, seq, pos, neg)


def _against_masked_oracle(cfg, sd, batch, switch, setenv, what, two_heads=False):
    """eval forward and last-position state with the flag on against the masked fp64 oracle, bound from the fp32 oracle"""
    from tests.gpu_util import cuda
    with K.masked(), torch.no_grad():
        x64 = O.forward(cfg, {k: v.double() for k, v in sd.items()}, *batch)
        x32 = G._one_thread(lambda: O.forward(cfg, sd, *batch))
    model = _model(cfg, sd, switch, setenv).eval()
    with torch.no_grad():
        got = model(None, *cuda(*batch))
        ids = model._prep(*cuda(*batch[:2]), None, None, None, None)
        last = model._launch_fwd_last(ids[0], ids[1])
    figs = {}
    for name, x, r64, r32 in zip(("hidden", "pos_logits", "neg_logits"), got, x64, x32):
        assert bool(torch.isfinite(x).all()), (what, name)
        figs[name] = F.figures(x, r64, r32)
    figs["last_state"] = F.figures(last[:, 0], x64[0][:, -1], x32[0][:, -1])
    F.assert_holds(figs, what)
    return got, x64


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
@pytest.mark.parametrize("switch", EDGE_SWITCHES, ids=[s or "default" for s in EDGE_SWITCHES])
def test_all_pad_single_item_and_interior_zero(kind, switch, monkeypatch):
    from tests.gpu_util import random_sd
    cfg = K.window_cfg(kind, EDGE_L)
    sd = random_sd(cfg, G.SD_SEED)
    batch = _edge_batch()
    got, x64 = _against_masked_oracle(cfg, sd, batch, switch, monkeypatch.setenv, f"keymask edges {kind} {switch}")
    h = got[0].cpu()
    assert torch.equal(h[0], h[0, :1].expand_as(h[0])) and torch.equal(h[4], h[0])      # all pad: the last LayerNorm's bias
    # on the oracle alone: the interior zero carries weight as a key (a kernel that dropped it would miss the bound above by
    # orders of magnitude), and the three pads in front do count without the mask
    taps = {}
    with K.masked(), torch.no_grad():
        O.forward(cfg, {k: v.double() for k, v in sd.items()}, *batch, taps=taps)
        assert float(taps["p0"][2, :, 28:, 27].max()) > 1e-3 and bool((taps["p0"][2, :, 3:, :3] == 0).all())
    with torch.no_grad():
        plain = O.forward(cfg, {k: v.double() for k, v in sd.items()}, *batch)[0]
    assert float((plain[2, 3:] - x64[0][2, 3:]).abs().max()) > 1e-2


@pytest.mark.parametrize("switch", EDGE_SWITCHES[:4], ids=[s or "default" for s in EDGE_SWITCHES[:4]])
def test_autograd_gradients_of_the_edge_batch_are_finite_and_leave_the_pads_alone(switch, monkeypatch):
    from tests.gpu_util import cuda, random_sd
    cfg = K.window_cfg("SASRec", EDGE_L)
    sd = random_sd(cfg, G.SD_SEED)
    batch = _edge_batch()
    with K.masked():
        g64 = G.fp64_grads(cfg, sd, batch)
        g32 = G.fp32_grads(cfg, sd, batch)
        assert G.relu_margin(cfg, {k: v.double() for k, v in sd.items()}, batch) >= 2 * G.RELU_MARGIN
    model = _model(cfg, sd, switch, monkeypatch.setenv).train()
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    _, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    FAM._bce(pl, nl, pos).backward()
    figs = {k: G.tensor_figures(k, p.grad, g64[k], g32[k], cfg.D) for k, p in model.named_parameters()}
    G.assert_holds(figs, f"keymask edges grad {switch}")


PAD_COUNTS = (1, 7, 30, 45)


def _loud_pad_key(cfg, sd, beta=20.0, gamma=70.0, delta=20.0):
    """Block 0's key bias scaled so that a pad's score is about +200 and the real keys' stay near 0.  A bias alone shifts
    every key alike, so: every position row carries delta on channel 0 (x_j . w = 1 +- 0.03 on a live row, w = e_0 / delta; a
    pad row is 0), the query bias gets beta u and the key bias gamma u (u = a fixed unit vector: a pad's k = b_k scores
    q . b_k = gamma beta / sqrt(D) = 198), and the key weight loses gamma u w^T, which takes gamma u off every LIVE key again."""
    sd = {k: v.clone() for k, v in sd.items()}
    D = cfg.D
    u = torch.zeros(D)
    u[1:9] = 8 ** -0.5
    sd[O.key_pos(cfg)][:, 0] += delta
    w = torch.zeros(D)
    w[0] = 1.0 / delta
    sd["attention_layers.0.in_proj_bias"][:D] += beta * u
    sd["attention_layers.0.in_proj_bias"][D:2 * D] += gamma * u
    sd["attention_layers.0.in_proj_weight"][D:2 * D] -= gamma * torch.outer(u, w)
    return sd


@pytest.mark.parametrize("switch", EDGE_SWITCHES[:4], ids=[s or "default" for s in EDGE_SWITCHES[:4]])
def test_a_pad_key_with_a_large_score_is_out_of_the_row_maximum(switch, monkeypatch):
    from tests.gpu_util import random_sd
    cfg = K.window_cfg("SASRec", EDGE_L)
    sd = _loud_pad_key(cfg, random_sd(cfg, G.SD_SEED))
    g = torch.Generator().manual_seed(22)
    seq, pos, neg = (torch.randint(1, G.I + 1, (4, EDGE_L), generator=g) for _ in range(3))
    for b, t0 in enumerate(PAD_COUNTS):
        for x in (seq, pos, neg):
            x[b, :t0] = 0
    batch = G._reviews(g, seq, pos, neg)
    # on the oracle alone: the pads' scores stand about 200 over the live keys', far past exp's fp32 range (88)
    taps = {}
    O.forward(cfg, {k: v.double() for k, v in sd.items()}, *batch, taps=taps)
    s = taps["q0"] @ taps["k0"].transpose(-1, -2)
    for b, t0 in enumerate(PAD_COUNTS):
        gap = s[b, t0:, 0] - torch.stack([s[b, r, t0:r + 1].max() for r in range(t0, EDGE_L)])
        assert 120.0 < float(gap.min()) and float(gap.max()) < 280.0, (b, float(gap.min()), float(gap.max()))
    _against_masked_oracle(cfg, sd, batch, switch, monkeypatch.setenv, f"keymask loud pad key {switch}")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. trainer
# ---------------------------------------------------------------------------------------------------------------------------
def _trainer_run(c, use_graph, setenv):
    import srfrd_amd
    from tests.gpu_util import cuda
    model = _model(G.cfg_of(c, "fused"), G.weights(c.id), c.switch, setenv).train()
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=use_graph, deterministic=True)
    losses = [tr.step(None, *cuda(*G.batch_of(c, 50 + s))).clone() for s in range(3)]
    torch.cuda.synchronize()
    return torch.stack(losses), model._flat.clone(), tr.m.clone(), tr.v.clone(), tr, model


@pytest.mark.parametrize("cid", ["t0", "s", "g"])
def test_graph_and_eager_steps_agree_bitwise_with_the_flag_and_a_changed_flag_raises(cid, monkeypatch):
    from tests.gpu_util import cuda
    c = G.BY_ID[cid]
    eager = _trainer_run(c, False, monkeypatch.setenv)
    graph = _trainer_run(c, True, monkeypatch.setenv)
    for a, b, what in zip(eager[:4], graph[:4], ("loss", "parameters", "exp_avg", "exp_avg_sq")):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), what
    # ... and the flag acts in the step: the same three steps without it end elsewhere
    model = _model(G.cfg_of(c, "fused"), G.weights(c.id), c.switch, monkeypatch.setenv, on=False).train()
    import srfrd_amd
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=True)
    plain = torch.stack([tr.step(None, *cuda(*G.batch_of(c, 50 + s))).clone() for s in range(3)])
    assert not torch.equal(plain, eager[0])
    # changing the flag behind a trainer's back
    model.use_key_padding_mask()
    with pytest.raises(RuntimeError, match="use_key_padding_mask"):
        tr.step(None, *cuda(*G.batch_of(c, 53)))
    with pytest.raises(RuntimeError, match="use_key_padding_mask"):
        tr.step_slot(0)
    model.use_key_padding_mask(False)
    tr.step(None, *cuda(*G.batch_of(c, 53)))
    tr_on, model_on = graph[4], graph[5]
    model_on.use_key_padding_mask(False)
    with pytest.raises(RuntimeError, match="use_key_padding_mask"):
        tr_on.step_slot(0)


def test_the_switch_reaches_the_bf16_layout_in_either_order():
    from tests.gpu_util import build_model, random_sd
    cfg = K.window_cfg("SASRec", 20)
    sd = random_sd(cfg, G.SD_SEED)
    a = build_model(cfg, sd).use_key_padding_mask().use_bf16_table()
    b = build_model(cfg, sd).use_bf16_table().use_key_padding_mask()
    for m in (a, b):
        assert m.key_padding_mask and m.layout.flags == 1 and m._lay16.flags == 1 and m._lay16.table_bf16 == 1
        assert m._table_args()[0] is m._lay16
    seq = torch.randint(1, G.I + 1, (3, 20), generator=torch.Generator().manual_seed(1))
    seq[0, :9] = 0
    with torch.no_grad():
        ha, hb = a.eval()(None, seq.cuda(), None)[0], b.eval()(None, seq.cuda(), None)[0]
    assert torch.equal(ha, hb)
    b.use_key_padding_mask(False)
    assert not b.key_padding_mask and b._lay16.flags == 0 and b.layout.flags == 0
    with torch.no_grad():
        hc = b(None, seq.cuda(), None)[0]
    assert torch.equal(hc[1:], hb[1:]) and not torch.equal(hc[0, 9:], hb[0, 9:])
    assert "flags" not in " ".join(a.state_dict()) and set(a.state_dict()) == set(sd)
