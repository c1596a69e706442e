"""-m gpu: FusedTrainer's learning-rate schedule, gradient-norm clipping and decoupled weight decay, and
srfrd_amd.AdamW on the module-level path.  Every trainer is ``deterministic=True`` over 300 items; the one-launch (ragged) family
runs at L = 50, B = 7, the generic two-launch family at L = 20, B = 5."""
import math

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.test_gpu_optim_options_kernels import _adamw_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FAMILIES = {"one_launch": (50, 7), "two_launch": (20, 5)}
K_NEG = 5
B1, B2, EPS = 0.9, 0.98, 1e-8
B1F = float(np.float32(B1))


def _cfg(L, dropout=0.2):
    return O.Cfg("SASRec", 300, L, 50, dropout=dropout)


def _batch(cfg, B, seed):
    import srfrd_amd
    return srfrd_amd.synthetic_batch(cfg.item_number, cfg.max_len, B, seed=seed, device="cuda")[1:]


def _token_negs(cfg, batch, seed):
    import srfrd_amd
    return srfrd_amd.sample_token_negatives(cfg.item_number, batch[2], K_NEG, generator=torch.Generator("cuda").manual_seed(seed))[0]


def _trainer(cfg, sd, B, loss="bce", **kw):
    import srfrd_amd
    from srfrd_amd import _lib
    from tests.gpu_util import build_model
    tr = srfrd_amd.FusedTrainer(build_model(cfg, sd).train(), B, cfg.max_len, loss=loss, num_negatives=K_NEG, deterministic=True,
                                seed=11, **kw)
    if loss == "bce":           # the family the shape was chosen for
        one = bool(_lib.encoder_plan_train(tr.lay, B, cfg.max_len, tr._train_mode, _lib.env_switches())[0])
        assert one == (cfg.max_len == 50)
    return tr


def _step(tr, cfg, batch, seed=0):
    if tr.token:
        return tr.step(None, batch[0], batch[1], batch[2], batch[3], _token_negs(cfg, batch, 100 + seed), batch[5])
    return tr.step(None, *batch)


def _bits(tr):
    torch.cuda.synchronize()
    return (tr.flat.detach().clone(), tr.m.detach().clone(), tr.v.detach().clone(), tr.state.detach().clone(),
            tr.loss.detach().clone())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- neutral ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_default_options_are_the_plain_step(family):
    from tests.gpu_util import random_sd
    L, B = FAMILIES[family]
    cfg = _cfg(L)
    sd = random_sd(cfg, 5)
    plain = _trainer(cfg, sd, B)
    named = _trainer(cfg, sd, B, weight_decay=0.0, max_grad_norm=None, lr_schedule="constant", warmup_steps=0, total_steps=None,
                     final_lr_ratio=0.0)
    assert named.opts is None and named.grad_norm is None and named.next_lr is None
    for s in range(3):
        batch = _batch(cfg, B, 20 + s)
        la, lb = float(_step(plain, cfg, batch)), float(_step(named, cfg, batch))
        assert math.isfinite(la) and la == lb
        assert _same(_bits(plain), _bits(named)), s
    g = named.state_dict()["param_groups"][0]
    assert g["weight_decay"] == 0 and g["decoupled_weight_decay"] is False and "schedule" not in named.state_dict()["srfrd"]


# ---- clipping -----------------------------------------------------------------------------------------------------------
CLIP_CASES = {"bce-one_launch": ("bce", 50, 7, 0.0), "bce-two_launch": ("bce", 20, 5, 0.0), "softmax": ("softmax", 50, 7, 0.0),
              "gbce": ("gbce", 20, 5, 0.0), "bce-l2_emb": ("bce", 50, 7, 1e-2)}


@pytest.mark.parametrize("case", CLIP_CASES)
def test_clipping(case):
    """step one from zero moments: m1 = (1 - b1) g, so the unclipped run gives the mean-loss gradient g (l2_emb term included)"""
    from tests.gpu_util import random_sd
    loss, L, B, l2 = CLIP_CASES[case]
    cfg = _cfg(L)
    sd = random_sd(cfg, 7)
    batch = _batch(cfg, B, 31)
    plain = _trainer(cfg, sd, B, loss, l2_emb=l2)
    measure = _trainer(cfg, sd, B, loss, l2_emb=l2, max_grad_norm=float("inf"))
    for tr in (plain, measure):
        _step(tr, cfg, batch)
    assert _same(_bits(plain)[:3], _bits(measure)[:3]) and float(plain.loss) == float(measure.loss)      # measuring changes nothing
    m1 = measure.m.detach().double().cpu()
    g = m1 / (1.0 - B1F)
    norm = float(torch.sqrt((g * g).sum()))
    got = float(measure.grad_norm)
    print(f"{case}: |g| from m1 {norm:.9g}, grad_norm {got:.9g}, rel {abs(got - norm) / norm:.3g}")
    assert norm > 0 and abs(got - norm) <= 4 * U * norm, (got, norm)
    assert float(measure.clip[1]) == 1.0

    # max_grad_norm = |g| / 2 (from the unclipped run: the clip is active): m1 is the unclipped m1 times the coefficient
    clipped = _trainer(cfg, sd, B, loss, l2_emb=l2, max_grad_norm=0.5 * norm)
    _step(clipped, cfg, batch)
    torch.cuda.synchronize()
    assert float(clipped.grad_norm) == got                            # the same gradient, the same bits
    coef = float(clipped.clip[1])
    want_coef = 0.5 * norm / (got + 1e-6)
    assert abs(coef - want_coef) <= 2 * U * want_coef and 0.49 < coef < 0.51, (coef, want_coef)
    want = m1 * coef
    have = clipped.m.detach().double().cpu()
    worst = 0.0
    for p, off in clipped.model._slots:
        n, d = p.numel(), p.shape[-1]
        w, h = want[off:off + n].view(-1, d), have[off:off + n].view(-1, d)
        floor = torch.from_numpy(np.spacing(w.abs().max(dim=1, keepdim=True).values.numpy().astype(np.float32)).astype(np.float64))
        bound = 4 * U * w.abs() + floor
        assert bool(((h - w).abs() <= bound).all()), (case, off, float(((h - w).abs() / bound).max()))
        worst = max(worst, float(((h - w).abs() / bound).max()))
    print(f"{case}: coefficient {coef:.7f}, worst |m1_clipped - coef m1| / bound {worst:.3f}")
    assert not torch.equal(clipped.flat, plain.flat)

    # max_grad_norm = 2 |g|: coefficient 1, the whole step is bitwise the unclipped one
    loose = _trainer(cfg, sd, B, loss, l2_emb=l2, max_grad_norm=2.0 * norm)
    _step(loose, cfg, batch)
    assert float(loose.clip[1]) == 1.0
    assert _same(_bits(loose)[:3], _bits(plain)[:3]) and float(loose.loss) == float(plain.loss)
    s_l, s_p = loose.state.cpu(), plain.state.cpu()
    assert all(int(s_l[i]) == int(s_p[i]) for i in (0, 1, 2, 4, 5))


# ---- schedule and decay -------------------------------------------------------------------------------------------------
SCHED = dict(lr_schedule="linear", warmup_steps=2, total_steps=5, final_lr_ratio=0.1, weight_decay=0.1)


def _lr(t, lr=1e-3):
    from srfrd_amd import lr_at
    return lr_at(t, lr, "linear", 2, 5, 0.1)


@pytest.mark.parametrize("family", FAMILIES)
def test_schedule_and_decay_follow_the_formula_in_graph_and_eager(family):
    """p_t = p_{t-1} (1 - lr_t wd) - lr_t / bc1 * m_t / (sqrt(v_t) / sqrt(bc2) + eps) in fp64 from the device's own p_{t-1}, m_t,
    v_t and lr_at(t).  Bound, in _adam_ref's form (2x the worst-case rounding sum): the state words lr_t / bc1, sqrt(bc2) and
    1 - lr_t wd are each one fp32 rounding of the fp64 value, p decay rounds once, and the update chain sqrt, /, + eps, /, *, -
    rounds six times: 2 (3 U |p| + 10 U |update|)."""
    from tests.gpu_util import random_sd
    L, B = FAMILIES[family]
    cfg = _cfg(L)
    sd = random_sd(cfg, 9)
    graph, eager = _trainer(cfg, sd, B, use_graph=True, **SCHED), _trainer(cfg, sd, B, use_graph=False, **SCHED)
    epsf = float(np.float32(EPS))
    assert abs(float(graph.next_lr) - _lr(1)) <= np.spacing(np.float32(_lr(1)))
    for t in range(1, 7):
        batch = _batch(cfg, B, 40 + t)
        p_prev = graph.flat.detach().double().cpu()
        lg, le = float(_step(graph, cfg, batch)), float(_step(eager, cfg, batch))
        assert math.isfinite(lg) and lg == le, (t, lg, le)
        assert _same(_bits(graph), _bits(eager)), t                   # (a rate baked into the graph fails here from t = 2)
        p, m, v = (x.detach().double().cpu() for x in (graph.flat, graph.m, graph.v))
        lr_t = _lr(t)
        upd = lr_t / (1.0 - B1 ** t) * m / (v.sqrt() / math.sqrt(1.0 - B2 ** t) + epsf)
        want = p_prev * (1.0 - lr_t * 0.1) - upd
        bound = 2 * (3 * U * p_prev.abs() + 10 * U * upd.abs())
        ratio = float(((p - want).abs() / bound.clamp_min(1e-300)).max())
        print(f"{family} t={t}: lr_t {lr_t:.3e}, worst |p - formula| / bound {ratio:.3f}")
        assert bool(((p - want).abs() <= bound).all()), (t, ratio)
        nxt = _lr(t + 1)
        assert abs(float(graph.next_lr) - nxt) <= np.spacing(np.float32(nxt)), (t, float(graph.next_lr), nxt)
    assert graph.captured and not eager.captured
    # the decay and the schedule really act: a plain trainer on the same batches ends elsewhere
    plain = _trainer(cfg, sd, B)
    for t in range(1, 7):
        _step(plain, cfg, _batch(cfg, B, 40 + t))
    assert float((plain.flat - graph.flat).abs().max()) > 1e-4


# ---- resume and spin_up -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_resume_mid_decay_is_the_uninterrupted_run(family):
    from tests.gpu_util import random_sd
    L, B = FAMILIES[family]
    cfg = _cfg(L)
    sd = random_sd(cfg, 13)
    kw = dict(SCHED, max_grad_norm=0.05)
    batches = [_batch(cfg, B, 60 + i) for i in range(5)]
    straight = _trainer(cfg, sd, B, **kw)
    for b in batches:
        _step(straight, cfg, b)
    first = _trainer(cfg, sd, B, **kw)
    for b in batches[:3]:
        _step(first, cfg, b)
    opt_sd = first.state_dict()
    model_sd = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    g = opt_sd["param_groups"][0]
    assert g["lr"] == 1e-3 and g["weight_decay"] == 0.1 and g["decoupled_weight_decay"] is True
    assert opt_sd["srfrd"]["schedule"] == {"kind": "linear", "warmup_steps": 2, "total_steps": 5, "final_lr_ratio": 0.1}
    assert opt_sd["srfrd"]["max_grad_norm"] == 0.05 and opt_sd["srfrd"]["steps_done"] == 3
    for fresh_kw in ({}, kw):                                         # the options come from the dict, whatever the trainer had
        second = _trainer(cfg, model_sd, B, **fresh_kw)
        second.load_state_dict(opt_sd)
        assert abs(float(second.next_lr) - _lr(4)) <= np.spacing(np.float32(_lr(4)))      # the save landed mid-decay
        assert _lr(5) < _lr(4) < _lr(3)
        for b in batches[3:]:
            _step(second, cfg, b)
        assert _same(_bits(second), _bits(straight))
        assert float(second.grad_norm) == float(straight.grad_norm) and float(second.clip[1]) < 1.0


def test_spin_up_changes_nothing():
    from tests.gpu_util import random_sd
    cfg = _cfg(50)
    B = 7
    sd = random_sd(cfg, 15)
    kw = dict(SCHED, max_grad_norm=0.05)
    batches = [_batch(cfg, B, 80 + i) for i in range(2)]
    outs = []
    for spin in (False, True):
        tr = _trainer(cfg, sd, B, **kw)
        _step(tr, cfg, batches[0])
        if spin:
            # (parameters, moments, state words; `loss` is an output, spin_up leaves its last replay's there)
            before = (_bits(tr)[:4], float(tr.next_lr), float(tr.grad_norm))
            tr.spin_up(20)
            assert tr.captured and tr.steps_done == 1
            assert (float(tr.next_lr), float(tr.grad_norm)) == before[1:] and _same(_bits(tr)[:4], before[0])
        _step(tr, cfg, batches[1])
        outs.append((_bits(tr), float(tr.next_lr), float(tr.grad_norm)))
    assert _same(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_coupled_weight_decay_is_still_refused():
    from tests.gpu_util import random_sd
    cfg = _cfg(20)
    tr = _trainer(cfg, random_sd(cfg, 1), 5, weight_decay=0.1)
    sd = tr.state_dict()
    before = _bits(tr)
    for bad in (dict(weight_decay=0.1, decoupled_weight_decay=False), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError):
            tr.load_state_dict(dict(sd, param_groups=[dict(sd["param_groups"][0], **bad)]))
    coupled = dict(sd["param_groups"][0], weight_decay=0.1)
    del coupled["decoupled_weight_decay"]                             # (torch.optim.Adam of an older torch: coupled)
    with pytest.raises(ValueError, match="decoupled"):
        tr.load_state_dict(dict(sd, param_groups=[coupled]))
    assert _same(_bits(tr), before) and tr.opts.weight_decay == 0.1
    tr.load_state_dict(sd)                                            # what state_dict() wrote is welcome


# ---- srfrd_amd.AdamW ----------------------------------------------------------------------------------------------------
def test_module_level_adamw_against_fp64_under_a_lambda_lr():
    """three steps of model(...) -> BCE -> backward -> srfrd_amd.AdamW.step() under a LambdaLR, the item table frozen: every
    stepped tensor against the fp64 AdamW restatement of the kernel tests (their bounds) on the autograd path's own gradients,
    from the optimizer's own previous moments; the frozen table and its (absent) state untouched"""
    import srfrd_amd
    from tests.gpu_util import build_model, random_sd
    cfg = _cfg(50, dropout=0.0)
    model = build_model(cfg, random_sd(cfg, 17)).train()
    model.item_emb.weight.requires_grad_(False)
    table0 = model.item_emb.weight.detach().clone()
    lr, wd = 2e-3, 0.1
    params = [p for p in model.parameters() if p.requires_grad]
    opt = srfrd_amd.AdamW(params, lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd)
    factor = lambda e: min(1.0, (e + 1) / 2) * (0.5 if e >= 2 else 1.0)      # noqa: E731  (0.5, 1, 0.5)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, factor)
    crit = torch.nn.BCEWithLogitsLoss()
    moments = {id(p): (np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32)) for p in params}
    for t in range(1, 4):
        u, seq, rsq, pos, prs, neg, nrs = srfrd_amd.synthetic_batch(300, 50, 7, seed=90 + t, device="cuda")
        _, pl, nl = model(u, seq, rsq, pos, prs, neg, nrs)
        idx = torch.where(pos != 0)
        loss = crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])
        opt.zero_grad()
        loss.backward()
        lr_t = opt.param_groups[0]["lr"]
        assert lr_t == lr * factor(t - 1)
        before = {id(p): (p.detach().cpu().numpy().reshape(-1).copy(), p.grad.detach().cpu().numpy().reshape(-1).copy()) for p in params}
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        words = opt._dev_state.cpu().numpy()
        ss, bc2s, decay = (float(words[i:i + 1].view(np.float32)[0]) for i in (4, 5, 7))
        for got, want in ((ss, lr_t / (1 - B1 ** t)), (bc2s, math.sqrt(1 - B2 ** t)), (decay, 1 - lr_t * wd)):
            assert abs(got - want) <= np.spacing(np.float32(want)), (t, got, want)
        assert int(words[0]) == t
        state = opt.state_dict()["state"]
        for i, p in enumerate(params):
            p0, g = before[id(p)]
            m0, v0 = moments[id(p)]
            rp, rm, rv, ep, em, ev = _adamw_ref(p0, g, m0, v0, B1, B2, EPS, ss, bc2s, 1.0, 1.0, decay)
            p1 = p.detach().cpu().numpy().reshape(-1)
            m1 = state[i]["exp_avg"].cpu().numpy().reshape(-1)
            v1 = state[i]["exp_avg_sq"].cpu().numpy().reshape(-1)
            assert float(state[i]["step"]) == t
            assert (np.abs(p1 - rp) <= ep).all() and (np.abs(m1 - rm) <= em).all() and (np.abs(v1 - rv) <= ev).all(), (t, i)
            moments[id(p)] = (m1.copy(), v1.copy())
    assert torch.equal(model.item_emb.weight.detach(), table0)
    sd = opt.state_dict()
    assert len(sd["state"]) == len(params) and sd["param_groups"][0]["weight_decay"] == wd
    assert sd["param_groups"][0]["decoupled_weight_decay"] is True
