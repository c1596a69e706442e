"""-m gpu: lazy Adam of the item table (include/srfrd_hip_lazy.h), in bits.

The KERNEL against the two kernels it replaces on the touched rows (srfrd_table_reduce into a zeroed gradient, then
srfrd_adam_step over the whole table), every other row against its pre-call bits.  The TRAINER against the dense
``deterministic=True`` trainer: the first step is the dense one (zero moments: an untouched row does not move under dense Adam
either), the second is fully characterised - dense parameters, touched rows and never-touched rows equal, the rows only the first
batch named frozen in the lazy trainer and moved by their momentum in the dense one.  Then six teacher-forced steps, the bf16
shadow, resume, and the skewed-barrier builds.  Equality is of bit patterns throughout: there is no tolerance in this file."""
import contextlib
import os

import pytest
import torch

import srfrd_amd
from srfrd_amd import _lib
from srfrd_amd._lib import call

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR = 0.9, 0.98, 1e-8, 2e-3
SEED = 37
CANARY_F, CANARY_H = 0x7FC0BEEF, 0x5A5A           # a NaN payload for m / v of rows nobody may touch, a bf16 pattern for the shadow
GENERIC = ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>")


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()]) if t.is_floating_point() else t


def _same(name, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
    bad = (_bits(a) != _bits(b)).reshape(-1)
    if bool(bad.any()):
        first = [int(i) for i in bad.nonzero().flatten()[:8]]
        raise AssertionError(f"{name}: {int(bad.sum())} of {a.numel()} elements differ, first at flat indices {first} "
                             f"({a.reshape(-1)[first].tolist()} vs {b.reshape(-1)[first].tolist()})")


def _bf16_rne(x):
    """f32_to_bf16 of finite floats: round to nearest even on the upper 16 bits -> int16"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
N_ROWS = 600


def _sorted_keys(case):
    """the SORTED key list of a case (the test shuffles it and sorts it back) -> int64 (n,)"""
    if case == "n1":
        return torch.tensor([7])
    if case == "n5":
        return torch.tensor([0, 3, 3, N_ROWS - 1, N_ROWS + 2])
    assert case == "big"
    runs = [(0, 3), (2, 1), (5, 4), (7, 300), (9, 64), (11, 65), (12, 8), (13, 9), (14, 7), (15, 128)]
    runs += [(k, 1 + (k % 3)) for k in range(20, 320, 2)]
    runs += [(N_ROWS - 1, 2), (N_ROWS, 3), (N_ROWS + 5, 2), (1 << 40, 1)]
    n = sum(c for _, c in runs)
    runs.insert(-4, (400, (1 - n) % 4 + 4))                       # n = 4 k + 1
    keys = torch.cat([torch.full((c,), k, dtype=torch.int64) for k, c in runs])
    assert bool((keys[1:] >= keys[:-1]).all()) and keys.numel() % 4 == 1
    start = {k: int((keys == k).nonzero()[0]) for k, _ in runs}
    count = dict(runs)
    # a workgroup owns four sorted positions: runs that end exactly where a workgroup does, one that IS a workgroup, the long
    # run over 75 workgroups and five prefetch chunks, runs of one chunk and one chunk + 1, of one prefetch depth and +- 1
    assert (start[2] + count[2]) % 4 == 0 and start[5] % 4 == 0 and count[5] == 4
    assert count[7] == 300 and (start[7] + 300) % 4 == 0 and count[9] == 64 and count[11] == 65
    assert (count[12], count[13], count[14]) == (8, 9, 7)
    return keys


def _state():
    state = torch.zeros(32, device="cuda", dtype=torch.int32)
    state[0], state[1] = 4, 12345
    call("srfrd_step_begin", state=state, lr=LR, beta1=B1, beta2=B2)
    return state


def _kernel_case(case, d, with_stats, with_shadow=True, seed=0):
    """inputs on the device, the expectation from the two existing kernels, the call -> everything the call could have written"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * d + len(case))
    skeys_want = _sorted_keys(case)
    n = skeys_want.numel()
    keys = skeys_want[torch.randperm(n, generator=g)].contiguous()
    contrib = torch.randn(n, d, generator=g).cuda()
    inside = (keys >= 1) & (keys < N_ROWS)
    touched = torch.unique(keys[inside])
    untouched = torch.ones(N_ROWS, dtype=torch.bool)
    untouched[touched] = False
    assert bool(untouched[0]) and touched.numel() >= 1
    table0 = torch.randn(N_ROWS, d, generator=g)
    m0, v0 = 0.1 * torch.randn(N_ROWS, d, generator=g), (0.05 * torch.randn(N_ROWS, d, generator=g)).abs()
    canary = torch.tensor([CANARY_F - (1 << 32) if CANARY_F >= 1 << 31 else CANARY_F], dtype=torch.int32).view(torch.float32)
    m0[untouched], v0[untouched] = canary, canary
    h0 = torch.full((N_ROWS, d), CANARY_H, dtype=torch.int16)
    stats = torch.tensor([2.0, 3.0, 41.0, 0.0]).cuda() if with_stats else None
    state = _state()
    state0 = state.clone()
    # the expectation: the in-range keys alone (srfrd_table_reduce would store through any other), stably sorted - a subset
    # keeps every run's order - into a zeroed gradient, then dense Adam over the whole table
    kr = torch.where(inside, keys, torch.zeros_like(keys)).cuda()
    sk, od = torch.sort(kr, stable=True)
    grad = torch.zeros(N_ROWS, d, device="cuda")
    call("srfrd_table_reduce", sorted_keys=sk, order=od, table_contrib=contrib, n=n, d_item=d, grad_table=grad)
    P, M, V, H = table0.cuda(), m0.cuda(), v0.cuda(), h0.cuda()
    call("srfrd_adam_step", param=P, grad=grad, m=M, v=V, n=N_ROWS * d, i0=0, i1=N_ROWS * d, n_zero=0, beta1=B1, beta2=B2, eps=EPS,
         state=state, stats=stats, table_bf16=H, n_table=N_ROWS * d)
    # the call
    skeys, order = torch.sort(keys.cuda(), stable=True)
    assert torch.equal(skeys.cpu(), skeys_want)
    T, m, v, h = table0.cuda(), m0.cuda(), v0.cuda(), (h0.cuda() if with_shadow else None)
    call("srfrd_table_reduce_adam", sorted_keys=skeys, order=order, table_contrib=contrib, n=n, d_item=d, n_rows=N_ROWS, table=T,
         m=m, v=v, beta1=B1, beta2=B2, eps=EPS, state=state, stats=stats, table_bf16=h)
    torch.cuda.synchronize()
    assert torch.equal(state, state0), "the call advanced the optimizer state"
    got = {"table": T.cpu(), "m": m.cpu(), "v": v.cpu()}
    if with_shadow:
        got["shadow"] = h.cpu()
    want = {"table": (P.cpu(), table0), "m": (M.cpu(), m0), "v": (V.cpu(), v0), "shadow": (H.cpu(), h0)}
    return got, want, touched, untouched


def _check_kernel(case, d, with_stats, with_shadow=True):
    got, want, touched, untouched = _kernel_case(case, d, with_stats, with_shadow)
    for name, t in got.items():
        stepped, before = want[name]
        _same(f"{name}: touched rows", t[touched], stepped[touched])
        _same(f"{name}: every other row (row 0 and the rows of out-of-range keys included)", t[untouched], before[untouched])
    assert torch.isfinite(got["table"][touched]).all() and not torch.equal(got["table"][touched], want["table"][1][touched])
    if with_shadow:
        _same("shadow: f32_to_bf16 of the stepped rows", got["shadow"][touched], _bf16_rne(got["table"][touched]))
        assert bool((got["shadow"][untouched] == CANARY_H).all())
    return got


@pytest.mark.parametrize("with_stats", [False, True], ids=["stats_null", "stats"])
@pytest.mark.parametrize("d", [1, 50, 64])
@pytest.mark.parametrize("case", ["n1", "n5", "big"])
def test_kernel_gives_the_bits_of_table_reduce_then_adam_step(case, d, with_stats):
    _check_kernel(case, d, with_stats)


def test_kernel_without_a_shadow():
    _check_kernel("big", 50, True, with_shadow=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the trainer
# ---------------------------------------------------------------------------------------------------------------------------------
ITEMS = 200
GEOMETRIES = {"SASRec-B3-L8": ("SASRec", 3, 8, None), "SASRec-B5-L50": ("SASRec", 5, 50, None), "SRFRN-B5-L50": ("SRFRN", 5, 50, None),
              "SASRec-B5-L50-noragged": ("SASRec", 5, 50, "SRFRD_NO_RAGGED"), "SRFRN-B5-L50-noragged": ("SRFRN", 5, 50, "SRFRD_NO_RAGGED")}


@contextlib.contextmanager
def _env(name):
    old = {k: os.environ.pop(k) for k in list(os.environ) if k in _lib.SWITCHES}
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        if name:
            os.environ.pop(name, None)
        os.environ.update(old)


def _model(kind, L, bf16=False):
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(ITEMS, L, 50, 0.5, 2, 1, "cuda") if kind == "SASRec" else srfrd_amd.SRFRN(ITEMS, L, 45, 5, 0.5, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().train()
    if bf16:
        m.use_bf16_table()
    return m


def _batch(hi, B, L, index):
    """(seq, rsq, pos, prs, neg, nrs) on the CPU, left-padded, every item id in [1, hi]"""
    return [x.clone() for x in srfrd_amd.synthetic_batch(hi, L, B, seed=11, index=index, device="cpu")[1:]]


def _rows(batch):
    ids = torch.cat([batch[0].reshape(-1), batch[2].reshape(-1), batch[4].reshape(-1)])
    return torch.unique(ids[ids != 0])


def _two_batches(B, L):
    """step 1 names ids up to 120, step 2 ids up to 60; 121..200 and the padding row are never named -> the batches and the
    three sets of rows, each asserted to hold at least 5, on the host"""
    b1, b2 = _batch(120, B, L, 0), _batch(60, B, L, 1)
    t1, t2 = set(_rows(b1).tolist()), set(_rows(b2).tolist())
    both, only1 = sorted(t1 & t2), sorted(t1 - t2)
    never = sorted(set(range(ITEMS + 1)) - t1 - t2)
    assert len(both) >= 5 and len(only1) >= 5 and len(never) >= 5 and 0 in never, (len(both), len(only1), len(never))
    assert bool((b1[0] == 0).any()), "no padded position in the batch"
    ix = lambda s: torch.tensor(s, dtype=torch.int64)      # noqa: E731
    return (b1, b2), ix(sorted(t2)), ix(both), ix(only1), ix(never)


def _assert_plan(tr, kind, B, L, switch):
    """the kernels this geometry plans, before anything is launched"""
    mode = tr._train_mode | _lib.PLAN_DROPOUT
    (fwd, _), (bwd, _) = _lib.encoder_plan(tr.lay, B, L, mode, _lib.env_switches(), scratch_floats=tr.n_scratch)
    train = _lib.encoder_plan_train(tr.lay, B, L, tr._train_mode, _lib.env_switches())[0]
    if L == 8:
        assert (fwd, bwd) == GENERIC and train == ""
    elif switch is None:
        assert train.startswith("srfrd::encoder_train_ragged_kernel<") and tr.train_launch
    else:
        assert train == "" and fwd.startswith("srfrd::encoder_fwd_kernel<50,64,8,50,") and bwd.startswith("srfrd::encoder_bwd_slots_kernel<50,50,")


class _Run:
    """one trainer on its own model: the state after every step"""

    def __init__(self, kind, B, L, lazy, graph, bf16=False, switch=None, **kw):
        self.model = _model(kind, L, bf16)
        self.tr = srfrd_amd.FusedTrainer(self.model, B, L, seed=SEED, use_graph=graph, deterministic=True, lazy_table=lazy, **kw)
        assert self.tr.lazy_table is bool(lazy) and self.tr.deterministic
        _assert_plan(self.tr, kind, B, L, switch)
        self.lay = self.tr.lay
        self.snaps = [self.snap(None)]

    def snap(self, loss):
        torch.cuda.synchronize()
        nt, d, tr = self.lay.n_table, self.lay.d_item, self.tr
        out = {"table": self.model._flat[:nt].view(-1, d), "m_table": tr.m[:nt].view(-1, d), "v_table": tr.v[:nt].view(-1, d),
               "dense": self.model._flat[tr.n_tab:], "m_dense": tr.m[tr.n_tab:], "v_dense": tr.v[tr.n_tab:],
               "flat": self.model._flat, "m": tr.m, "v": tr.v}
        out = {k: t.detach().cpu().clone() for k, t in out.items()}
        if loss is not None:
            out["loss"] = loss.detach().cpu().clone()
        if self.model.bf16_table:
            out["shadow"] = self.model._table16.detach().cpu().clone().view(-1, d)
        return out

    def step(self, batch):
        loss = self.tr.step(None, *[x.cuda() for x in batch])
        self.snaps.append(self.snap(loss))
        return self.snaps[-1]


ROW_NAMES = ("table", "m_table", "v_table")


def _two_steps(kind, B, L, switch, bf16=False):
    (b1, b2), t2, both, only1, never = _two_batches(B, L)
    with _env(switch):
        dense = _Run(kind, B, L, False, False, bf16, switch)
        lazy = _Run(kind, B, L, True, False, bf16, switch)
        lazy_g = _Run(kind, B, L, True, True, bf16, switch)
        init = lazy.snaps[0]
        for k in ("flat", "m", "v"):
            _same(f"initial {k}", init[k], dense.snaps[0][k])
        assert not bool(init["m"].any()) and not bool(init["v"].any())
        # step 1: zero moments - dense Adam leaves an untouched row where it is, so the two optimizers agree everywhere
        d1, l1, g1 = dense.step(b1), lazy.step(b1), lazy_g.step(b1)
        for k in ("flat", "m", "v", "loss"):
            _same(f"step 1: {k}, lazy against dense", l1[k], d1[k])
        d2, l2, g2 = dense.step(b2), lazy.step(b2), lazy_g.step(b2)
    for s, (a, b) in enumerate(((l1, g1), (l2, g2)), 1):
        for k in a:
            _same(f"step {s}: {k}, graph against eager", b[k], a[k])
    assert torch.isfinite(l2["flat"]).all() and torch.isfinite(l2["loss"]).all()
    _same("step 2: loss", l2["loss"], d2["loss"])                       # (its forward read step 1's parameters: the same ones)
    for k in ("dense", "m_dense", "v_dense"):
        _same(f"step 2: {k}", l2[k], d2[k])
        assert not torch.equal(l2[k], l1[k])
    for k in ROW_NAMES:
        _same(f"step 2: {k}, rows touched in step 2", l2[k][t2], d2[k][t2])
        _same(f"step 2: {k}, never-touched rows", l2[k][never], d2[k][never])
        _same(f"step 2: {k}, never-touched rows against the start", l2[k][never], init[k][never])
        _same(f"step 2: {k}, rows of step 1 alone keep their bits in the lazy trainer", l2[k][only1], l1[k][only1])
    assert not bool(l2["m_table"][never].any()) and not bool(l2["v_table"][never].any())
    assert not torch.equal(l2["table"][both], l1["table"][both])
    # ... and the dense optimizer moved them by their momentum: a dense step passed off as lazy fails here
    assert bool((_bits(l2["table"][only1]) != _bits(d2["table"][only1])).any())
    assert bool((_bits(l2["m_table"][only1]) != _bits(d2["m_table"][only1])).any())
    for run in (lazy, lazy_g):
        assert not bool(run.tr.grad[:run.tr.n_tab].any()), "the table's slice of the gradient was written"
    return dense, lazy


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_two_steps_against_the_dense_deterministic_trainer(geometry):
    _two_steps(*GEOMETRIES[geometry])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. six steps, teacher-forced
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [False, True], ids=["constant", "cosine_warmup2"])
@pytest.mark.parametrize("geometry", ["SASRec-B3-L8", "SRFRN-B5-L50"])
def test_six_teacher_forced_steps(geometry, schedule):
    kind, B, L, _ = GEOMETRIES[geometry]
    kw = dict(lr_schedule="cosine", warmup_steps=2, total_steps=6) if schedule else {}
    lazy = _Run(kind, B, L, True, True, **kw)
    dense = _Run(kind, B, L, False, False, **kw)
    assert (lazy.tr.opts is not None) == schedule
    for s in range(6):
        batch = _batch((40, 200, 90, 15, 150, 60)[s], B, L, 20 + s)
        touched = _rows(batch)
        rest = torch.ones(ITEMS + 1, dtype=torch.bool)
        rest[touched] = False
        assert bool(rest[1:].any())
        dense.model.load_state_dict(lazy.model.state_dict())
        dense.tr.load_state_dict(lazy.tr.state_dict())
        before = lazy.snaps[-1]
        a, b = lazy.step(batch), dense.step(batch)
        _same(f"step {s + 1}: loss", a["loss"], b["loss"])
        for k in ("dense", "m_dense", "v_dense"):
            _same(f"step {s + 1}: {k}", a[k], b[k])
        for k in ROW_NAMES:
            _same(f"step {s + 1}: {k}, touched rows", a[k][touched], b[k][touched])
            _same(f"step {s + 1}: {k}, untouched rows keep their bits", a[k][rest], before[k][rest])
        if s >= 1:        # rows with momentum that this batch did not name: the dense step decays it (and, wherever the rate
            # is not zero - the cosine schedule ends at 0 - moves the row)
            assert bool((_bits(a["m_table"][rest]) != _bits(b["m_table"][rest])).any())
    assert lazy.tr.steps_done == 6 and torch.isfinite(lazy.snaps[-1]["flat"]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the bf16 table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", ["SASRec-B3-L8", "SASRec-B5-L50"])
def test_bf16_table_two_steps_shadow_and_topk(geometry):
    kind, B, L, switch = GEOMETRIES[geometry]
    dense, lazy = _two_steps(kind, B, L, switch, bf16=True)
    for run in (dense, lazy):
        for s, snap in enumerate(run.snaps):
            _same(f"step {s}: the shadow is bf16(fp32 table) on every row", snap["shadow"], _bf16_rne(snap["table"]))
    assert not torch.equal(lazy.snaps[2]["shadow"], lazy.snaps[0]["shadow"])
    # the stepped model ranks as a model freshly loaded from its state_dict does
    seq, rsq = (x.cuda() for x in _batch(ITEMS, B, L, 7)[:2])
    shadow = lazy.model._table16.clone()
    lazy.model.eval()
    fresh = _model(kind, L)
    fresh.load_state_dict(lazy.model.state_dict())
    fresh.use_bf16_table().eval()
    with torch.no_grad():
        idx, val = lazy.model.topk(None, seq, rsq, k=10)
        idx_f, val_f = fresh.topk(None, seq, rsq, k=10)
    _same("topk indices", idx.cpu(), idx_f.cpu())
    _same("topk values", val.cpu(), val_f.cpu())
    _same("the trainer's shadow against the fresh model's", shadow.cpu(), fresh._table16.cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. resume
# ---------------------------------------------------------------------------------------------------------------------------------
def test_resume_is_the_uninterrupted_run_and_dense_checkpoints_load():
    kind, B, L, _ = GEOMETRIES["SASRec-B3-L8"]
    batches = [_batch((120, 60, 200, 30, 90, 150)[s], B, L, 40 + s) for s in range(6)]
    whole = _Run(kind, B, L, True, True)
    for b in batches[:3]:
        whole.step(b)
    model_sd = {k: v.detach().cpu().clone() for k, v in whole.model.state_dict().items()}
    optim_sd = whole.tr.state_dict()
    assert set(optim_sd) == {"state", "param_groups", "srfrd"} and "lazy" not in str(sorted(optim_sd["srfrd"]))
    for b in batches[3:]:
        whole.step(b)
    resumed = _Run(kind, B, L, True, True)
    resumed.model.load_state_dict(model_sd)
    resumed.tr.load_state_dict(optim_sd)
    assert resumed.tr.lazy_table and resumed.tr.steps_done == 3
    for s, b in enumerate(batches[3:], 4):
        got, want = resumed.step(b), whole.snaps[s]
        for k in ("loss", "flat", "m", "v"):
            _same(f"step {s} after the resume: {k}", got[k], want[k])
    # a dense trainer's checkpoint into a lazy trainer, and back
    dense = _Run(kind, B, L, False, False)
    for b in batches[:2]:
        dense.step(b)
    lazy = _Run(kind, B, L, True, False)
    lazy.model.load_state_dict(dense.model.state_dict())
    lazy.tr.load_state_dict(dense.tr.state_dict())
    before = lazy.snap(None)
    for k in ("flat", "m", "v"):
        _same(f"loaded {k}", before[k], dense.snaps[-1][k])
    after = lazy.step(batches[3])
    touched = _rows(batches[3])
    rest = torch.ones(ITEMS + 1, dtype=torch.bool)
    rest[touched] = False
    assert torch.isfinite(after["flat"]).all() and lazy.tr.steps_done == 3
    for k in ROW_NAMES:
        _same(f"{k}: untouched rows", after[k][rest], before[k][rest])
        assert not torch.equal(after[k][touched], before[k][touched])
    back = _Run(kind, B, L, False, False)
    back.model.load_state_dict(lazy.model.state_dict())
    back.tr.load_state_dict(lazy.tr.state_dict())
    assert back.tr.steps_done == 3 and not back.tr.lazy_table
    assert torch.isfinite(back.step(batches[4])["flat"]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. skewed barriers
# ---------------------------------------------------------------------------------------------------------------------------------
def _one_lazy_step():
    kind, B, L, _ = GEOMETRIES["SASRec-B5-L50"]
    run = _Run(kind, B, L, True, False)
    return run.step(_batch(120, B, L, 0))


@pytest.mark.parametrize("lib", ["even", "odd"])
def test_same_bits_under_skewed_barriers(lib):
    from tests import skew_cases as S
    want_kernel = _check_kernel("big", 50, True)
    want_step = _one_lazy_step()
    mask = S.libraries()[lib][2]
    with S.use(lib) as rec:
        assert rec._handle.srfrd_skew_mask(None, None) == mask != 0
        got_kernel = _check_kernel("big", 50, True)
        got_step = _one_lazy_step()
    assert {"srfrd_table_reduce_adam", "srfrd_adam_pack_step", "srfrd_encoder_train_ranked"} <= rec.called
    for k in want_kernel:
        _same(f"kernel under {lib}: {k}", got_kernel[k], want_kernel[k])
    for k in want_step:
        _same(f"step under {lib}: {k}", got_step[k], want_step[k])
