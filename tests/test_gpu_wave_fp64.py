"""-m gpu, fp32 item table: a workgroup's second and third sequence, held to the fp64 oracle and to the first pass's own bits
(tests/wave_refs.py: batches, reference, kernel names, bounds; tests/test_wave_refs.py: their CPU side).

Every case of wave_refs.CASES runs its admissible batch k times along the batch axis, B = B0 k just above twice the larger
grid of the device, so that every persistent workgroup loops twice and some three times.  Before each launch the planned kernel
names are asserted at that B with the read-modify-write flag ON the name (wave_refs.names), and that the grid is below B / 2.

  A  forward, in bits (no tolerance).  Nothing per sequence is reduced across sequences, so copy j of the tiled launch must equal
     the untiled B0-sequence launch - one sequence per workgroup, the path the rest of the suite pins - element for element:
     hidden state and both logits in the eval, last-position and training launches, and in the training launch the
     checkpoints save_x / save_h1 on the rows from a sequence's first live position on (rows in front of it belong to tiles the
     ragged kernels never compute, and the module path hands them uninitialised memory; save_aux holds kernel-specific
     padding of the same kind and is read back by B and C instead).  The training launch runs with KEEP_ALL_P, and with
     p = 0.5, where the copies differ: rows [j B0, (j + 1) B0) of the tiled launch at seq0 = 0 against the untiled launch at
     seq0 = j B0.  DESIGN.md documents no output whose bits depend on a sequence's place in the batch: a difference is a bug.
  B  backward with real masks, device against device: ``_launch_fwd`` / ``_launch_bwd`` with p = 0.5 and fixed upstream
     gradients 0.3 / -0.2.  The flat gradient of ONE tiled launch against the sum, in fp64 on the host, of the k untiled
     launches at seq0 = j B0.  A backward that regenerates its second sequence's masks from the wrong index fails here and
     nowhere else.  Every forward of the k launches is compared in bits on the way, so no ReLU unit differs between the sides.
  C  gradients against the fp64 oracle; the reference is the BASE batch's g64 (the loss is a mean over targets).
     autograd: ``model.train()``, dropout 0, ``loss.backward()``.  fused: one ``FusedTrainer.step`` with
     ``model.dropout_rate = KEEP_ALL_P`` - the training instantiations, masks on, the function of dropout 0 - both scatter
     modes, gradients and their squares read from the moments, the loss against the base fp64 loss, the step's per-sequence
     outputs (loss partials, logits on targets, live hidden rows) equal between the copies; at the default geometry through the
     one-launch train kernel ``<..., true>`` and as two launches.

Bounds: wave_refs.bound_wave - 1e-4 of the row's norm, the clamp of grad_refs' OVER_CAP jobs; zero rows exactly zero; the K
bias under its own rule; the exception tensors of wave_refs.EXCEPTIONS under min(4 e32_tiled, 1 / (2 B)).
profiles/wave_fp64_errors.json holds the measured figures (tools/grad_fp64_report.py --wave calls the run_* functions below).
"""
import pytest
import torch

from tests import fwd_refs as R
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests import wave_refs as W

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", W.CASES, ids=W.case_ids())
scatter = pytest.mark.parametrize("det", [True, False], ids=["deterministic", "atomics"])
SEED = 0xBEEF                 # the dropout seed word of the module-path launches (A with p = 0.5, B)
D_PL, D_NL = 0.3, -0.2


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ref(c):
    return W.reference(c.id, _n_cu())


def _model(c, ref, setenv, dropout=0.0):
    from tests.gpu_util import build_model
    if c.switch:
        setenv(c.switch, "1")
    model = build_model(ref.cfg, {k: v.clone() for k, v in ref.sd.items()})
    assert not model.bf16_table and model.dropout_rate == 0.0
    model.dropout_rate = dropout
    return model


def _assert_plan(c, model, B, launch, scratch=None):
    """test_gpu_bf16_families._assert_plan at the tiled B: full names, flag included, and both grids under B / 2"""
    from srfrd_amd import _lib
    if c.switch:
        assert _lib.env_switches() == _lib.SWITCHES[c.switch]
    sf, sb = F.case_scratch(model.layout, B, c.L, launch) if scratch is None else (scratch, scratch)
    got = W.planned(model.layout, B, c.L, launch, _lib.env_switches(), _n_cu(), sf, sb)
    assert got == W.names(c)[launch], (c.id, launch, B, got, W.names(c)[launch])
    assert 2 * max(W.grids(c, _n_cu())) < B


def _ids(model, batch):
    from tests.gpu_util import cuda
    return model._prep(*cuda(*batch))


def _live_rows(seq):
    """(B, L) bool: the positions from a sequence's first live one on"""
    return (seq != 0).cumsum(dim=1) > 0


def _differing(x, base, rows=None):
    """elements of `x` ((n B0, ...): n copies) that differ from `base` ((B0, ...)), every copy counted; a NaN differs from
    everything.  rows: (B0, L) bool - only these positions of a (B0, [blocks,] L, D) checkpoint"""
    B0 = base.shape[0]
    ne = x.reshape(-1, *base.shape) != base.unsqueeze(0)
    if rows is not None:
        rows = rows.to(x.device)
        mask = rows[:, None, :, None] if base.dim() == 4 else rows[:, :, None]
        ne = ne & mask.unsqueeze(0)
    assert x.shape[0] % B0 == 0
    return int(ne.sum())


FWD_OUTPUTS = ("hidden", "pos_logits", "neg_logits")
CKPTS = ("save_x", "save_h1")


def _fwd_differing(out, base, seq0_rows):
    """{output: differing elements} of a training launch's outputs and checkpoints"""
    d = {n: _differing(out[n], base[n]) for n in FWD_OUTPUTS}
    d.update({n: _differing(out[n], base[n], seq0_rows) for n in CKPTS})
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# A: forward, in bits
# ---------------------------------------------------------------------------------------------------------------------------
def run_forward_bits(c, mode, setenv):
    """mode "eval" | "last" | "train" (KEEP_ALL_P) | "masks" (p = 0.5) -> {output: number of differing elements}"""
    ref = _ref(c)
    model = _model(c, ref, setenv)
    k, B, B0 = ref.k, ref.B, c.B
    base_batch = W.base_batch(c)
    ids, ids0 = _ids(model, ref.batch), _ids(model, base_batch)
    if mode == "eval":
        model.eval()
        _assert_plan(c, model, B, "eval")
        with torch.no_grad():
            out = dict(zip(FWD_OUTPUTS, model(None, *ids)))
            base = dict(zip(FWD_OUTPUTS, model(None, *ids0)))
        return {n: _differing(out[n], base[n]) for n in FWD_OUTPUTS}
    if mode == "last":
        model.eval()
        _assert_plan(c, model, B, "last")
        with torch.no_grad():
            return {"last_state": _differing(model._launch_fwd_last(ids[0], ids[1]), model._launch_fwd_last(ids0[0], ids0[1]))}
    model.train()
    _assert_plan(c, model, B, "train")
    rows = _live_rows(base_batch[0])
    if mode == "train":
        out = model._launch_fwd(*ids, W.KEEP_ALL_P, SEED, save=True)
        base = model._launch_fwd(*ids0, W.KEEP_ALL_P, SEED, save=True)
        return _fwd_differing(out, base, rows)
    assert mode == "masks"
    out = model._launch_fwd(*ids, W.P_MASKS, SEED, save=True)
    total = dict.fromkeys(FWD_OUTPUTS + CKPTS, 0)
    for j in sorted({0, 1, k // 2, k - 1}):
        base = model._launch_fwd(*ids0, W.P_MASKS, SEED, save=True, seq0=j * B0)
        part = {n: out[n][j * B0:(j + 1) * B0] for n in total}
        for n, d in _fwd_differing(part, base, rows).items():
            total[n] += d
    # the copies do differ under real masks: a launch that ignored the sequence index would pass everything above
    assert not torch.equal(out["hidden"][:B0], out["hidden"][B0:2 * B0])
    return total


@pytest.mark.parametrize("mode", ["eval", "last", "train", "masks"])
@cases
def test_every_copy_of_the_forward_equals_the_untiled_launch_in_bits(c, mode, monkeypatch):
    diff = run_forward_bits(c, mode, monkeypatch.setenv)
    print(f"case {c.id} {mode}: differing elements {diff}")
    assert not any(diff.values()), (c.id, mode, diff)


# ---------------------------------------------------------------------------------------------------------------------------
# B: backward with real masks, device against device
# ---------------------------------------------------------------------------------------------------------------------------
def _by_tensor(model, gflat):
    out = {}
    for name, prm in model.named_parameters():
        off = next(o for q, o in model._slots if q is prm)
        out[name] = gflat[off:off + prm.numel()].view(prm.shape).detach().cpu().double()
    return out


def _fwd_bwd(model, ids, seq0):
    out = model._launch_fwd(*ids, W.P_MASKS, SEED, save=True, seq0=seq0)
    dpl = torch.full_like(out["pos_logits"], D_PL)
    dnl = torch.full_like(out["neg_logits"], D_NL)
    return out, model._launch_bwd(*ids, W.P_MASKS, SEED, out, None, dpl, dnl, seq0=seq0)


def run_masks(c, setenv):
    """-> ({tensor: figures} of the tiled launch's gradient against the fp64 sum of the untiled launches', {output: differing
    forward elements over all k copies})"""
    ref = _ref(c)
    model = _model(c, ref, setenv).train()
    k, B, B0 = ref.k, ref.B, c.B
    _assert_plan(c, model, B, "train")
    from srfrd_amd import _lib
    sb = F.case_scratch(model.layout, B, c.L, "autograd")[1]
    bits = F._plan_bits()["autograd"][1] | _lib.PLAN_DROPOUT
    assert _lib.encoder_plan(model.layout, B, c.L, bits, _lib.env_switches(), _n_cu(), sb)[1][0] == W.names(c)["autograd"][1]
    base_batch = W.base_batch(c)
    ids, ids0 = _ids(model, ref.batch), _ids(model, base_batch)
    rows = _live_rows(base_batch[0])
    out, gflat = _fwd_bwd(model, ids, 0)
    total = torch.zeros(gflat.numel(), dtype=torch.float64)
    diff = dict.fromkeys(FWD_OUTPUTS + CKPTS, 0)
    for j in range(k):
        base, g = _fwd_bwd(model, ids0, j * B0)
        total += g.detach().cpu().double()
        part = {n: out[n][j * B0:(j + 1) * B0] for n in diff}
        for n, d in _fwd_differing(part, base, rows).items():
            diff[n] += d
    return W.compare_sums(_by_tensor(model, gflat), _by_tensor(model, total), ref), diff


@cases
def test_masked_backward_of_the_tiled_launch_is_the_sum_of_the_untiled_ones(c, monkeypatch):
    figs, diff = run_masks(c, monkeypatch.setenv)
    assert not any(diff.values()), (c.id, diff)
    G.assert_holds(figs, f"case {c.id} masks, B = {_ref(c).B}")


# ---------------------------------------------------------------------------------------------------------------------------
# C: gradients against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------------
def run_autograd(c, setenv):
    """-> {tensor: grad_refs.tensor_figures} of p.grad after a training-mode forward and backward on the tiled batch"""
    from tests.gpu_util import cuda
    ref = _ref(c)
    G.assert_admissible(G.reference(c.id, W.MODE), f"case {c.id} base batch")
    model = _model(c, ref, setenv).train()
    _assert_plan(c, model, ref.B, "autograd")
    seq, rsq, pos, prs, neg, nrs = cuda(*ref.batch)
    _, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    F._bce(pl, nl, pos).backward()
    return W.compare({k: p.grad for k, p in model.named_parameters()}, ref)


def _copies_differing(tr, ref, B0):
    """the fused step's per-sequence outputs, copy j against copy 0: loss partials, logits where there is a target, hidden
    rows from the first live position on"""
    seq, pos = ref.batch[0][:B0], ref.batch[2][:B0]
    tgt = (pos != 0).to(tr.pl.device)
    rows = _live_rows(seq).to(tr.pl.device)
    d = {"loss_part": _differing(tr.loss_part, tr.loss_part[:B0])}
    for n, x in (("pos_logits", tr.pl), ("neg_logits", tr.nl)):
        d[n] = int(((x.reshape(-1, *tgt.shape) != x[:B0].unsqueeze(0)) & tgt.unsqueeze(0)).sum())
    d["hidden"] = int(((tr.hidden.reshape(-1, *tr.hidden[:B0].shape) != tr.hidden[:B0].unsqueeze(0)) & rows[None, :, :, None]).sum())
    return d


def run_fused(c, det, setenv, train_launch=True):
    """-> (figures of exp_avg / (1 - beta1), figures of exp_avg_sq / (1 - beta2) against g64^2, {output: elements that differ
    between the copies}) after one step with dropout KEEP_ALL_P"""
    import srfrd_amd
    from srfrd_amd import _lib
    from tests.gpu_util import cuda
    ref = _ref(c)
    model = _model(c, ref, setenv, dropout=W.KEEP_ALL_P).train()
    B = ref.B
    tr = srfrd_amd.FusedTrainer(model, batch_size=B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=det)
    tr.train_launch = train_launch
    _assert_plan(c, model, B, "fused", scratch=tr.n_scratch)
    if c.id in W.TRAIN_KERNEL_IDS:
        name, grid = _lib.encoder_plan_train(tr.lay, B, c.L, tr._train_mode, _lib.env_switches(), _n_cu(), tr.n_scratch)
        assert name.startswith(W.TRAIN_KERNEL) and name.endswith(",true>") and 2 * grid < B, (c.id, name, grid)
    loss = tr.step(None, *cuda(*ref.batch))
    assert bool(torch.isfinite(loss).all())
    # the loss of the tiled batch is the base batch's: the evaluation forward's fp64 loss at the base batch (keep-all masks)
    R.assert_loss_holds(loss.detach().cpu(), R.reference_at(c.id, "eval", G.SEEDS[c.id, W.MODE]), f"case {c.id} fused det={det}")
    g, g2 = G.fused_gradients(tr, model)
    return W.compare(g, ref), W.compare(g2, ref, squares=True), _copies_differing(tr, ref, c.B)


@cases
def test_autograd_gradients_of_later_passes_meet_the_fp64_oracle(c, monkeypatch):
    G.assert_holds(run_autograd(c, monkeypatch.setenv), f"case {c.id} autograd, B = {_ref(c).B}")


def _assert_fused(c, det, setenv, train_launch, what):
    figs, figs2, diff = run_fused(c, det, setenv, train_launch)
    print(f"case {c.id} {what} det={det}: elements differing between copies {diff}")
    assert not any(diff.values()), (c.id, diff)
    G.assert_holds(figs, f"case {c.id} {what} det={det}, B = {_ref(c).B}")
    G.assert_holds(figs2, f"case {c.id} {what} det={det} second moment")


@scatter
@cases
def test_fused_step_gradients_of_later_passes_meet_the_fp64_oracle(c, det, monkeypatch):
    _assert_fused(c, det, monkeypatch.setenv, True, "fused")


@scatter
@pytest.mark.parametrize("cid", W.TRAIN_KERNEL_IDS)
def test_two_launch_step_gradients_of_later_passes_meet_the_fp64_oracle(cid, det, monkeypatch):
    """the default geometry through srfrd_encoder_fwd_sched + srfrd_encoder_bwd_sched (the test above runs it through the
    one-launch train kernel)"""
    _assert_fused(G.BY_ID[cid], det, monkeypatch.setenv, False, "two launches")
