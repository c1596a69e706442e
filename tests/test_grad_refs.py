"""CPU side of the fp64 gradient checks (tests/grad_refs.py, tests/test_gpu_grad_fp64.py): the cases' inputs are admissible on
the oracle alone, their kernel names and family coverage hold on the host-only plan, the fp64 oracle is the REFERENCE's
gradient (the golden fixtures), and the metric rejects the wrong gradients the old absolute bar accepts."""
import pytest
import torch

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests import grad_refs as G
from tests import test_bf16_family_cover as C
from tests import test_gpu_bf16_families as F
from tests.helpers import HEAD_CASES, KINDS, golden_cfg, load_golden, sub
from tests.test_encoder_plan import N_CU, _layout, _rows

JOBS = [(c.id, mode, 0.0) for c in G.ALL_CASES for mode in ("autograd", "fused")] + [(G.L2_ID, "fused", G.L2_EMB)]


@pytest.mark.parametrize("cid,mode,l2", JOBS, ids=[f"{cid}-{mode}" + ("-l2" if l2 else "") for cid, mode, l2 in JOBS])
def test_case_inputs_are_admissible(cid, mode, l2):
    """on the oracle alone (grad_refs.assert_admissible; the GPU tests assert it again where they compute their bounds), and the
    fp32 oracle itself inside its bound"""
    ref = G.reference(cid, mode, l2)
    G.assert_admissible(ref, f"case {cid} {mode}")
    assert all(G.bound(e, ref.clamp) >= G.R_MIN and (not ref.clamp or G.bound(e, True) <= G.CAP) for e in ref.e32.values())
    figs = G.compare(ref.g32, ref)
    assert not any(G.failures(f) for f in figs.values())
    assert any("kbias" in f for f in figs.values()) == (l2 == 0.0)


def test_seed_table_is_complete_and_batches_have_their_shape():
    assert set(G.SEEDS) == {(c.id, m) for c in G.ALL_CASES for m in ("autograd", "fused")}
    assert len(G.BY_ID) == len(G.ALL_CASES) and all(5 <= c.B <= 17 for c in G.ALL_CASES)
    seq, _, pos, _, neg, _ = G.tile_batch(3)
    assert tuple(int((row == 0).sum()) for row in seq) == tuple(t + (b == 3) for b, t in enumerate(G.TILE_PADS))
    on_pad = [b for b in range(17) if bool(((seq[b] == 0) & (pos[b] != 0)).any())]
    assert on_pad == [3, 5, 11] and bool((neg[5, :15] != 0).all())        # (3: its interior pad keeps its target)
    seq, _, pos, _, neg, _ = G.dup_batch(3)
    ids = torch.cat([seq.flatten(), pos.flatten(), neg.flatten()])
    top = int(torch.bincount(ids)[1:].argmax()) + 1
    assert top <= 8 and all(int((x == top).sum()) >= 12 for x in (seq, pos, neg))


def test_depth_jobs_over_the_cap_are_the_depth_8_ones_and_a_quarter_of_the_rest_at_most():
    """at depth 8 the condition 64 e32 <= CAP has no input (every job clamped at CAP - tighter than 64 e32, never wider); at
    depths 1 and 3 it has, and the jobs listed without one stay an exception"""
    jobs = {(c.id, m) for c in G.DEPTH for m in ("autograd", "fused")}
    deep = {(c.id, m) for c in G.DEPTH if c.blocks == 8 for m in ("autograd", "fused")}
    mine = G.OVER_CAP & jobs
    assert mine == G.DEPTH_OVER_CAP and deep <= mine and len(deep) == 10
    assert len(mine - deep) <= G.MAX_DEPTH_OVER_CAP == len(jobs - deep) // 4
    assert not any(k[0] in {c.id for c in G.DEPTH} for k in G.OVER_CAP - mine)       # (no head job at another depth)
    for cid, mode in sorted(deep):                  # the clamp acts on every depth-8 job: its bounds are CAP, not 64 e32
        ref = G.reference(cid, mode)
        assert ref.clamp and not G.under_cap(ref) and max(G.bound(e, True) for e in ref.e32.values()) == G.CAP, (cid, mode)


# ---------------------------------------------------------------------------------------------------------------------------
# names and families
# ---------------------------------------------------------------------------------------------------------------------------
def _lay(c):
    return _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)


@pytest.mark.parametrize("c", G.EXTRA, ids=[c.id for c in G.EXTRA])
def test_extra_case_names_are_the_plans(c):
    """(test_bf16_family_cover.test_case_names_are_the_plans holds CASES; the names carry no table flag)"""
    lay = _lay(c)
    for launch, names in (("autograd", c.autograd), ("fused", c.fused)):
        assert F.planned(lay, c.B, c.L, launch, 0, N_CU, *F.case_scratch(lay, c.B, c.L, launch)) == names, (c.id, launch)
    fused = _lib.PLAN_POS | _lib.PLAN_NEG | _lib.PLAN_CKPT | _lib.PLAN_LOSS | _lib.PLAN_FUSED_BCE
    assert _lib.encoder_plan_train(lay, c.B, c.L, fused)[0].startswith("srfrd::encoder_train_ragged_kernel<") == (c.L == 50)


def test_every_backward_family_is_reached_in_both_modes():
    """every backward key of test_bf16_family_cover.TARGETS that the plan can answer to an autograd launch is run by an
    autograd case, every one it can answer to a fused step by a fused case"""
    can = {"autograd": set(), "fused_p": set()}
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        if mname in can:
            can[mname].update(k for k in C._keys(_layout(kind, di, df, nl, heads), B, L, mname, sw) if "_bwd" in k)
    assert can["autograd"] | can["fused_p"] == {k for k in C.TARGETS if "_bwd" in k}
    run = {"autograd": {C.family_key(c.autograd[1]) for c in G.ALL_CASES},
           "fused_p": {C.family_key(c.fused[1]) for c in G.ALL_CASES}}
    for mname in can:
        assert can[mname] <= run[mname], (mname, sorted(can[mname] - run[mname]))


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 oracle is the reference's gradient
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,heads", [(k, 1) for k in KINDS] + list(HEAD_CASES))
def test_reference_gradients_meet_the_fp64_oracle(kind, heads):
    """the gradients the reference's own classes produced (tests/golden/, read by test_oracle_golden.py at 2e-6 absolute)
    under the metric and bound the kernels are held to.  The fixtures' inputs are what they are - no seed to choose, and on
    five of the nine the fp32 oracle's e32 is 1.6e-6 .. 1.9e-6 - so the bound is clamped at CAP as for the OVER_CAP jobs."""
    g, sd, batch = load_golden(kind, heads)
    cfg = golden_cfg(kind, heads=heads)
    g64 = G.fp64_grads(cfg, sd, batch)
    g32 = G.fp32_grads(cfg, sd, batch)
    gold = sub(g, "g/")
    assert set(gold) == set(g64)
    for k in g64:
        fig = G.tensor_figures(k, gold[k], g64[k], g32[k], cfg.D, clamp=True)
        assert fig["bound"] <= G.CAP and not G.failures(fig), (k, fig)


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------
SHARP = ("a", "autograd")         # SASRec, seq_len 50, B = 6
# the wrong gradients below that max|g - g_oracle| < 1e-4 accepts at that shape (the gap these tests close).  With 6 sequences
# a single item-row contribution is still 9e-3; it shrinks with the target count (2e-5 at the 300-sequence batches of
# tests/test_gpu_c4_c5.py), while the relative metric does not care.
OLD_BAR_ACCEPTS = ["tensor scaled by 1 + 4R", "element moved by 4R row norms"]


def _mutations(ref):
    cfg, (seq, _, pos, _, neg, _) = ref.cfg, ref.batch
    item, w = O.key_item(cfg), "attention_layers.0.in_proj_weight"
    counts = torch.bincount(torch.cat([seq.flatten(), pos.flatten(), neg.flatten()]), minlength=cfg.item_number + 1)
    counts[0] = 0
    fresh = lambda: {k: v.clone() for k, v in ref.g64.items()}

    m = fresh()
    m[w] *= 1 + 4 * G.bound(ref.e32[w])
    yield "tensor scaled by 1 + 4R", m

    m = fresh()
    r = int(m[w].norm(dim=1).argmax())
    m[w][r, 7] += 4 * G.bound(ref.e32[w]) * float(m[w][r].norm())
    yield "element moved by 4R row norms", m

    m = fresh()
    once = [int(i) for i in torch.where(counts == 1)[0] if bool((ref.g64[item][i] != 0).any())]
    m[item][once[0]] = 0
    yield "single contribution dropped", m

    m = fresh()
    i, j = once[1], once[2]
    m[item][[i, j]] = m[item][[j, i]]
    yield "two item rows swapped", m

    # the row with the most contributions, without the one of its first position as a positive target:
    # d loss / d pos_logit = (sigmoid(pos_logit) - 1) / count, times the hidden state of that position
    m = fresh()
    sd64 = {k: v.double() for k, v in ref.sd.items()}
    _, _, h, pl, _ = O.grads_of(cfg, sd64, ref.batch)
    top = int(torch.where(torch.bincount(pos.flatten(), minlength=cfg.item_number + 1)[1:] > 0, counts[1:], 0).argmax()) + 1
    b, t = (int(x[0]) for x in torch.where(pos == top))
    m[item][top] -= (torch.sigmoid(pl[b, t]) - 1) / int((pos != 0).sum()) * h[b, t]
    assert int(counts[top]) >= 3
    yield "most-used row without one of its targets", m

    yield "whole gradient doubled", {k: 2 * v for k, v in ref.g64.items()}


def test_metric_rejects_what_the_old_bar_accepts():
    ref = G.reference(*SHARP)
    assert ref.cfg.kind == "SASRec" and ref.cfg.max_len == 50
    assert not any(G.failures(f) for f in G.compare(ref.g64, ref).values())
    old_accepts = []
    for name, mut in _mutations(ref):
        figs = G.compare(mut, ref)
        bad = {k: G.failures(f) for k, f in figs.items() if G.failures(f)}
        old = max(float((mut[k] - ref.g32[k].double()).abs().max()) for k in mut)
        print(f"{name}: old metric {old:.2e}; rejected on {sorted(bad)}")
        assert bad, name
        if old < G.OLD_BAR:
            old_accepts.append(name)
    assert old_accepts == OLD_BAR_ACCEPTS
