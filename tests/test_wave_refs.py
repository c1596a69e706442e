"""CPU side of tests/test_gpu_wave_fp64.py (tests/wave_refs.py): the conditions its comparisons rest on, on the oracle and the
host-only plan alone - the keep-all dropout rate computes the function of dropout 0, the tiled batch's fp64 gradient is the
base batch's, the bounds reject a gradient with one copy dropped or counted twice, which the old absolute bar accepts, and the
tiled cases put every kernel family, and every read-modify-write instantiation, on a grid below half the batch."""
import re

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests import grad_refs as G
from tests import test_bf16_family_cover as C
from tests import test_gpu_bf16_families as F
from tests import wave_refs as W
from tests.test_encoder_plan import MODES, N_CU, _layout, _rows

cases = pytest.mark.parametrize("c", W.CASES, ids=W.case_ids())
ONE_PER_KIND = ("a", "c", "b", "f")       # SASRec, SRFR, SRFRN, SRFU_B


# ---------------------------------------------------------------------------------------------------------------------------
# KEEP_ALL_P
# ---------------------------------------------------------------------------------------------------------------------------
def test_keep_all_rate_keeps_every_hash_and_scales_by_one():
    p = W.KEEP_ALL_P
    assert 0.0 < p and O.drop_threshold(p) == 0 and int(np.uint32(p * 4294967296.0)) == 0       # (uint32_t)(p * 2^32)
    assert np.float32(1.0 / (1.0 - p)) == np.float32(1.0)
    mask = O.keep_mask(123, O.site_ffn1(1), 5, 7, 50, 50, p)
    assert bool((mask == 1.0).all())


@pytest.mark.parametrize("cid", ONE_PER_KIND)
def test_keep_all_training_mode_is_the_eval_function_in_bits(cid):
    c = G.BY_ID[cid]
    cfg = F.cfg_of(c, bf16=False, dropout=W.KEEP_ALL_P)
    sd, batch = G.weights(cid), W.base_batch(c)
    assert {G.BY_ID[i].kind for i in ONE_PER_KIND} == {"SASRec", "SRFR", "SRFRN", "SRFU_B"}
    with torch.no_grad():
        ev, tr = O.forward(cfg, sd, *batch), O.forward(cfg, sd, *batch, train=True, seed=123)
    assert all(torch.equal(a, b) for a, b in zip(ev, tr))
    (l0, g0, *_), (l1, g1, *_) = O.grads_of(cfg, sd, batch), O.grads_of(cfg, sd, batch, train=True, seed=123)
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
@cases
def test_tiled_fp64_gradient_is_the_base_gradient(c):
    """at k = 3 (the mean over targets does not see the copies; k enters nowhere else)"""
    base = G.reference(c.id, W.MODE)
    g = G.fp64_grads(base.cfg, base.sd, W.repeat(base.batch, 3))
    for n in base.g64:
        assert G.row_errors(g[n], base.g64[n]) < 1e-12 and G.zero_row_leaks(g[n], base.g64[n]) == 0, n


def test_tiled_batches_are_copies_above_twice_the_grid():
    assert len(W.CASES) == len(G.DEPTH2_CASES) + len(W.TWINS) and all(c in G.ALL_CASES for c in W.CASES)
    assert {W.MODE} == {"autograd"} and all((c.id, W.MODE) in G.SEEDS for c in W.CASES)
    for c in W.CASES:
        batch, k, B = W.tiled(c)
        base = W.base_batch(c)
        g = max(W.grids(c))
        assert B == c.B * k and 2 * g + 1 <= B < 2 * g + 1 + c.B and all(t.shape[0] == B for t in batch), c.id
        for j in (0, 1, k - 1):
            assert all(torch.equal(t[j * c.B:(j + 1) * c.B], t0) for t, t0 in zip(batch, base)), c.id
    assert sorted({W.copies(c)[1] for c in W.CASES}) == [515, 1026, 1032, 1037]


# ---------------------------------------------------------------------------------------------------------------------------
# bounds and sharpness
# ---------------------------------------------------------------------------------------------------------------------------
def test_bound_rule():
    assert W.bound_wave("x", 3.6e-6, 1030) == W.bound_wave("x", W.CAP / 4, 1030) == G.CAP == 1e-4
    assert W.bound_wave("x", 3.3e-5, 1026) == 4 * 3.3e-5 and W.bound_wave("x", 7.1e-5, 515) == 4 * 7.1e-5
    assert W.bound_wave("x", 2e-4, 1026) == 1 / 2052                     # never so wide that a dropped copy would pass
    assert G.bound(1.0, clamp=True) == W.CAP                              # the clamp of grad_refs' OVER_CAP jobs
    assert set(W.EXCEPTIONS) <= {c.id for c in W.CASES if c.kind in ("SRFR", "SRFRN")}


@cases
def test_bounds_reject_a_dropped_and_a_doubled_copy(c):
    """the base g64 scaled by 1 - 1 / B (one copy's whole contribution dropped) and by 1 + 1 / B (one copy counted twice):
    every tensor misses its bound by SHARP (an exception tensor by SHARP_EXC), and the fp32 oracle on the tiled batch is inside
    every bound.  wave_refs.reference asserts the exception list where it computes e32_tiled."""
    ref = W.reference(c.id)
    assert ref.B == W.copies(c)[1] and W.exceptions_of(ref) == tuple(W.EXCEPTIONS.get(c.id, ()))
    assert not any(G.failures(f) for f in W.compare(ref.g32, ref).values())
    old = 0.0
    for s in (1.0 - 1.0 / ref.B, 1.0 + 1.0 / ref.B):
        wrong = {n: v * s for n, v in ref.g64.items()}
        figs = W.compare(wrong, ref)
        for n, f in figs.items():
            assert bool((ref.g64[n] != 0).any()), n                       # (no tensor without a gradient: every one is held)
            need = W.SHARP_EXC if n in W.EXCEPTIONS.get(c.id, ()) else W.SHARP
            assert f["err"] >= need * f["bound"], (c.id, s, n, f["err"] / f["bound"])
        old = max(old, max(f["old"] for f in figs.values()))
    print(f"case {c.id} B = {ref.B}: old metric of the wrong gradients {old:.2e}")
    assert (old < G.OLD_BAR) == (c.id not in W.OLD_BAR_REJECTS), (c.id, old)


def test_old_bar_accepts_the_wrong_gradients_at_most_cases():
    assert W.OLD_BAR_REJECTS <= {c.id for c in W.CASES} and len(W.OLD_BAR_REJECTS) * 3 < len(W.CASES)


def test_bit_comparison_counts_every_differing_element_of_every_copy():
    """the GPU file's own helpers, on the host: a NaN differs, the last copy counts, a checkpoint row in front of the first
    live position does not (an interior pad does)"""
    from tests import test_gpu_wave_fp64 as T
    base = torch.arange(24.0).reshape(2, 3, 4)
    x = base.repeat(3, 1, 1)
    assert T._differing(x, base) == 0
    x[5, 2, 3] += 1.0
    x[1, 0, 0] = float("nan")
    assert T._differing(x, base) == 2 and T._differing(x[:2], base) == 1
    rows = T._live_rows(torch.tensor([[0, 7, 0], [0, 0, 0]]))
    assert rows.tolist() == [[False, True, True], [False, False, False]]
    ck = torch.zeros(2, 2, 3, 4)                            # (B0, blocks, L, D)
    y = ck.repeat(2, 1, 1, 1)
    y[2, 1, 0, 0] = y[2, 1, 2, 3] = y[3, 0, 2, 0] = 1.0     # a leading pad, the interior pad, an all-pad sequence
    assert T._differing(y, ck) == 3 and T._differing(y, ck, rows) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# cover
# ---------------------------------------------------------------------------------------------------------------------------
LAUNCHES = ("eval", "last", "train", "autograd", "fused")
_FLAG = re.compile(r",(true|false)>$")


def _key(name):
    """(family key of test_bf16_family_cover - function, form - , read-modify-write flag | None)"""
    m = _FLAG.search(name)
    if name.startswith(W.TRAIN_KERNEL):
        return "srfrd::encoder_train_ragged_kernel", m.group(1)
    return C.family_key(name), m.group(1) if m else None


def _case_names(c, B):
    """every name the plan answers the GPU file's launches of one case at batch B, the train kernel included"""
    lay, sw = W.layout_of(c), W.switches_of(c)
    out = set()
    for launch in LAUNCHES:
        sf, sb = F.case_scratch(lay, B, c.L, "autograd" if launch == "train" else launch)
        out.update(n for n in W.planned(lay, B, c.L, launch, sw, N_CU, sf, sb) if n)
    name = W.train_plan(lay, B, c.L, sw, N_CU, max(_lib.scratch_floats(lay, B, c.L)))[0]
    return out | ({name} if name else set())


@cases
def test_case_names_are_the_plans_at_the_tiled_batch(c):
    lay, sw = W.layout_of(c), W.switches_of(c)
    k, B = W.copies(c)
    for launch in LAUNCHES:
        sf, sb = F.case_scratch(lay, B, c.L, "autograd" if launch == "train" else launch)
        assert W.planned(lay, B, c.L, launch, sw, N_CU, sf, sb) == W.names(c)[launch], (c.id, launch)
        if launch in F._plan_bits():
            fbits, bbits = F._plan_bits()[launch]
            grids = [_lib.encoder_plan(lay, B, c.L, fbits, sw, N_CU, sf)[0][1]]
            grids += [_lib.encoder_plan(lay, B, c.L, bbits, sw, N_CU, sb)[1][1]] if bbits is not None else []
            assert all(0 < 2 * g < B for g in grids) and max(grids) <= max(W.grids(c)), (c.id, launch, grids)
    # the untiled launches the tiled ones are compared with run the same instantiations, but for the flag
    assert {F.strip_rmw(n) for n in _case_names(c, B)} == {F.strip_rmw(n) for n in _case_names(c, c.B)}, c.id
    name, grid = W.train_plan(lay, B, c.L, sw, N_CU, max(_lib.scratch_floats(lay, B, c.L)))
    assert (c.id in W.TRAIN_KERNEL_IDS) <= (name.startswith(W.TRAIN_KERNEL) and name.endswith(",true>") and 2 * grid < B)


def test_tiled_cases_reach_every_family_and_every_read_modify_write_instantiation():
    """every (family, form, flag) key the plan produces over test_encoder_plan's rows at B = 600 - more sequences than either
    grid at 256 CUs - is run by a tiled case; so is every ``<..., true>`` instantiation the plan can answer the cases' own
    layouts, on both sides of the kind variant"""
    targets = set()
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        if mname in C.RUN_MODES and B == 600:
            lay = _layout(kind, di, df, nl, heads)
            (f, gf), (b, gb) = _lib.encoder_plan(lay, B, L, MODES[mname], _lib.SWITCHES[sw] if sw else 0, N_CU,
                                                 max(_lib.scratch_floats(lay, B, L)))
            assert (not f or gf < B) and (not b or gb < B)
            targets.update(_key(n) for n in (f, b) if n)
    assert {k for k, _ in targets} == C.TARGETS
    by_case = {c.id: _case_names(c, W.copies(c)[1]) for c in W.CASES}
    produced = {_key(n) for names in by_case.values() for n in names}
    assert targets <= produced, sorted(targets - produced)
    assert not any(flag == "false" for _, flag in produced)
    # every family that carries the flag: an SRFRN case and one without a fake channel (the kind variant selects the gather)
    rmw = {}
    for c in W.CASES:
        for n in by_case[c.id]:
            if n.endswith(",true>"):
                rmw.setdefault(_key(n)[0], set()).add(c.kind)
    assert set(rmw) == {"srfrd::encoder_bwd_slots_kernel<L=50>", "srfrd::encoder_bwd_slots_kernel<L=100>",
                        "srfrd::encoder_bwd_chunks_kernel", "srfrd::encoder_bwd_ragged_kernel",
                        "srfrd::encoder_train_ragged_kernel"}
    for key, kinds in rmw.items():
        assert "SRFRN" in kinds and kinds & {"SASRec", "SRFU_B"}, (key, kinds)
    # and the names the GPU file asserts are all of them
    asserted = {n for c in W.CASES for pair in W.names(c).values() for n in pair if n}
    assert {n for names in by_case.values() for n in names if not n.startswith(W.TRAIN_KERNEL)} == asserted
