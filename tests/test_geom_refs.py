"""CPU side of the width and head-split checks (tests/geom_refs.py, tests/test_gpu_geom_fp64.py), on the oracle alone: every
job's inputs are admissible under grad_refs' and fwd_refs' own conditions, the jobs over the cap stay within the caps the case
list was cut to, the lookups of the 61 older cases are untouched, the bf16 cases' seeds meet test_gpu_bf16_families' rule, and
the references tell a wrong head split from the right one by at least a hundred bounds."""
import pytest

from tests import fwd_refs as R
from tests import geom_refs as W
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F


@pytest.mark.parametrize("cid,mode", W.GRAD_JOBS, ids=[f"{cid}-{mode}" for cid, mode in W.GRAD_JOBS])
def test_gradient_job_inputs_are_admissible(cid, mode):
    """grad_refs.assert_admissible on whichever CPU runs this (the GPU tests assert it again where they compute their bounds),
    and the fp32 oracle itself inside its bound"""
    ref = G.reference(cid, mode)
    G.assert_admissible(ref, f"case {cid} {mode}")
    assert ref.clamp == ((cid, mode) in W.GEOM_OVER_CAP)
    assert all(G.bound(e, ref.clamp) >= G.R_MIN and (not ref.clamp or G.bound(e, True) <= G.CAP) for e in ref.e32.values())
    figs = G.compare(ref.g32, ref)
    assert not any(G.failures(f) for f in figs.values()) and any("kbias" in f for f in figs.values())
    c = W.BY_ID[cid]
    assert tuple(ref.batch[0].shape) == (c.B, c.L) and ref.cfg.D == W.width(c) and ref.cfg.num_heads == c.heads
    assert ref.cfg.dropout == (0.5 if mode == "fused" else 0.0) and not ref.cfg.table_bf16


@pytest.mark.parametrize("cid,mode", W.FWD_JOBS, ids=[f"{cid}-{mode}" for cid, mode in W.FWD_JOBS])
def test_forward_job_inputs_are_admissible(cid, mode):
    ref = R.reference(cid, mode)
    R.assert_admissible(ref, f"case {cid} {mode}")
    assert ref.clamp == ((cid, mode) in W.GEOM_FWD_OVER_CAP)
    assert set(ref.x64) == set(R.OUTPUTS[mode])
    assert all(R.holds(f) for f in R.compare(ref.x32, ref).values())
    if mode == "train":                              # the fused step's loss is held to this reference's
        assert R.fused_step_reference(cid) is ref or (cid, mode) in W.GEOM_FWD_SEEDS
        loss64, e32 = R.loss_reference(R.fused_step_reference(cid))
        assert R.FACTOR_FWD * e32 <= R.CAP_FWD and loss64 > 0.0


def test_jobs_over_the_cap_stay_within_the_caps():
    """at most 8 of the 32 gradient jobs and 4 of the 48 forward jobs (the project's one tenth) are clamped; the tables are
    complete, scanned from 50 on, and reach the lookups"""
    assert W.GEOM_OVER_CAP <= set(W.GRAD_JOBS) and len(W.GEOM_OVER_CAP) <= W.MAX_GEOM_OVER_CAP == 8
    assert W.GEOM_FWD_OVER_CAP <= set(W.FWD_JOBS) and len(W.GEOM_FWD_OVER_CAP) <= W.MAX_GEOM_FWD_OVER_CAP
    assert W.MAX_GEOM_FWD_OVER_CAP == 4 <= len(W.FWD_JOBS) // 10
    assert set(W.GEOM_SEEDS) == set(W.GRAD_JOBS) and all(50 <= s < 250 for s in W.GEOM_SEEDS.values())
    assert set(W.GEOM_FWD_SEEDS) <= set(W.FWD_JOBS) and set(W.GEOM_SD_SEEDS) <= set(W.BY_ID)
    assert all(v == G.SD_SEED + 1 for v in W.GEOM_SD_SEEDS.values())
    for cid, mode in W.GRAD_JOBS:
        assert G.seed_of(cid, mode) == W.GEOM_SEEDS[cid, mode]
    for cid, mode in W.FWD_JOBS:
        first = W.GEOM_SEEDS[cid, "fused" if mode == "train" else "autograd"]
        assert R.seed_of(cid, mode) == W.GEOM_FWD_SEEDS.get((cid, mode), first) >= first
    # the clamp never widens: a clamped job's bounds are at most CAP, an admissible job's 64 e32 are under it by the condition
    for cid, mode in sorted(W.GEOM_OVER_CAP):
        assert max(G.bound(e, True) for e in G.reference(cid, mode).e32.values()) <= G.CAP


def test_the_older_cases_lookups_are_untouched():
    """the OTHER tables are read for the cases outside ALL_CASES only: the 61 cases' seeds, weight seeds and clamps come from
    grad_refs' and fwd_refs' own tables as before"""
    assert len(G.ALL_CASES) == 61 and not set(W.BY_ID) & set(G.BY_ID)
    assert not {k[0] for k in G.SEEDS} & set(W.BY_ID) and not {k[0] for k in G.OVER_CAP} & set(W.BY_ID)
    assert not {k[0] for k in R.FWD_SEEDS} & set(W.BY_ID) and not {k[0] for k in R.FWD_OVER_CAP} & set(W.BY_ID)
    assert not {k[0] for k in G.OTHER_SEEDS} & set(G.BY_ID) and not set(G.OTHER_SD_SEEDS) & set(G.BY_ID)
    assert not {k[0] for k in G.OTHER_OVER_CAP} & set(G.BY_ID) and not {k[0] for k in R.OTHER_FWD_OVER_CAP} & set(G.BY_ID)
    for c in G.ALL_CASES:
        for mode in W.GRAD_MODES:
            assert G.seed_of(c.id, mode) == G.SEEDS[c.id, mode]
        for mode in R.MODES:
            assert R.seed_of(c.id, mode) == R.FWD_SEEDS.get((c.id, mode), G.SEEDS[c.id, "fused" if mode == "train" else "autograd"])


@pytest.mark.parametrize("c", W.BF16_CASES, ids=[c.id for c in W.BF16_CASES])
def test_bf16_case_seeds_meet_the_family_files_rule(c):
    """test_gpu_bf16_families' stated rule, on the CPU oracle: top-11 gaps above 3 TOL, the two oracles' positive logits 20 TOL
    apart, ReLU margin above 2 RELU_MARGIN (at the two fused steps' batches too) - and no earlier seed from 6 / 50 on has all"""
    def ok(seed, fused_seed):
        gap, seen, margin, fused = W.bf16_conditions(c, seed, fused_seed)
        return gap > 3 * F.TOL and seen > 20 * F.TOL and margin > 2 * F.RELU_MARGIN, fused > 2 * F.RELU_MARGIN
    gap, seen, margin, fused = W.bf16_conditions(c)
    print(f"case {c.id}: top-11 gap {gap:.2e}, bf16 vs fp32 {seen:.2e}, relu margin {margin:.2e} / fused {fused:.2e}")
    assert ok(c.seed, c.fused_seed) == (True, True)
    assert not any(ok(s, c.fused_seed)[0] for s in range(6, c.seed))
    assert not any(ok(c.seed, s)[1] for s in range(50, c.fused_seed))


# Smallest distances seen at geom_refs' seeds and weights, in bounds: forward 14438 (w64b with two heads for four), gradient 6936
# (w16a with one head for two, its least-affected attention weight).  The test asserts geom_refs.SHARP_BOUNDS = 100.
@pytest.mark.parametrize("c", W.MULTI_HEAD, ids=[c.id for c in W.MULTI_HEAD])
def test_a_wrong_head_split_is_a_hundred_bounds_away(c):
    """the case's own weights and batch through the fp64 oracle with one head, and for even H > 2 with H / 2: some forward
    output and the LEAST-affected attention weight gradient each lie at least 100 bounds from the case's reference, so the
    head split cannot become invisible to these tests through a change of weights or batches"""
    assert W.wrong_splits(c) == [1] + ([c.heads // 2] if c.heads % 2 == 0 and c.heads > 2 else [])
    for heads in W.wrong_splits(c):
        fwd, grad = W.split_distances(c.id, heads)
        print(f"case {c.id} with {heads} head(s) for {c.heads}: forward {fwd:.0f} bounds, gradient {grad:.0f} bounds")
        assert fwd >= W.SHARP_BOUNDS and grad >= W.SHARP_BOUNDS, (c.id, heads, fwd, grad)
