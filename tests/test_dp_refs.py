"""CPU side of the data-parallel gradient checks (tests/dp_refs.py, tests/test_gpu_dp_fp64.py), on the fp64 oracle alone: the
whole-batch oracle IS the data-parallel step's reference (additivity), the metric rejects every wrong form of the exchange by
ten times the bound - forms the stepped-weight tolerance of tools/dp_parity.py accepts -, the skew batches are skewed, the job
table covers what it says, and the new jobs' inputs are admissible."""
import importlib.util
import os

import pytest

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from srfrd_amd.exchange import shard_bounds
from tests import dp_refs as D
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests.test_encoder_plan import N_CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
worlds = pytest.mark.parametrize("world", D.WORLDS, ids=[f"w{w}" for w in D.WORLDS])


def test_all_cases_is_the_list_it_was():
    """the new cases live in dp_refs; the suites that parametrize over grad_refs.ALL_CASES do not grow"""
    assert len(G.ALL_CASES) == 61 and not {c.id for c in D.NEW} & set(G.BY_ID)
    from tests import geom_refs                  # (the other module that registers cases there: sixteen of its own)
    assert set(G.OTHER) == {"v0", "v1", "g6", "j6", "e38"} | set(geom_refs.BY_ID) and len(G.OTHER) == 5 + 16
    assert all(G.case_of(c.id) is c for c in D.CASES)
    assert [c.id for c in D.CASES] == list(D.REUSED) + ["v0", "v1", "g6", "j6", "e38"]
    for cid, twin in (("g6", "g"), ("j6", "j"), ("e38", "e")):
        assert D.BY_ID[cid]._replace(id=twin, B=G.BY_ID[twin].B, L=G.BY_ID[twin].L, fused_seed=G.BY_ID[twin].fused_seed) == G.BY_ID[twin]
    assert (D.BY_ID["g6"].B, D.BY_ID["j6"].B, D.BY_ID["e38"].L) == (6, 6, 38)


# ---------------------------------------------------------------------------------------------------------------------------
# additivity: what licenses the whole-batch oracle as the reference
# ---------------------------------------------------------------------------------------------------------------------------
@worlds
@pytest.mark.parametrize("cid", ["s", "u0", "v0", "v1"])
def test_count_weighted_rank_gradients_are_the_whole_batch_gradient(cid, world):
    """per-rank fp64 gradients with b0 = rank * B_local, weighted by count / global count (a rank without a target skipped)"""
    ref = D.reference(cid)
    got = D.combined(ref, world)
    worst = max(G.row_errors(got[k], ref.g64[k]) for k in ref.g64)
    leaks = sum(G.zero_row_leaks(got[k], ref.g64[k]) for k in ref.g64)
    print(f"{cid} world {world}: counts {D.rank_counts(ref, world)}, worst row error {worst:.1e}")
    assert worst <= 1e-12 and leaks == 0


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------
FORMS = ("local_mean", "b0_zero", "stats_twice", "rank_dropped", "seam_element")
# the wrong forms whose stepped weights after one Adam step from zero moments tools/dp_parity.py's tolerance accepts (the gap the
# GPU tests close): Adam's first step moves an element by lr g / (|g| + eps), so the gradient's scale is invisible to it
ADAM_ACCEPTS = {("v0", 2): ["stats_twice"], ("v0", 3): ["stats_twice"], ("v1", 2): ["stats_twice"], ("v1", 3): ["stats_twice"]}


def _dp_parity():
    spec = importlib.util.spec_from_file_location("dp_parity", os.path.join(ROOT, "tools", "dp_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _adam_first_step(g, lr=1e-3, eps=1e-8):
    return -lr * g / (g.abs() + eps)


@worlds
@pytest.mark.parametrize("cid", ["v0", "v1"])
def test_metric_rejects_every_wrong_exchange(cid, world):
    ref = D.reference(cid)
    G.assert_admissible(ref, f"case {cid}")
    assert not any(G.failures(f) for f in G.compare(D.combined(ref, world), ref).values())
    forms = D.wrong_forms(ref, world)
    assert tuple(forms) == FORMS
    tolerance = _dp_parity().adam_tolerance
    accepted = []
    for name, mut in forms.items():
        figs = G.compare(mut, ref)
        worst = max(figs, key=lambda k: figs[k]["err"] / figs[k]["bound"])
        best = min(figs[k]["err"] for k in figs)
        over = figs[worst]["err"] / figs[worst]["bound"]
        # one Adam step from the same weights under the right and the wrong gradient, held as dp_parity holds two runs
        viol = sum(int(((_adam_first_step(mut[k]) - _adam_first_step(ref.g64[k])).abs() > tolerance([ref.g64[k]])).sum())
                   for k in mut)
        print(f"{cid} world {world} {name}: worst {worst} {figs[worst]['err']:.2e} = {over:.0f} bounds, best tensor {best:.1e}; "
              f"{viol} stepped weights outside dp_parity's tolerance")
        assert over >= 10.0, (name, worst, figs[worst])
        if viol == 0:
            accepted.append(name)
    assert accepted == ADAM_ACCEPTS[cid, world]


# ---------------------------------------------------------------------------------------------------------------------------
# skew
# ---------------------------------------------------------------------------------------------------------------------------
def test_skew_batches_are_skewed():
    v0, v1 = D.reference("v0"), D.reference("v1")
    assert D.rank_counts(v0, 2) == [227, 11] and D.rank_counts(v0, 3) == [194, 41, 3]
    assert D.rank_counts(v1, 2) == [277, 13] and D.rank_counts(v1, 3) == [194, 96, 0]
    a, b = D.rank_counts(v0, 2)
    assert a >= 10 * b
    assert D.rank_counts(v1, 3)[2] == 0
    assert all(n >= 1 for n in D.rank_counts(v0, 2) + D.rank_counts(v0, 3) + D.rank_counts(v1, 2) + D.rank_counts(v1, 3)[:2])
    seq = v0.batch[0]
    assert [int((row != 0).sum()) for row in seq[8:]] == [1, 1, 1, 0]            # single-item sequences and an all-pad one
    assert [int((row != 0).sum()) for row in v1.batch[0][8:]] == [0, 0, 0, 0]
    assert v0.cfg.kind == "SASRec" and v1.cfg.kind == "SRFRN" and (v1.cfg.d_item, v1.cfg.d_fake) == (45, 5)
    for ref in (v0, v1):        # pads carry no input and no target
        s, _, p, _, n, _ = ref.batch
        assert bool(((s == 0) == (p == 0)).all()) and bool(((s == 0) == (n == 0)).all())


# ---------------------------------------------------------------------------------------------------------------------------
# cover
# ---------------------------------------------------------------------------------------------------------------------------
def test_job_table():
    assert len(D.JOBS) == len(set(D.JOBS)) == len({D.job_id(j) for j in D.JOBS}) == 84
    for cid, world, exchange, det, graph, l2 in D.JOBS:
        assert D.BY_ID[cid].B % world == 0 and world in D.WORLDS and exchange in ("sharded", "allreduce")
        assert D.BY_ID[cid].L <= 200 and D.BY_ID[cid].B <= 12
    for world in D.WORLDS:
        mine = D.jobs_of(world)
        assert {(j[2], j[3]) for j in mine} == {(x, d) for x in ("sharded", "allreduce") for d in (True, False)}
        for c in D.CASES:
            assert (c.id, world, "sharded", True, False, 0.0) in mine and (c.id, world, "sharded", False, False, 0.0) in mine
        extra = [j for j in mine if not (j[2] == "sharded" and not j[4] and j[5] == 0.0)]
        assert sorted(extra) == sorted(
            [(cid, world, "allreduce", False, False, 0.0) for cid in ("c", "f", "u0", "v0", "v1")]
            + [("v0", world, "allreduce", True, False, 0.0), ("u0", world, "sharded", False, True, 0.0),
               ("v1", world, "sharded", False, True, 0.0), ("u0", world, "sharded", True, False, G.L2_EMB),
               ("u0", world, "allreduce", False, False, G.L2_EMB)])
        assert (D.REPEATED[0], world) + D.REPEATED[1:] in mine
    assert D.job_id(("u0", 3, "sharded", True, False, G.L2_EMB)) == "u0-w3-sharded-det-l2"
    assert D.job_id(("v1", 2, "sharded", False, True, 0.0)) == "v1-w2-sharded-atomics-graph"


def test_over_cap_status_carries_over_and_new_jobs_are_not_clamped_past_two():
    for cid in D.REUSED:
        assert D.reference(cid).clamp == ((cid, "fused") in G.OVER_CAP) == D.over_cap(cid)
    assert [cid for cid in D.REUSED if D.over_cap(cid)] == ["f"]
    assert D.DP_OVER_CAP <= {c.id for c in D.NEW} and len(D.DP_OVER_CAP) <= D.MAX_DP_OVER_CAP == 2 and "v0" not in D.DP_OVER_CAP
    assert set(D.DP_SEEDS) == {c.id for c in D.NEW} and all(50 <= s < 250 for s in D.DP_SEEDS.values())


@pytest.mark.parametrize("cid", [c.id for c in D.NEW])
def test_new_job_inputs_are_admissible(cid):
    ref = D.reference(cid)
    G.assert_admissible(ref, f"case {cid} fused")
    assert ref.clamp == (cid in D.DP_OVER_CAP)
    assert all(G.bound(e, ref.clamp) >= G.R_MIN and (not ref.clamp or G.bound(e, True) <= G.CAP) for e in ref.e32.values())
    figs = G.compare(ref.g32, ref)
    assert not any(G.failures(f) for f in figs.values()) and any("kbias" in f for f in figs.values())
    assert tuple(ref.batch[0].shape) == (D.BY_ID[cid].B, D.BY_ID[cid].L)


def test_l2_reference_is_u0s():
    ref = D.reference("u0", G.L2_EMB)
    assert ref.l2 == G.L2_EMB and ref is G.reference("u0", "fused", G.L2_EMB)
    G.assert_admissible(ref, "case u0 fused l2_emb")


def _lay(c):
    return _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)


@worlds
@pytest.mark.parametrize("c", D.CASES, ids=[c.id for c in D.CASES])
def test_local_batch_keeps_the_case_kernel_names(c, world):
    """the host-only plan at B / world under the case's switch: the names the rank program asserts before it launches"""
    lay, Bl = _lay(c), c.B // world
    sw = _lib.SWITCHES[c.switch] if c.switch else 0
    got = F.planned(lay, Bl, c.L, "fused", sw, N_CU, *F.case_scratch(lay, Bl, c.L, "fused"))
    assert got == D.local_names(c.id, world), (c.id, world, got)
    assert F.planned(lay, c.B, c.L, "fused", sw, N_CU, *F.case_scratch(lay, c.B, c.L, "fused")) == tuple(c.fused)


def test_world_3_seams_fall_inside_a_table_row_and_inside_a_dense_tensor():
    """(the item-row seam is e38's: its reason to be here)"""
    in_row = in_dense = 0
    for c in D.CASES:
        cfg = G.cfg_of(c, "fused")
        slots, n_flat = D.flat_slots(cfg)
        assert slots[0][1] == 0 and slots[0][0] == O.key_item(cfg)
        width = slots[0][2] // (cfg.item_number + 1)
        for name, idx, i0 in D.seams(cfg, 3):
            assert i0 == shard_bounds(n_flat, 3, 1)[0] or i0 == shard_bounds(n_flat, 3, 2)[0]
            if name == slots[0][0]:
                in_row += idx % width != 0
            elif name is not None:
                in_dense += idx != 0
    assert in_row >= 1 and in_dense >= 1, (in_row, in_dense)
