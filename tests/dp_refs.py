"""The data-parallel train step's gradient checks (no GPU): jobs, batches and the wrong forms an exchange can take.

tests/test_gpu_dp_fp64.py holds N ranks' first FusedTrainer step, each on its B / N sequences, to the fp64 oracle of the WHOLE
batch under tests/grad_refs.py's metric and bound rule - reference ``grad_refs.fp64_grads`` with ``b0 = 0``.  That is the
data-parallel step's reference as it stands: the loss is a mean over the global target count and the dropout masks are keyed by
the global sequence index, so the count-weighted sum of the ranks' fp64 gradients drawn with ``b0 = rank * B_local`` IS the
whole-batch gradient (tests/test_dp_refs.py: 1e-12).  What only this step runs: the 16-byte statistics all-reduce behind the
``1 / count`` scale, ``rank * B`` as the masks' first sequence, Adam over a biased slice whose moments exist for that slice
only, ``l2_emb`` per slice, the optimizer state advanced in srfrd_pack_weights.

Cases
  reused   every depth-2 case of grad_refs whose batch splits over 2 and 3 ranks, at its ("<id>", "fused") seed and weights:
           ``grad_refs.reference(cid, "fused")`` and ``fwd_refs.fused_step_reference(cid)`` are the references, its OVER_CAP
           status carries over;
  v0, v1   skewed batches at the default geometry (grad_refs.SKEW_PADS, B = 12): target counts 227 / 11 and 194 / 41 / 3 (v0,
           SASRec: the last rank of three holds single-item sequences and an all-pad one), 277 / 13 and 194 / 96 / 0 (v1,
           SRFRN: the last rank of three has no target at all);
  g6, j6   twins of g (seq_len 100, slot-placed backward) and j (seq_len 200, row-owner forward, row-chunked backward) with
           B = 6 instead of 5;
  e38      a twin of e at seq_len 38, whose first seam of three cuts an item-table row.
The five new cases live here, registered in ``grad_refs.OTHER``; ``grad_refs.ALL_CASES`` does not grow.

``wrong_forms``: what a broken exchange would compute, from the fp64 oracle alone; tests/test_dp_refs.py shows each at least ten
times over the bound.
"""
import functools

import torch

from oracle import srfrd_oracle as O
from srfrd_amd.exchange import shard_bounds
from tests import fwd_refs as R
from tests import grad_refs as G

WORLDS = (2, 3)
REUSED = ("a", "b", "c", "d", "e", "f", "p", "q", "s", "u0", "u2")
SKEW = [G._ragged("v0", "SASRec", 50, 0, 0, 12), G._ragged("v1", "SRFRN", 45, 5, 2, 12)]
LONG = [G.BY_ID["g"]._replace(id="g6", B=6, fused_seed=50), G.BY_ID["j"]._replace(id="j6", B=6, fused_seed=50)]
# a twin of e (SASRec, d_item 40) at seq_len 38: under three ranks the first seam of its flat vector cuts item row 280 at
# column 16 - at 300 items no other case here has a seam strictly inside an item row (e's own falls on that row's first element)
SEAM = [G.BY_ID["e"]._replace(id="e38", L=38, fused_seed=50)]
NEW = SKEW + LONG + SEAM
G.OTHER.update({c.id: c for c in NEW})
CASES = [G.BY_ID[cid] for cid in REUSED] + NEW
BY_ID = {c.id: c for c in CASES}
assert all(c.blocks == 2 and c.B % 6 == 0 for c in CASES)
assert REUSED == tuple(c.id for c in G.DEPTH2_CASES if c.B % 6 == 0)

# Batch seeds of the new jobs, by grad_refs' rule (scan_seeds / pick_seed from 50 on, on both kinds of machine the suite runs
# on): the first seed with relu_margin >= 2 * RELU_MARGIN and 64 e32 <= SEARCH_HEADROOM * CAP for every tensor on both.
# Worst-machine e32 at the chosen seeds: v0 1.00e-6 (seeds 50 and 51 have the margin at 1.45e-6 and 1.40e-6: under the condition,
# without the headroom), v1 1.03e-6 (the only seed of 200 with the headroom: the next best are 1.25e-6 at 249 and 138; the
# first seeds are near 2e-6), g6 1.01e-6, j6 1.18e-6, e38 7.9e-7 at its first seed.  The two kinds of machine differ by up to 24 % on one batch (j6 at 52).
DP_SEEDS = {"v0": 60, "v1": 196, "g6": 52, "j6": 53, "e38": 50}
# New jobs without such a seed would take the scanned seed with the margin whose e32 is smallest on the worse machine, bound
# clamped at CAP (tighter than 64 e32 where it acts, never wider): at most MAX_DP_OVER_CAP of them, and never v0.  None needs it.
DP_OVER_CAP = frozenset()
MAX_DP_OVER_CAP = 2


def over_cap(cid):
    return cid in DP_OVER_CAP or (cid, "fused") in G.OVER_CAP


def seed_of(cid):
    return G.SEEDS[cid, "fused"] if cid in G.BY_ID else DP_SEEDS[cid]


def inputs(cid):
    """(case, cfg, weights, whole batch) of one case's first fused step, without any oracle run: what the rank program reads"""
    c = BY_ID[cid]
    return c, G.cfg_of(c, "fused"), G.weights(cid), G.batch_of(c, seed_of(cid))


@functools.lru_cache(maxsize=None)
def reference(cid, l2=0.0):
    """the whole-batch Ref of one case's first fused step; shared by every test of the process, read-only"""
    if cid in G.BY_ID:
        return G.reference(cid, "fused", l2)
    return G.build_ref(BY_ID[cid], "fused", DP_SEEDS[cid], l2)._replace(clamp=cid in DP_OVER_CAP)


@functools.lru_cache(maxsize=None)
def step_reference(cid):
    """the train-mode FwdRef on the same batch: its fp64 loss is the loss of reference(cid)"""
    if cid in G.BY_ID:
        return R.fused_step_reference(cid)
    return R.build_ref(BY_ID[cid], "train", DP_SEEDS[cid])


# ---------------------------------------------------------------------------------------------------------------------------
# jobs
# ---------------------------------------------------------------------------------------------------------------------------
def _jobs():
    jobs = []
    for w in WORLDS:
        jobs += [(c.id, w, "sharded", det, False, 0.0) for c in CASES for det in (True, False)]
        jobs += [(cid, w, "allreduce", False, False, 0.0) for cid in ("c", "f", "u0", "v0", "v1")]
        jobs += [("v0", w, "allreduce", True, False, 0.0)]
        jobs += [(cid, w, "sharded", False, True, 0.0) for cid in ("u0", "v1")]
        jobs += [("u0", w, "sharded", True, False, G.L2_EMB), ("u0", w, "allreduce", False, False, G.L2_EMB)]
    return jobs


JOBS = _jobs()           # (case id, world, exchange, deterministic, use_graph, l2_emb)
REPEATED = ("v0", "sharded", True, False, 0.0)      # run twice at each world: the deterministic exchange repeats its bits


def job_id(job):
    cid, world, exchange, det, graph, l2 = job
    return f"{cid}-w{world}-{exchange}-{'det' if det else 'atomics'}" + ("-graph" if graph else "") + ("-l2" if l2 else "")


def jobs_of(world):
    return [j for j in JOBS if j[1] == world]


# The fused step's (forward, backward) names at the LOCAL batch size, where the plan answers otherwise than at the case's own:
# (case id, B_local) -> names.  Empty: at B_local = 2, 3, 4 and 6 every case keeps its `fused` names (the batch size moves
# only the backward's read-modify-write flag, which the names here do not carry); tests/test_dp_refs.py holds that.
LOCAL_NAMES = {}


def local_names(cid, world):
    c = BY_ID[cid]
    return tuple(LOCAL_NAMES.get((cid, c.B // world), c.fused))


# ---------------------------------------------------------------------------------------------------------------------------
# the ranks' own gradients on the fp64 oracle, and the wrong ways to put them together
# ---------------------------------------------------------------------------------------------------------------------------
def rank_counts(ref, world):
    pos = ref.batch[2]
    Bl = pos.shape[0] // world
    return [int((pos[r * Bl:(r + 1) * Bl] != 0).sum()) for r in range(world)]


def rank_grads(ref, world, b0_of=lambda r, Bl: r * Bl):
    """[(target count, {name: fp64 mean gradient of the rank's own slice} | None where the rank has no target)]: rank r's
    B / world sequences, masks drawn from global sequence b0_of(r, B_local) on (the l2_emb term left out)"""
    sd64 = {k: v.detach().double() for k, v in ref.sd.items()}
    Bl = ref.batch[0].shape[0] // world
    out = []
    for r, n in enumerate(rank_counts(ref, world)):
        part = tuple(x[r * Bl:(r + 1) * Bl] for x in ref.batch)
        out.append((n, O.grads_of(ref.cfg, sd64, part, train=ref.train, seed=ref.seed, b0=b0_of(r, Bl))[1] if n else None))
    return out


def weighted_sum(parts, weights, like):
    out = {k: torch.zeros_like(v) for k, v in like.items()}
    for (_, g), w in zip(parts, weights):
        if g is not None and w != 0.0:
            for k in out:
                out[k] += w * g[k]
    return out


def combined(ref, world):
    """the count-weighted sum of the ranks' gradients: what a correct exchange computes"""
    parts = rank_grads(ref, world)
    total = sum(n for n, _ in parts)
    return weighted_sum(parts, [n / total for n, _ in parts], ref.g64)


def flat_slots(cfg):
    """[(name, offset, numel)] of the model's flat vector [item table | pad | dense] and its length, from a host-side model"""
    from tests.gpu_util import _cpu_model
    m = _cpu_model(cfg)
    names = {id(p): k for k, p in m.named_parameters()}
    return [(names[id(p)], off, p.numel()) for p, off in m._current_slots(m._item_param())], m.n_flat


def seams(cfg, world):
    """[(tensor name | None in the padding, element index inside the tensor, flat index)] of the element each shard but the
    first starts on"""
    slots, n_flat = flat_slots(cfg)
    out = []
    for r in range(1, world):
        i0, _ = shard_bounds(n_flat, world, r)
        hit = [(k, i0 - off) for k, off, n in slots if off <= i0 < off + n]
        out.append((hit[0][0], hit[0][1], i0) if hit else (None, None, i0))
    return out


def wrong_forms(ref, world):
    """{name: gradients} a broken exchange would produce, on the fp64 oracle alone (ref without l2_emb)"""
    assert ref.l2 == 0.0
    parts = rank_grads(ref, world)
    counts = [n for n, _ in parts]
    total = sum(counts)
    out = {}
    # each rank divides by its own count, then the ranks are averaged
    out["local_mean"] = weighted_sum(parts, [1.0 / world] * world, ref.g64)
    # every rank draws rank 0's masks
    out["b0_zero"] = weighted_sum(rank_grads(ref, world, lambda r, Bl: 0), [n / total for n in counts], ref.g64)
    # the statistics summed twice (or the gradient divided by the world once more)
    out["stats_twice"] = {k: v / world for k, v in ref.g64.items()}
    # the rank with the fewest targets (of those that have any) contributes nothing
    least = min((r for r in range(world) if counts[r]), key=lambda r: counts[r])
    out["rank_dropped"] = weighted_sum(parts, [0.0 if r == least else n / total for r, n in enumerate(counts)], ref.g64)
    # the first element of each shard lost
    m = {k: v.clone() for k, v in ref.g64.items()}
    for name, idx, _ in seams(ref.cfg, world):
        if name is not None:
            m[name].view(-1)[idx] = 0.0
    out["seam_element"] = m
    return out
