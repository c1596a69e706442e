"""The encoder gradients' reference and metric (no GPU): an fp64 oracle and a bound relative to each row's own size.

The suite's older gradient checks are ``max|g - g_oracle32| < 1e-4``: one absolute number for every tensor, against the fp32
oracle.  The loss is a mean over all target positions, so at the batches those tests use most gradient elements are themselves
below 1e-4; tests/test_grad_refs.py records which wrong gradients that bar accepts.  Here

  reference  ``fp64_grads``: ``O.grads_of`` on the weights cast to double (the oracle takes its dtype from the weights; dropout
             keep masks stay the fp32 values ``float32(1 / (1 - p))``, promoted - the operation the kernels perform);
  metric     ``row_errors``: per row r of a tensor viewed as (shape[0], -1) (a 1-D tensor is one row), over the rows whose
             fp64 gradient is not exactly zero,   e_r = ||g_r - g64_r||_2 / (||g64_r||_2 + 1e-3 max_r ||g64_r||_2);
             the floor keeps rows a thousand times smaller than the largest on an absolute footing.  Worst row returned;
  zero rows  a row whose fp64 gradient is exactly zero (an item no sequence touches, padding row 0, a position that is pad
             in every sequence) must be exactly zero on the device: ``zero_row_leaks`` counts the elements that are not;
  K bias     the K slice of every ``in_proj_bias`` has true gradient 0 (tests/helpers.py, drop_kbias): left out of e_r, held
             to |g| <= R max|g64| over the Q and V slices instead;
  bound      ``R = bound(e32) = max(64 e32, 2e-5)``, e32 the fp32 ORACLE's row_errors against the fp64 oracle for the same
             tensor and case, computed on the CPU.  64 is a judgement: the kernels sum the same 50 to 64-term products and
             attention sums of at most 208 terms in other orders, use the hardware exp / rcp / rsqrt and (non-deterministic
             mode) sum item rows by float atomics - a few ulp per operation each: tens of times the oracle's own rounding,
             not hundreds.  ``64 e32 <= 1e-4`` is a condition on the INPUTS of a case (``assert_admissible``, asserted on
             the CPU and again where the GPU tests compute their bounds), so every bound is at least 100 times tighter than
             the old bar, relative to the row; the jobs that have no such input are listed in OVER_CAP and clamped there.

Every batch below also keeps every feed-forward ReLU input 2 * RELU_MARGIN away from zero on the fp64 oracle
(test_gpu_bf16_families.relu_margin): no outlier allowance anywhere.

The cases: test_gpu_bf16_families.CASES (every encoder kernel family the plan can choose; tests/test_bf16_family_cover.py) with
the fp32 table, plus ``EXTRA``: the <50,32,8,0> first-generation pair (seq_len 20), and at the default geometry (seq_len 50, no
switch: the ragged pair and the one-launch train kernel) a 17-sequence batch on the tile boundaries and a duplicate-heavy one.
Kernel names do not carry the table flag, so the names of CASES hold for the fp32 table as they stand.

A third mode, "head" (the section of that name below), holds the first step of the four catalog losses to the same metric and
bound rule: reference ``head_grads``, jobs ``HEAD_JOBS``, seeds ``HEAD_SEEDS``.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import srfrd_oracle as O
from tests import loss_refs as LR
from tests import test_gpu_bf16_families as F
from tests.test_gpu_bf16_families import RELU_MARGIN, Case, relu_margin

FLOOR = 1e-3
FACTOR = 64.0
R_MIN = 2e-5
CAP = 1e-4
OLD_BAR = 1e-4            # the suite's absolute bar on max|g - g_oracle32|
BETA1, BETA2 = 0.9, 0.98
BASE = 77                 # FusedTrainer(seed=BASE): the first step's dropout seed is O.step_seed(BASE, 1)
I = F.I
SD_SEED = 7               # random_sd(cfg, 7), as the bf16 family tests
L2_EMB = 1e-3
SEARCH_HEADROOM = 0.8     # seeds are chosen with 64 e32 <= 0.8e-4 (see SEEDS); the tests assert the condition itself, <= 1e-4

_RAG = "srfrd::encoder_{d}_ragged_kernel<{a}>"


def _ragged(cid, kind, d_item, d_fake, K, B):
    f = lambda t: _RAG.format(d="fwd", a=f"{K},{t},{d_item}")
    b = _RAG.format(d="bwd", a=f"{K},{d_item}")
    return Case(cid, kind, d_item, d_fake, 1, 50, B, None, None, None, eval_fwd=f(0), last_fwd=f(0), autograd=(f(0), b),
                fused=(f(1), b))


_G32 = "<50,32,8,0,-1,0,0>"
# ids: "s" seq_len 20; "t*" the tile-boundary batch (TILE_PADS), "u*" the duplicate-heavy batch, both at the default geometry
EXTRA = [
    Case("s", "SASRec", 50, 0, 1, 20, 6, None, None, None, **F._same(F._F + _G32, F._B + _G32)),
    _ragged("t0", "SASRec", 50, 0, 0, 17), _ragged("t1", "SRFR", 45, 5, 1, 17), _ragged("t2", "SRFRN", 45, 5, 2, 17),
    _ragged("t3", "SRFU_B", 50, 0, -1, 17),
    _ragged("u0", "SASRec", 50, 0, 0, 12), _ragged("u2", "SRFRN", 45, 5, 2, 12),
]
DEPTH2_CASES = list(F.CASES) + EXTRA                 # num_blocks = 2: the list the catalog-loss "head" mode stays on

# Depths 1, 3 and 8 (every case above has two blocks, so each of its blocks is the first or the last: a checkpoint offset, a
# packed-weight index, a LayerNorm-cache slot or a dropout site that is right for i = 0 and i = n - 1 and wrong in between
# passes all of them; so does a prefetch that is wrong only where one block is both).  Twins of the cases above - same kind,
# width, heads, switch, batch size and kernel names, id "<twin's id>.<depth>" - with the fp32 table:
#   1, 3  one case per family key the plan produces at that depth (tests/test_depth_cover.py): both sides of every kind-variant
#         backward (a | p, b | q, g | h, j | k, t0 | t2), SRFR (c), the two-head generic pair (d).  k at seq_len 200: with three
#         blocks the row-chunked backward's LDS no longer fits at 203 and the plan answers srfrd_long:: there;
#   8     the LayerNorm caches are at their largest ((4 * 8 + 2) * 64 floats, twice in a backward) and move the plan: the
#         first-generation backward no longer fits at LP = 64 (41 280 floats of 40 960), so the two-head pair (d) runs the generic
#         forward with the srfrd_long:: backward; the default geometry (t0, t2: ragged pair, one-launch train kernel), the
#         slot-placed backward at seq_len 100 (g) and the row-owner / row-chunked pair at seq_len 113 (l) keep their names.
_TWINS_1_3 = ("a", "b", "c", "d", "f", "g", "h", "i", "j", "k", "n", "p", "q", "s", "t0", "t2")
_DEPTH8 = {"t0": {}, "t2": {}, "g": {}, "l": {}, "d": F._same(F._F + F._GEN, F._BL + F._GEN)}
_DEPTH_L = {("k", 3): 200}


def _twin(cid, n, **names):
    base = next(c for c in DEPTH2_CASES if c.id == cid)
    return base._replace(id=f"{cid}.{n}", blocks=n, L=_DEPTH_L.get((cid, n), base.L), **names)


DEPTH = [_twin(cid, n) for n in (1, 3) for cid in _TWINS_1_3] + [_twin(cid, 8, **names) for cid, names in _DEPTH8.items()]
ALL_CASES = DEPTH2_CASES + DEPTH
BY_ID = {c.id: c for c in ALL_CASES}
OTHER = {}                # id -> Case held by another module outside ALL_CASES (tests/dp_refs.py registers its own here)
# What `reference`, `weights` and fwd_refs' lookups read for an OTHER case that runs through them (tests/geom_refs.py registers
# its own here; the tables below - SEEDS, SD_SEEDS, OVER_CAP - stay the 61 cases'): (id, mode) -> batch seed, id -> weight seed,
# the (id, mode) jobs whose bound is clamped at CAP.
OTHER_SEEDS, OTHER_SD_SEEDS, OTHER_OVER_CAP = {}, {}, set()


def case_of(cid):
    return BY_ID[cid] if cid in BY_ID else OTHER[cid]


def seed_of(cid, mode):
    return SEEDS[cid, mode] if cid in BY_ID else OTHER_SEEDS[cid, mode]


TRAIN_KERNEL_IDS = ("t0", "t1", "t2", "t3", "t0.1", "t0.3", "t0.8")          # run with train_launch on and off
L2_ID = "t0"                                         # the one fused case that also runs with l2_emb = L2_EMB
# leading pad counts of the tile-boundary batch: the boundaries tests/fuzz_ragged.py names, with both neighbours
TILE_PADS = (0, 1, 3, 4, 5, 15, 16, 17, 19, 20, 21, 35, 36, 37, 48, 49, 50)

# e32 is the fp32 oracle's rounding, and a matrix product sums in the order its CPU's kernels choose: between the two kinds of
# machine the suite runs on, the worst-tensor e32 of one batch differs by -20 % .. +13 % (5th .. 95th percentile of 2300
# batches) and by a factor of two at the extremes (1.30e-6 and 1.9e-6 for one tensor of one batch).  So a seed is chosen on
# both (tools/grad_fp64_report.py --scan on each, then --pick; pick_seed below):
# (case id, mode) -> batch seed: from the bf16 file's own seed on (6 / 50 for EXTRA), the first of 48 - of 200 where those hold
# none - at which on BOTH machines relu_margin >= 2 * RELU_MARGIN and 64 e32 <= SEARCH_HEADROOM * CAP for every tensor.
SEEDS = {
    ("a", "autograd"): 9, ("a", "fused"): 50, ("b", "autograd"): 6, ("b", "fused"): 62, ("c", "autograd"): 198,
    ("c", "fused"): 110,
    ("d", "autograd"): 7, ("d", "fused"): 50, ("e", "autograd"): 6, ("e", "fused"): 51, ("f", "autograd"): 16,
    ("f", "fused"): 93,
    ("g", "autograd"): 16, ("g", "fused"): 50, ("h", "autograd"): 9, ("h", "fused"): 78, ("i", "autograd"): 16, ("i", "fused"): 50,
    ("j", "autograd"): 131, ("j", "fused"): 56, ("k", "autograd"): 11, ("k", "fused"): 90, ("l", "autograd"): 46,
    ("l", "fused"): 71,
    ("m", "autograd"): 24, ("m", "fused"): 69, ("n", "autograd"): 131, ("n", "fused"): 56, ("o", "autograd"): 130,
    ("o", "fused"): 70,
    ("p", "autograd"): 6, ("p", "fused"): 62, ("q", "autograd"): 9, ("q", "fused"): 50, ("s", "autograd"): 6, ("s", "fused"): 51,
    ("t0", "autograd"): 10, ("t0", "fused"): 50, ("t1", "autograd"): 97, ("t1", "fused"): 165, ("t2", "autograd"): 92,
    ("t2", "fused"): 83, ("t3", "autograd"): 65, ("t3", "fused"): 128, ("u0", "autograd"): 12, ("u0", "fused"): 50,
    ("u2", "autograd"): 11, ("u2", "fused"): 100,
}
# DEPTH, by the same rule over 200 batches a job, from three scans: both kinds of machine, and the first kind once more with the
# BLAS library held to its AVX2 code path (MKL_CBWR=AVX2; its default is AVX-512).  The third scan moved six picks and no job
# in or out of OVER_CAP; one batch differed by 42 % between the kinds (k.3 autograd at batch 35: 1.13e-6 and 1.60e-6).
SEEDS.update({
    ("a.1", "autograd"): 8, ("a.1", "fused"): 50, ("b.1", "autograd"): 7, ("b.1", "fused"): 54, ("c.1", "autograd"): 104,
    ("c.1", "fused"): 194, ("d.1", "autograd"): 8, ("d.1", "fused"): 50, ("f.1", "autograd"): 153, ("f.1", "fused"): 202,
    ("g.1", "autograd"): 9, ("g.1", "fused"): 50, ("h.1", "autograd"): 13, ("h.1", "fused"): 67, ("i.1", "autograd"): 9,
    ("i.1", "fused"): 50, ("j.1", "autograd"): 11, ("j.1", "fused"): 57, ("k.1", "autograd"): 29, ("k.1", "fused"): 84,
    ("n.1", "autograd"): 11, ("n.1", "fused"): 57, ("p.1", "autograd"): 7, ("p.1", "fused"): 54, ("q.1", "autograd"): 8,
    ("q.1", "fused"): 50, ("s.1", "autograd"): 6, ("s.1", "fused"): 50, ("t0.1", "autograd"): 6, ("t0.1", "fused"): 50,
    ("t2.1", "autograd"): 13, ("t2.1", "fused"): 51,
    ("a.3", "autograd"): 9, ("a.3", "fused"): 54, ("b.3", "autograd"): 26, ("b.3", "fused"): 168, ("c.3", "autograd"): 185,
    ("c.3", "fused"): 55, ("d.3", "autograd"): 11, ("d.3", "fused"): 55, ("f.3", "autograd"): 201, ("f.3", "fused"): 85,
    ("g.3", "autograd"): 107, ("g.3", "fused"): 67, ("h.3", "autograd"): 37, ("h.3", "fused"): 143, ("i.3", "autograd"): 107,
    ("i.3", "fused"): 67, ("j.3", "autograd"): 208, ("j.3", "fused"): 124, ("k.3", "autograd"): 88, ("k.3", "fused"): 157,
    ("n.3", "autograd"): 208, ("n.3", "fused"): 124, ("p.3", "autograd"): 26, ("p.3", "fused"): 168, ("q.3", "autograd"): 9,
    ("q.3", "fused"): 54, ("s.3", "autograd"): 12, ("s.3", "fused"): 55, ("t0.3", "autograd"): 11, ("t0.3", "fused"): 51,
    ("t2.3", "autograd"): 21, ("t2.3", "fused"): 79,
    ("t0.8", "autograd"): 104, ("t0.8", "fused"): 224, ("t2.8", "autograd"): 45, ("t2.8", "fused"): 69, ("g.8", "autograd"): 107,
    ("g.8", "fused"): 72, ("l.8", "autograd"): 106, ("l.8", "fused"): 55, ("d.8", "autograd"): 63, ("d.8", "fused"): 58,
})
# Weights: random_sd(cfg, SD_SEED) as in the bf16 family tests, but for b, k and p (SRFRN): the next weight seed, under which
# their batches are found among the first.  At depth 3 the same for h, k and t2 (under SD_SEED: no batch of 200 with headroom for
# h.3 in either mode, k.3 in either mode, t2.3 fused; under 8 all but the fused jobs of h.3 and k.3 have one).
SD_SEEDS = {"b": 8, "k": 8, "p": 8, "h.3": 8, "k.3": 8, "t2.3": 8}
# Jobs without such a seed.  Of the scanned batches with the ReLU margin they take the one whose e32 is smallest on the worse
# machine: f 2.2e-6 / 1.8e-6, l 3.3e-6 / 2.7e-6, m 2.8e-6 / 2.2e-6 (autograd / fused; SRFU_B and SRFR at seq_len 64 .. 128: no
# input comes near the 1.5625e-6 the condition allows - these kinds add one large shared vector to every position, which the V
# and out_proj rows cancel, and the worst of 150 rows is an extreme value that grows with the length); and the autograd batches
# of c 1.27e-6, j = n 1.40e-6, o 1.47e-6, t1 1.44e-6, t3 1.41e-6: under the condition on both machines, without the headroom
# that would promise it on a third.  For these jobs alone the condition is not asserted and `bound` is clamped at CAP -
# tighter than 64 e32 where it acts, never wider.  They keep their place: f is the only case of the <50,64,8,0> pair, o of the
# two-head srfrd_long:: pair.
OVER_CAP = frozenset([(c, m) for c in "flm" for m in ("autograd", "fused")]
                     + [(c, "autograd") for c in ("c", "j", "n", "o", "t1", "t3")])
# DEPTH.  e32 grows with the depth (worst tensor of the chosen batches, worse code path: 5.8e-7 .. 1.2e-6 at depth 1 outside
# this set, 1.0e-6 .. 1.25e-6 at depth 3, 2.3e-6 .. 6.9e-6 at depth 8), so at depth 8 the condition has no input: EVERY depth-8
# job is clamped at CAP, 14 .. 43 times its e32 where an admissible job has 64.  At depths 1 and 3, of 200 batches: SRFR and
# SRFU_B as at depth 2 (c.1 1.42e-6 / 1.27e-6, f.1 1.71e-6 / 1.36e-6, c.3 2.22e-6 / 2.22e-6, f.3 2.70e-6 / 2.24e-6), the fused
# steps of SRFRN at depth 3 (b.3 = p.3 1.43e-6, h.3 1.34e-6, k.3 1.55e-6) and j.3 = n.3 autograd 1.65e-6 (seq_len 200).
# MAX_DEPTH_OVER_CAP: they may be a quarter of the depth-1 and depth-3 jobs at most (tests/test_grad_refs.py).
DEPTH_OVER_CAP = frozenset([(c.id, m) for c in DEPTH if c.blocks == 8 for m in ("autograd", "fused")]
                           + [(c, m) for c in ("c.1", "f.1", "c.3", "f.3") for m in ("autograd", "fused")]
                           + [(c, "fused") for c in ("b.3", "p.3", "h.3", "k.3")] + [("j.3", "autograd"), ("n.3", "autograd")])
MAX_DEPTH_OVER_CAP = 2 * sum(c.blocks != 8 for c in DEPTH) // 4
OVER_CAP = OVER_CAP | DEPTH_OVER_CAP


def case_ids(cases=None):
    return [f"{c.id}-{c.kind}-L{c.L}" + (f"-{c.switch}" if c.switch else "") + (f"-h{c.heads}" if c.heads > 1 else "")
            + (f"-b{c.blocks}" if c.blocks != 2 else "") for c in (cases or ALL_CASES)]


# ---------------------------------------------------------------------------------------------------------------------------
# reference and metric
# ---------------------------------------------------------------------------------------------------------------------------
def fp64_grads(cfg, sd, batch, train=False, seed=0, l2_emb=0.0):
    """{name: fp64 gradient} of the oracle on the weights cast to double"""
    return O.grads_of(cfg, {k: v.detach().double() for k, v in sd.items()}, batch, train=train, seed=seed, b0=0, l2_emb=l2_emb)[1]


def fp32_grads(cfg, sd, batch, train=False, seed=0, l2_emb=0.0):
    """the fp32 oracle's gradients, on one thread: e32 is this run's rounding, and the order of a threaded matrix product's
    sums follows the thread count (seen: 1.50e-6 on 8 threads, 1.61e-6 on 64, for one tensor of one case)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return O.grads_of(cfg, sd, batch, train=train, seed=seed, b0=0, l2_emb=l2_emb)[1]
    finally:
        torch.set_num_threads(n)


def _as_rows(t):
    t = t.detach().cpu().double()
    return t.reshape(t.shape[0], -1) if t.dim() >= 2 else t.reshape(1, -1)


def row_errors(g, g64):
    """worst e_r over the rows whose fp64 gradient is not exactly zero (0.0 where there is none)"""
    a, b = _as_rows(g), _as_rows(g64)
    assert a.shape == b.shape
    live = (b != 0).any(dim=1)
    if not bool(live.any()):
        return 0.0
    nb = b.norm(dim=1)
    e = (a - b).norm(dim=1) / (nb + FLOOR * nb.max())
    return float(e[live].max())


def zero_row_leaks(g, g64):
    """number of non-zero elements of `g` in the rows whose fp64 gradient is exactly zero"""
    a, b = _as_rows(g), _as_rows(g64)
    dead = ~(b != 0).any(dim=1)
    return int((a[dead] != 0).sum())


def bound(e32, clamp=False):
    """max(64 e32, 2e-5); clamp (the OVER_CAP jobs only): never past CAP"""
    r = max(FACTOR * e32, R_MIN)
    return min(r, CAP) if clamp else r


def is_kbias(name):
    return name.endswith("in_proj_bias")


def without_k(t, D):
    """the Q and V slices of an in_proj_bias (its K slice's true gradient is 0)"""
    return torch.cat([t[:D], t[2 * D:]])


def tensor_figures(name, g, g64, g32, D, kbias=True, clamp=False, r=None):
    """One tensor of one run against its reference -> dict: e32, bound, err (the device's row_errors), zero_leaks, old (the
    former metric: max|g - g32|), and for an in_proj_bias kbias / kbias_limit.  r: the bound, where it is not bound(e32) of
    these very tensors (the second moment)."""
    g = g.detach().cpu().double()
    out = {"old": float((g - g32.double()).abs().max())}
    kbias = kbias and is_kbias(name)        # (under l2_emb the K slice has a gradient of its own: an ordinary part of the row)
    if kbias:
        k = g[D:2 * D]
        g, g64, g32 = without_k(g, D), without_k(g64, D), without_k(g32, D)
    out["e32"] = row_errors(g32, g64)
    out["bound"] = bound(out["e32"], clamp) if r is None else r
    out["err"] = row_errors(g, g64)
    out["zero_leaks"] = zero_row_leaks(g, g64)
    if kbias:
        out["kbias"], out["kbias_limit"] = float(k.abs().max()), out["bound"] * float(g64.abs().max())
    return out


def failures(fig):
    """what one tensor_figures() result misses, as text ([] = it holds)"""
    bad = []
    if not fig["err"] <= fig["bound"]:
        bad.append(f"row error {fig['err']:.3e} > {fig['bound']:.3e}")
    if fig["zero_leaks"]:
        bad.append(f"{fig['zero_leaks']} non-zero elements in rows whose true gradient is exactly zero")
    if "kbias" in fig and not fig["kbias"] <= fig["kbias_limit"]:
        bad.append(f"K bias {fig['kbias']:.3e} > {fig['kbias_limit']:.3e}")
    return bad


def compare(grads, ref, squares=False):
    """every tensor of `grads` ({name: device gradient}) against a Ref -> {name: tensor_figures}.  squares: `grads` holds
    g ** 2 (Adam's second moment / (1 - beta2)): compared with g64 ** 2 under twice the gradient's bound; its K-bias slice,
    as sqrt(v) = |g|, against twice the gradient's K-bias limit."""
    assert set(grads) == set(ref.g64)
    out = {}
    for k in ref.g64:
        kb = ref.l2 == 0.0
        if not squares:
            out[k] = tensor_figures(k, grads[k], ref.g64[k], ref.g32[k], ref.cfg.D, kbias=kb, clamp=ref.clamp)
            continue
        r = 2.0 * bound(ref.e32[k], ref.clamp)
        fig = tensor_figures(k, grads[k], ref.g64[k] ** 2, ref.g32[k].double() ** 2, ref.cfg.D, kbias=kb, r=r)
        fig["e32"] = ref.e32[k]
        if "kbias" in fig:
            fig["kbias"], fig["kbias_limit"] = fig["kbias"] ** 0.5, r * float(without_k(ref.g64[k], ref.cfg.D).abs().max())
        out[k] = fig
    return out


def assert_holds(figs, what):
    bad = {k: failures(f) for k, f in figs.items() if failures(f)}
    worst = max(figs, key=lambda k: figs[k]["err"] / figs[k]["bound"])
    print(f"{what}: worst {worst} {figs[worst]['err']:.2e} of {figs[worst]['bound']:.2e}"
          f" (old metric {max(f['old'] for f in figs.values()):.2e})")
    assert not bad, (what, bad)


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------
def _reviews(g, seq, pos, neg):
    rsq = torch.where(seq != 0, torch.randint(1, 3, seq.shape, generator=g), torch.zeros_like(seq))
    prs = torch.where(pos != 0, torch.randint(1, 3, seq.shape, generator=g), torch.zeros_like(pos))
    return seq, rsq, pos, prs, neg, (neg != 0).long()


def tile_batch(seed, L=50):
    """17 sequences, sequence i with TILE_PADS[i] leading pads (the last is all pad); an interior pad in sequence 3; rows 5
    and 11 keep target ids on their padded positions (the head's range starts in front of the blocks')"""
    g = torch.Generator().manual_seed(seed)
    B = len(TILE_PADS)
    seq, pos, neg = (torch.randint(1, I + 1, (B, L), generator=g) for _ in range(3))
    for b, t0 in enumerate(TILE_PADS):
        seq[b, :t0] = 0
        if b not in (5, 11):
            pos[b, :t0] = 0
            neg[b, :t0] = 0
    seq[3, 27] = 0
    return _reviews(g, seq, pos, neg)


def dup_batch(seed, B=12, L=50):
    """a quarter of the rows draw inputs, positives and negatives from items 1..8: one id occurs dozens of times, as input,
    positive and negative at once; leading pads on the other rows as in any batch"""
    g = torch.Generator().manual_seed(seed)
    seq, pos, neg = (torch.randint(1, I + 1, (B, L), generator=g) for _ in range(3))
    for b in range(B):
        if b % 4 == 0:
            for x in (seq, pos, neg):
                x[b] = torch.randint(1, 9, (L,), generator=g)
        else:
            t0 = int(torch.randint(0, L - 1, (1,), generator=g))
            for x in (seq, pos, neg):
                x[b, :t0] = 0
    return _reviews(g, seq, pos, neg)


# leading pad counts of the skewed batches (tests/dp_refs.py: split over 2 or 3 ranks, a rank's share of the targets is a tenth
# of another's, or nothing): v0 ends in single-item sequences and one all-pad sequence, v1 in four all-pad sequences
SKEW_PADS = {"v0": (0, 1, 2, 3, 30, 37, 44, 48, 49, 49, 49, 50), "v1": (0, 1, 2, 3, 0, 17, 40, 47, 50, 50, 50, 50)}


def skew_batch(seed, pads, L=50):
    """sequence i with pads[i] leading pads, inputs and both targets zero there"""
    g = torch.Generator().manual_seed(seed)
    seq, pos, neg = (torch.randint(1, I + 1, (len(pads), L), generator=g) for _ in range(3))
    for b, t0 in enumerate(pads):
        for x in (seq, pos, neg):
            x[b, :t0] = 0
    return _reviews(g, seq, pos, neg)


def batch_of(c, seed):
    import srfrd_amd
    if c.id in SKEW_PADS:
        return skew_batch(seed, SKEW_PADS[c.id])
    if c.id.startswith("t"):
        return tile_batch(seed)
    if c.id.startswith("u"):
        return dup_batch(seed, c.B)
    return tuple(srfrd_amd.synthetic_batch(I, c.L, c.B, seed=seed, device="cpu")[1:])


def first_seed(c, mode):
    if mode.startswith("head/"):
        mode = "fused"
    return {"autograd": c.seed, "fused": c.fused_seed}[mode] or {"autograd": 6, "fused": 50}[mode]


# ---------------------------------------------------------------------------------------------------------------------------
# per-case references, computed once per process
# ---------------------------------------------------------------------------------------------------------------------------
Ref = namedtuple("Ref", "cfg sd batch train seed l2 g64 g32 e32 margin clamp")


def cfg_of(c, mode):
    return F.cfg_of(c, bf16=False, dropout=0.0 if mode == "autograd" else 0.5)


@functools.lru_cache(maxsize=None)
def weights(cid, sd_seed=None):
    from tests.gpu_util import random_sd
    return random_sd(cfg_of(case_of(cid), "autograd"), sd_seed or SD_SEEDS.get(cid) or OTHER_SD_SEEDS.get(cid, SD_SEED))


def build_ref(c, mode, seed, l2=0.0):
    """mode "autograd": a training-mode forward with dropout 0; "fused": the first FusedTrainer step, dropout 0.5"""
    cfg, sd, batch = cfg_of(c, mode), weights(c.id), batch_of(c, seed)
    train = mode == "fused"
    dseed = O.step_seed(BASE, 1) if train else 0
    g64 = fp64_grads(cfg, sd, batch, train=train, seed=dseed, l2_emb=l2)
    g32 = fp32_grads(cfg, sd, batch, train=train, seed=dseed, l2_emb=l2)
    e32 = {k: tensor_figures(k, g32[k], g64[k], g32[k], cfg.D, kbias=l2 == 0.0)["e32"] for k in g64}
    margin = relu_margin(cfg, {k: v.double() for k, v in sd.items()}, batch, train=train, seed=dseed)
    return Ref(cfg, sd, batch, train, dseed, l2, g64, g32, e32, margin, (c.id, mode) in OVER_CAP or (c.id, mode) in OTHER_OVER_CAP)


def under_cap(ref):
    return FACTOR * max(ref.e32.values()) <= CAP


def assert_admissible(ref, what):
    """the condition on a case's inputs, on the oracle alone, on whichever CPU computes the bounds: every ReLU input
    2 * RELU_MARGIN from zero, and 64 e32 <= CAP for every tensor (but for the OVER_CAP jobs, whose bounds are clamped there)"""
    worst = max(ref.e32, key=ref.e32.get)
    print(f"{what}: worst e32 {ref.e32[worst]:.2e} ({worst}), relu margin {ref.margin:.2e}")
    assert ref.margin >= 2 * RELU_MARGIN, what
    assert ref.clamp or under_cap(ref), (what, worst, ref.e32[worst])


@functools.lru_cache(maxsize=None)
def reference(cid, mode, l2=0.0):
    """the Ref of one case and mode at its SEEDS entry, shared by every test of the process; treat as read-only"""
    return build_ref(case_of(cid), mode, seed_of(cid, mode), l2)


def scan_seeds(job):
    """(case id, mode, count) -> [[seed, worst e32, relu margin], ...] from first_seed on, on THIS machine's CPU"""
    cid, mode, count = job
    c = case_of(cid)
    out = []
    for seed in range(first_seed(c, mode), first_seed(c, mode) + count):
        ref = build_head_ref(head_job(cid, mode[5:]), seed).ref if mode.startswith("head/") else build_ref(c, mode, seed)
        out.append([seed, max(ref.e32.values()), ref.margin])
    return out


def pick_seed(scans):
    """scans: scan_seeds' rows of one case and mode, one list per kind of machine the suite runs on.  -> (seed, found): the
    first seed whose ReLU margin holds and whose 64 e32 stays under SEARCH_HEADROOM * CAP on all of them; where there is none,
    the seed with the margin whose e32 is smallest on its worst machine, and False (an OVER_CAP job)"""
    ok = [rows for rows in zip(*scans) if all(m >= 2 * RELU_MARGIN for _, _, m in rows)]
    assert all(len({r[0] for r in rows}) == 1 for rows in ok)
    for rows in ok:
        if all(FACTOR * e <= SEARCH_HEADROOM * CAP for _, e, _ in rows):
            return rows[0][0], True
    return min(ok, key=lambda rows: max(e for _, e, _ in rows))[0][0], False

# ---------------------------------------------------------------------------------------------------------------------------
# mode "head": the first FusedTrainer(loss=...) step of the four catalog losses
# ---------------------------------------------------------------------------------------------------------------------------
# The step runs srfrd_encoder_fwd_sched with the plan bits CKPT | DROPOUT and srfrd_encoder_bwd_sched with DROPOUT alone: the
# NON-training instantiations with dropout masks on, the gradient entering through d_hidden - a combination neither mode above
# reaches ("autograd": those instantiations, dropout 0, gradient through the logits; "fused": the training instantiations).
# Around it the loss head, its table rows merged with the encoder's input rows (srfrd_table_reduce over contrib_ce,
# srfrd_table_reduce_mixed over the rank-1 rows, the de_ce add under deterministic=True) and the Adam tail's 1 / stats[2]:
# stepped weights show none of these scales.  Same cases, weights, dropout, metric and bound rule as "fused".
HEAD_LOSSES = ("softmax", "sampled_softmax", "token_softmax", "gbce")
TOKEN_LOSSES = ("token_softmax", "gbce")
OBJECTIVE = {"token_softmax": "softmax", "gbce": "gbce"}
GBCE_BETA = 0.6
K_TOKEN, K_TOKEN_WIDE = 5, 65      # 65 (the duplicate-heavy batches): one more than a wave, many rank-1 rows per item
K_SAMPLED, NEG_ALPHA = 96, 0.75    # neg_counts = arange(n + 1) ** 0.5, as test_gpu_ce_trainer.test_one_step_against_fp64_oracle
DEFAULT_IDS = ("t0", "t1", "t2", "t3", "u0", "u2")           # the default geometry: ragged pair
# Every other case under ONE loss, so that every backward family runs once from d_hidden with masks on: the losses in rotation
# inside each family (gbce skipped on SRFRN, which the trainer refuses), so that each loss meets a first-generation, a
# slot-placed, a row-chunked and a srfrd_long:: backward.  Only i and o have a srfrd_long:: backward: they run two losses each.
ROTATION = {
    "b": ("softmax",), "c": ("sampled_softmax",), "d": ("token_softmax",), "e": ("gbce",), "f": ("softmax",),     # first generation
    "q": ("sampled_softmax",), "s": ("token_softmax",),
    "a": ("gbce",), "g": ("softmax",), "h": ("sampled_softmax",), "p": ("token_softmax",),                        # slot-placed
    "j": ("gbce",), "k": ("softmax",), "l": ("sampled_softmax",), "m": ("token_softmax",), "n": ("gbce",),        # row-chunked
    "i": ("softmax", "token_softmax"), "o": ("sampled_softmax", "gbce"),                                          # srfrd_long::
}
HEAD_L2 = ("token_softmax", "softmax")     # the two losses L2_ID also runs with l2_emb = L2_EMB (a term NOT divided by the count)

# cid: remove_accidental_hits on for half the jobs; with_lq: whether step() is handed the log-Q plane (None: zeros; "gbce" never
# passes it to its head, "token_softmax" subtracts it).  l2: l2_emb.
HeadJob = namedtuple("HeadJob", "cid loss K remove with_lq l2")


def _head_jobs():
    pairs = [(cid, loss) for cid in DEFAULT_IDS for loss in HEAD_LOSSES]
    pairs += [(c.id, loss) for c in ALL_CASES if c.id in ROTATION for loss in ROTATION[c.id]]
    pairs = [(cid, loss) for cid, loss in pairs if not (loss == "gbce" and BY_ID[cid].kind == "SRFRN")]
    jobs, n_tok = [], {loss: 0 for loss in TOKEN_LOSSES}
    for cid, loss in pairs:
        K, remove, with_lq = 0, True, True
        if loss == "sampled_softmax":
            K = K_SAMPLED
        elif loss in TOKEN_LOSSES:
            i = n_tok[loss]
            n_tok[loss] += 1
            K = K_TOKEN_WIDE if cid.startswith("u") else K_TOKEN
            remove, with_lq = i % 2 == 0, i % 3 != 2
        jobs.append(HeadJob(cid, loss, K, remove, with_lq, 0.0))
    by = {(j.cid, j.loss): j for j in jobs}
    return jobs + [by[L2_ID, loss]._replace(l2=L2_EMB) for loss in HEAD_L2]


HEAD_JOBS = _head_jobs()


def head_job(cid, loss, l2=0.0):
    return next(j for j in HEAD_JOBS if (j.cid, j.loss, j.l2) == (cid, loss, l2))


def head_id(j):
    return f"{j.cid}-{j.loss}" + ("-l2" if j.l2 else "")


# (forward, backward) as srfrd_encoder_plan prints them on the built library for the head step's two launches
# (test_gpu_bf16_families._plan_bits()["head"]), the backward's read-modify-write flag dropped: the non-training instantiations.
HEAD_NAMES = {
    "a": ("srfrd::encoder_fwd_kernel<50,64,8,50,0,0,50>", "srfrd::encoder_bwd_slots_kernel<50,50,0,50>"),
    "b": ("srfrd::encoder_fwd_kernel<50,64,8,50,2,0,45>", "srfrd::encoder_bwd_kernel<50,64,8,50,2,0,45>"),
    "c": ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    "d": ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    "e": ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    "f": ("srfrd::encoder_fwd_kernel<50,64,8,0,-1,0,0>", "srfrd::encoder_bwd_kernel<50,64,8,0,-1,0,0>"),
    "g": ("srfrd::encoder_fwd_kernel<50,112,8,100,0,0,50>", "srfrd::encoder_bwd_slots_kernel<50,100,0,50>"),
    "h": ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_slots_kernel<50,100,2,45>"),
    "i": ("srfrd::encoder_fwd_kernel<50,112,8,100,0,0,50>", "srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    "j": ("srfrd::encoder_fwd_rows_kernel<50,0,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,0,50>"),
    "k": ("srfrd::encoder_fwd_rows_kernel<50,2,45,1>", "srfrd::encoder_bwd_chunks_kernel<50,2,45>"),
    "l": ("srfrd::encoder_fwd_rows_kernel<50,-1,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,-1,50>"),
    "m": ("srfrd::encoder_fwd_rows_kernel<50,1,45,1>", "srfrd::encoder_bwd_chunks_kernel<50,1,45>"),
    "n": ("srfrd_long::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_chunks_kernel<50,0,50>"),
    "o": ("srfrd_long::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    "p": ("srfrd::encoder_fwd_rows_kernel<50,2,45,1>", "srfrd::encoder_bwd_slots_kernel<50,50,2,45>"),
    "q": ("srfrd::encoder_fwd_kernel<50,64,8,50,0,0,50>", "srfrd::encoder_bwd_kernel<50,64,8,50,0,0,50>"),
    "s": ("srfrd::encoder_fwd_kernel<50,32,8,0,-1,0,0>", "srfrd::encoder_bwd_kernel<50,32,8,0,-1,0,0>"),
    "t0": ("srfrd::encoder_fwd_ragged_kernel<0,0,50>", "srfrd::encoder_bwd_ragged_kernel<0,50>"),
    "t1": ("srfrd::encoder_fwd_ragged_kernel<1,0,45>", "srfrd::encoder_bwd_ragged_kernel<1,45>"),
    "t2": ("srfrd::encoder_fwd_ragged_kernel<2,0,45>", "srfrd::encoder_bwd_ragged_kernel<2,45>"),
    "t3": ("srfrd::encoder_fwd_ragged_kernel<-1,0,50>", "srfrd::encoder_bwd_ragged_kernel<-1,50>"),
    "u0": ("srfrd::encoder_fwd_ragged_kernel<0,0,50>", "srfrd::encoder_bwd_ragged_kernel<0,50>"),
    "u2": ("srfrd::encoder_fwd_ragged_kernel<2,0,45>", "srfrd::encoder_bwd_ragged_kernel<2,45>"),
}

# (case id, loss) -> batch seed, chosen as SEEDS is (tools/grad_fp64_report.py --scan --jobs head on each kind of machine, then
# --pick): from the fused step's first seed on, the first of 200 - of 600 where those hold none - at which on BOTH machines
# relu_margin >= 2 * RELU_MARGIN and 64 e32 <= SEARCH_HEADROOM * CAP for every tensor.  The l2_emb jobs run at the seed of
# their case and loss.
HEAD_SEEDS = {
    ("t0", "softmax"): 50, ("t0", "sampled_softmax"): 50, ("t0", "token_softmax"): 50, ("t0", "gbce"): 50,
    ("t1", "softmax"): 192, ("t1", "sampled_softmax"): 93, ("t1", "token_softmax"): 381, ("t1", "gbce"): 50,
    ("t2", "softmax"): 78, ("t2", "sampled_softmax"): 270, ("t2", "token_softmax"): 309, ("t3", "softmax"): 514,
    ("t3", "sampled_softmax"): 230, ("t3", "token_softmax"): 512, ("t3", "gbce"): 90, ("u0", "softmax"): 50,
    ("u0", "sampled_softmax"): 50, ("u0", "token_softmax"): 50, ("u0", "gbce"): 88, ("u2", "softmax"): 191,
    ("u2", "sampled_softmax"): 551, ("u2", "token_softmax"): 177, ("a", "gbce"): 50, ("b", "softmax"): 124,
    ("c", "sampled_softmax"): 229, ("d", "token_softmax"): 50, ("e", "gbce"): 52, ("f", "softmax"): 220, ("g", "softmax"): 54,
    ("h", "sampled_softmax"): 134, ("i", "softmax"): 54, ("i", "token_softmax"): 52, ("j", "gbce"): 56, ("k", "softmax"): 122,
    ("l", "sampled_softmax"): 112, ("m", "token_softmax"): 83, ("n", "gbce"): 56, ("o", "sampled_softmax"): 70,
    ("o", "gbce"): 72, ("p", "token_softmax"): 392, ("q", "sampled_softmax"): 50, ("s", "token_softmax"): 50,
}
# Weights: as "fused", but for t2 under token_softmax the next weight seed (as SD_SEEDS does for b / k / p): under SD_SEED its
# first 200 batches hold no seed with headroom on both machines (best 1.66e-6).  The same was tried for the other SRFRN jobs
# without a seed (t2, u2, b, k under softmax, u2 under token_softmax, h under sampled_softmax) and for t1 / t3 under softmax: no
# batch of 200 either.
HEAD_SD_SEEDS = {("t2", "token_softmax"): 8}
# Head jobs without such a seed: entries (case id, "head/" + loss) of OVER_CAP, bound clamped at CAP, at the scanned batch
# with the ReLU margin whose e32 is smallest on the worse machine.  The full-catalog softmax on every kind but SASRec (t1 1.36e-6,
# t2 1.99e-6, t3 1.52e-6, u2 1.76e-6, b 1.52e-6, k 2.69e-6, f 2.42e-6: three hundred logits per position through the shared
# vector these kinds add); the long SRFU_B / SRFR cases that are over the cap in every mode (f above, l 2.17e-6, m 1.84e-6);
# the duplicate-heavy SRFRN batch at K = 65 (u2 token_softmax 3.24e-6); and h sampled_softmax 1.34e-6, t3 token_softmax
# 1.28e-6: under the condition on both machines, without the headroom.
HEAD_OVER_CAP = frozenset([(cid, "head/softmax") for cid in ("t1", "t2", "t3", "u2", "b", "f", "k")]
                          + [("l", "head/sampled_softmax"), ("m", "head/token_softmax"), ("u2", "head/token_softmax"),
                             ("h", "head/sampled_softmax"), ("t3", "head/token_softmax")])
OVER_CAP = OVER_CAP | HEAD_OVER_CAP


def token_negatives(c, pos, K, seed):
    """(negatives (B, L, K) int64, log_q (B, L, K) float32) on the host from the job's seed: zero at dead positions; at live
    ones a fifth of the slots unused (0), a seventh accidental hits (the position's own target), every ninth live position -
    the first among them - with all K slots unused; on the duplicate-heavy batch the rows that draw their ids from items 1..8
    draw their negatives there too.  log_q: standard normal at live positions."""
    g = torch.Generator().manual_seed(1000 * seed + K)
    B, L = pos.shape
    neg = torch.randint(1, I + 1, (B, L, K), generator=g)
    if c.id.startswith("u"):
        neg[0::4] = torch.randint(1, 9, neg[0::4].shape, generator=g)
    neg[torch.rand(B, L, K, generator=g) < 0.2] = 0
    hit = torch.rand(B, L, K, generator=g) < 1.0 / 7.0
    neg = torch.where(hit, pos.unsqueeze(-1).expand_as(neg), neg)
    live = pos != 0
    flat = neg.view(-1, K)
    flat[live.view(-1).nonzero().view(-1)[0::9]] = 0
    neg = neg * live.unsqueeze(-1)
    log_q = torch.randn(B, L, K, generator=g) * live.unsqueeze(-1)
    return neg.contiguous(), log_q.contiguous()


def sampled_counts():
    return torch.arange(I + 1.0) ** 0.5


@functools.lru_cache(maxsize=None)
def sampled_negatives(seed_word, K=K_SAMPLED):
    """what FusedTrainer(loss="sampled_softmax", num_negatives=K, neg_counts=sampled_counts(), neg_alpha=NEG_ALPHA) draws on
    the device under the step seed word `seed_word`: (ids (K,) int64, log(K q) (K,) float32), by the numpy restatement"""
    from srfrd_amd.sampler import alias_table, negative_q
    q = negative_q(I, sampled_counts(), NEG_ALPHA)
    prob, alias = alias_table(q)
    ids = LR.ref_negatives(seed_word, I, K, prob, alias)
    log_q = np.concatenate([[0.0], np.log(K * q)]).astype(np.float32)[ids]
    return torch.from_numpy(ids), torch.from_numpy(log_q)


def head_grads(cfg, sd, batch, loss, neg=None, log_q=None, beta=1.0, remove=True, seed=0, l2_emb=0.0, double=True, parts=False):
    """The first catalog-loss step's gradient on the oracle: O.forward in training mode under the step seed, the materialised
    loss (tests/loss_refs.py) on its hidden state, mean over the positions whose target is not 0; padding rows zeroed and the
    l2_emb term added exactly as O.grads_of does.  -> (loss, {name: gradient}) in fp64 (double) or fp32; parts: also the
    item table's gradient through the loss head alone (the rest of that tensor came through the encoder's input rows)."""
    dt = torch.float64 if double else torch.float32
    leaves = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in sd.items()}
    seq, rsq, pos = batch[:3]
    h, _, _ = O.forward(cfg, leaves, seq, rsq, train=True, seed=seed, b0=0)
    item = O.key_item(cfg)
    table = leaves[item].detach().clone().requires_grad_(True)          # the head's view of the item table: its own leaf
    E = O.item_table(cfg, {item: table})
    lq = None if log_q is None else log_q.to(dt)
    if loss == "softmax":
        ce = LR.xent_mean_loss(h, E, pos)
    elif loss == "sampled_softmax":
        ce = LR.sxent_mean_loss(h, E, pos, neg, lq, remove)
    else:
        ce = LR.tneg_mean_loss(h, E, pos, neg, lq if loss == "token_softmax" else None, OBJECTIVE[loss], beta, remove)
    ce.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    head_part = table.grad.clone()
    head_part[0].zero_()
    grads[item] = grads[item] + table.grad
    grads[item][0].zero_()                                              # nn.Embedding(padding_idx=0), as O.grads_of
    if cfg.kind in ("SRFR", "SRFRN"):
        grads[O.key_side(cfg)][0].zero_()
    total = ce.detach()
    if l2_emb != 0.0:
        for k, v in leaves.items():
            nrm = torch.norm(v.detach())
            total = total + l2_emb * nrm
            if float(nrm) > 0.0:
                grads[k] = grads[k] + l2_emb * v.detach() / nrm
    return (total, grads, head_part) if parts else (total, grads)


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


HeadRef = namedtuple("HeadRef", "ref job neg log_q loss64")     # ref: a Ref; neg / log_q: what the step reads (None: "softmax")


def build_head_ref(job, seed):
    c = BY_ID[job.cid]
    cfg, batch = cfg_of(c, "head"), batch_of(c, seed)
    sd = weights(c.id, HEAD_SD_SEEDS.get((job.cid, job.loss)))
    dseed = O.step_seed(BASE, 1)
    neg = log_q = None
    if job.loss == "sampled_softmax":
        neg, log_q = sampled_negatives(dseed, job.K)
    elif job.loss in TOKEN_LOSSES:                      # (without job.with_lq the trainer is handed None and reads zeros)
        neg, log_q = token_negatives(c, batch[2], job.K, seed)
        log_q = log_q if job.with_lq else None
    kw = dict(neg=neg, log_q=log_q, beta=GBCE_BETA, remove=job.remove, seed=dseed, l2_emb=job.l2)
    loss64, g64 = head_grads(cfg, sd, batch, job.loss, double=True, **kw)
    g32 = _one_thread(lambda: head_grads(cfg, sd, batch, job.loss, double=False, **kw)[1])
    e32 = {k: tensor_figures(k, g32[k], g64[k], g32[k], cfg.D, kbias=job.l2 == 0.0)["e32"] for k in g64}
    margin = relu_margin(cfg, {k: v.double() for k, v in sd.items()}, batch, train=True, seed=dseed)
    clamp = (job.cid, "head/" + job.loss) in OVER_CAP
    return HeadRef(Ref(cfg, sd, batch, True, dseed, job.l2, g64, g32, e32, margin, clamp), job, neg, log_q, float(loss64))


@functools.lru_cache(maxsize=None)
def head_reference(job):
    """the HeadRef of one job at its HEAD_SEEDS entry, shared by every test of the process; treat as read-only"""
    return build_head_ref(job, HEAD_SEEDS[job.cid, job.loss])


# ---------------------------------------------------------------------------------------------------------------------------
# reading the device's gradients
# ---------------------------------------------------------------------------------------------------------------------------
def fused_gradients(trainer, model):
    """after ONE FusedTrainer step from zero moments: ({name: g}, {name: g ** 2}) in fp64, from exp_avg / (1 - beta1) and
    exp_avg_sq / (1 - beta2) of the optimizer state"""
    assert trainer.steps_done == 1 and trainer.betas == (BETA1, BETA2)
    state = trainer.state_dict()["state"]
    g, g2 = {}, {}
    for i, (k, _) in enumerate(model.named_parameters()):
        g[k] = state[i]["exp_avg"].detach().cpu().double() / (1.0 - BETA1)
        g2[k] = state[i]["exp_avg_sq"].detach().cpu().double() / (1.0 - BETA2)
    return g, g2
