"""The width and head-split cases of the run-time-geometry encoder kernels (no GPU): sixteen cases, their seeds, and the wrong
head splits the references must tell apart.

``srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>`` / ``encoder_bwd_kernel<0,0,0,0,-1,0,0>`` and their ``srfrd_long::`` builds serve
every layout whose hidden width is not 50 or that has more than one head; in them NT = ceil(D / 16), DK = ceil4(D), the row
strides DS = DK + 2 and SLD = LP + 2, the ``c < D`` guards, the per-head column windows ``[c0, c0 + dh)``, the H probability
planes of the checkpoint, SRFR's ``last_conv`` tiles and every (position, channel) walk are run-time values.  grad_refs.ALL_CASES
meets them at D = 50 (one and two heads) and D = 40 (one head) only.  The cases below, one per seam, run through the fp64
suites' own runners (tests/test_gpu_geom_fp64.py) under grad_refs' and fwd_refs' reference, metric and bound rule, unchanged;
they live here, registered in ``grad_refs.OTHER`` - ``grad_refs.ALL_CASES`` does not grow.

All cases: two blocks, I = 300, no switch, B = 6 below seq_len 100 and 5 from there on.

  id     kind     d_item + d_fake  heads (dh)  L    the seam
  w64a   SASRec   64               1           20   NT = 4, every lane a live channel: no ``c < D`` guard is ever false
  w64b   SASRec   64               4 (16)      50   LP = 64: the backward's LDS no longer fits at this width (LDS forward,
                                                    srfrd_long:: backward)
  w64c   SRFU_B   64               8 (8)       37   the label vector at width 64, odd LP = 48
  w64d   SRFR     59 + 5           1           48   last_conv over 4 tiles, d_out = 59 < D; LP = 48 is the last length whose
                                                    backward stays in LDS at width 64
  w64e   SASRec   64               2 (32)      100  LP = 112: the forward leaves LDS too (both srfrd_long::)
  w63    SRFRN    58 + 5           7 (9)       50   DK = 64 > D, odd D, head windows off every 4-column k-step (the LDS is
                                                    sized by DK: LDS forward, srfrd_long:: backward, as w64b)
  w33    SASRec   33               3 (11)      50   NT = 3 with one live column in the last tile, DK = 36
  w32a   SRFR     27 + 5           1           50   last_conv over 2 tiles, d_out = 27
  w32b   SASRec   32               4 (8)       100  narrow and long: S (LP x SLD) is the larger overlay of imax(LP DS, LP SLD)
  w17    SASRec   17               17 (1)      33   dh = 1, seventeen turns in the S buffer, DK = 20, LP = 48
  w16a   SRFU_B   16               2 (8)       50   NT = 1
  w16b   SRFRN    11 + 5           1           16   L = LP = 16: one row tile, the side channel in a 16-wide state
  w8     SASRec   8                2 (4)       16   half a column tile, dh equal to one k-step
  w4     SASRec   4                4 (1)       20   DK = 4: one k-step per GEMM, nthr / D at its largest
  h5     SRFRN    45 + 5           5 (10)      50   the default width with the _h5 golden's split, at the default length
  h10    SASRec   50               10 (5)      100  dh = 5 at seq_len 100

Seeds follow grad_refs.SEEDS' rule (``grad_refs.scan_seeds`` / ``pick_seed``, ``fwd_refs.scan_seeds`` / ``pick_seed``; the tool
is tools/geom_fp64_report.py --scan / --pick); the comments at the tables say which scans were made.
"""
import dataclasses
import functools

from oracle import srfrd_oracle as O
from tests import fwd_refs as R
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests.test_gpu_bf16_families import Case

# the three pairs of generic kernels, as srfrd_encoder_plan prints them on the built library (tests/test_geom_cover.py holds
# every case's names to the host-only plan in all four launch modes)
LDS_LDS = ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>")
LDS_LONG = ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>")
LONG_LONG = ("srfrd_long::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>")
PAIRS = (LDS_LDS, LDS_LONG, LONG_LONG)
FIRST_SEED = 50           # every job's scan starts here (Case.seed and Case.fused_seed, which grad_refs.first_seed reads)


def _case(cid, kind, d_item, d_fake, heads, L, B, pair):
    return Case(cid, kind, d_item, d_fake, heads, L, B, None, FIRST_SEED, FIRST_SEED, **F._same(*pair))


CASES = [
    _case("w64a", "SASRec", 64, 0, 1, 20, 6, LDS_LDS),
    _case("w64b", "SASRec", 64, 0, 4, 50, 6, LDS_LONG),
    _case("w64c", "SRFU_B", 64, 0, 8, 37, 6, LDS_LDS),
    _case("w64d", "SRFR", 59, 5, 1, 48, 6, LDS_LDS),
    _case("w64e", "SASRec", 64, 0, 2, 100, 5, LONG_LONG),
    _case("w63", "SRFRN", 58, 5, 7, 50, 6, LDS_LONG),        # (DK = 64 sizes the LDS: LP = 64 as w64b)
    _case("w33", "SASRec", 33, 0, 3, 50, 6, LDS_LDS),
    _case("w32a", "SRFR", 27, 5, 1, 50, 6, LDS_LDS),
    _case("w32b", "SASRec", 32, 0, 4, 100, 5, LDS_LONG),
    _case("w17", "SASRec", 17, 0, 17, 33, 6, LDS_LDS),
    _case("w16a", "SRFU_B", 16, 0, 2, 50, 6, LDS_LDS),
    _case("w16b", "SRFRN", 11, 5, 1, 16, 6, LDS_LDS),
    _case("w8", "SASRec", 8, 0, 2, 16, 6, LDS_LDS),
    _case("w4", "SASRec", 4, 0, 4, 20, 6, LDS_LDS),
    _case("h5", "SRFRN", 45, 5, 5, 50, 6, LDS_LDS),
    _case("h10", "SASRec", 50, 0, 10, 100, 5, LDS_LONG),
]
BY_ID = {c.id: c for c in CASES}
GRAD_MODES = ("autograd", "fused")
GRAD_JOBS = [(c.id, m) for c in CASES for m in GRAD_MODES]
FWD_JOBS = [(c.id, m) for c in CASES for m in R.MODES]


def width(c):
    """the hidden width D"""
    return c.d_item + (c.d_fake if c.kind in ("SRFR", "SRFRN") else 0)


def geometry(c):
    """the run-time values the generic kernels derive from a case: D, NT, DK, LP, dh, d_out and last_conv's tile count (0: none)"""
    D = width(c)
    d_out = c.d_item if c.kind == "SRFR" else D
    return dict(D=D, NT=(D + 15) // 16, DK=(D + 3) & ~3, LP=(c.L + 15) & ~15, dh=D // c.heads, d_out=d_out,
                conv_tiles=(c.d_item + 15) // 16 if c.kind == "SRFR" else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# seeds
# ---------------------------------------------------------------------------------------------------------------------------
# (case id, mode) -> batch seed, by grad_refs.SEEDS' rule: from 50 on, the first of 200 batches at which on EVERY scan
# relu_margin >= 2 * RELU_MARGIN and 64 e32 <= SEARCH_HEADROOM * CAP for every tensor.
# Three scans of 200 batches a job: an Intel Xeon with the BLAS library's default code path, the same machine with
# MKL_CBWR=AVX2, and the GPU host's CPU (an AMD EPYC 9575F); each under weight seeds 7 and 8.  Under weight seed 7 the third
# scan moved nine picks and took three jobs' seeds away (w63 autograd, w16a autograd, h5 autograd); one batch differs by up to
# 47 % between scans (h5 autograd at 142: 1.36e-6, 9.2e-7, 9.4e-7).
GEOM_SEEDS = {
    ("w64a", "autograd"): 50, ("w64a", "fused"): 55, ("w64b", "autograd"): 50, ("w64b", "fused"): 50,
    ("w64c", "autograd"): 220, ("w64c", "fused"): 126, ("w64d", "autograd"): 66, ("w64d", "fused"): 217,
    ("w64e", "autograd"): 62, ("w64e", "fused"): 50, ("w63", "autograd"): 108, ("w63", "fused"): 174,
    ("w33", "autograd"): 50, ("w33", "fused"): 51, ("w32a", "autograd"): 57, ("w32a", "fused"): 62,
    ("w32b", "autograd"): 51, ("w32b", "fused"): 50, ("w17", "autograd"): 51, ("w17", "fused"): 50,
    ("w16a", "autograd"): 238, ("w16a", "fused"): 200, ("w16b", "autograd"): 51, ("w16b", "fused"): 51,
    ("w8", "autograd"): 52, ("w8", "fused"): 52, ("w4", "autograd"): 69, ("w4", "fused"): 86,
    ("h5", "autograd"): 99, ("h5", "fused"): 94, ("h10", "autograd"): 53, ("h10", "fused"): 53,
}
# Weights: random_sd(cfg, grad_refs.SD_SEED), but for w32a and h5 the next weight seed, as grad_refs.SD_SEEDS: under SD_SEED
# w32a autograd and both jobs of h5 have no batch of 200 with the headroom on all three scans (best 1.53e-6, 1.36e-6, 1.66e-6);
# under 8 all four jobs of the two cases have one.  The same was tried for w64c, w64d, w63, w16a and w4: no batch of 200 either
# (w16a then loses its fused seed too), so they keep SD_SEED.
GEOM_SD_SEEDS = {"w32a": 8, "h5": 8}
# Jobs without such a seed: bound clamped at CAP - tighter than 64 e32 where it acts, never wider - at the scanned batch with
# the ReLU margin whose e32 is smallest on its worst scan (autograd / fused): w64c 1.93e-6 / 1.56e-6 and w64d 1.69e-6 / 1.39e-6
# (SRFU_B and SRFR at width 64: the kinds grad_refs.OVER_CAP documents), w63 1.39e-6 / 1.40e-6 (SRFRN, seven heads), w16a
# autograd 1.30e-6, w4 fused 1.26e-6: the last four under the condition on all three scans, without the headroom that would
# promise it on a fourth.  MAX_GEOM_OVER_CAP of the 32 jobs at most (tests/test_geom_refs.py).
GEOM_OVER_CAP = frozenset([(c, m) for c in ("w64c", "w64d", "w63") for m in ("autograd", "fused")]
                          + [("w16a", "autograd"), ("w4", "fused")])
MAX_GEOM_OVER_CAP = 8
# the forward modes keep the gradient job's seed (eval, last: autograd's; train: fused's) unless 16 e32 > SEARCH_HEADROOM * CAP_FWD
# on some scan, as fwd_refs.FWD_SEEDS.  None does, on the same three scans (every batch from 50 to 249): all 48 jobs keep their
# seed; worst e32 on the worse scan 1.21e-6 (w64a eval) of the 1.25e-6 the headroom allows, then 1.11e-6 (w64e
# train) and 1.05e-6 (h10 train).
GEOM_FWD_SEEDS = {}
GEOM_FWD_OVER_CAP = frozenset()
MAX_GEOM_FWD_OVER_CAP = 4

G.OTHER.update({c.id: c for c in CASES})
G.OTHER_SEEDS.update(GEOM_SEEDS)
G.OTHER_SD_SEEDS.update(GEOM_SD_SEEDS)
G.OTHER_OVER_CAP.update(GEOM_OVER_CAP)
R.OTHER_FWD_SEEDS.update(GEOM_FWD_SEEDS)
R.OTHER_FWD_OVER_CAP.update(GEOM_FWD_OVER_CAP)


def case_ids(cases=None):
    return G.case_ids(cases or CASES)


def scan_job(job):
    """(case id, mode, count, weight seed | None) -> grad_refs.scan_seeds' rows on THIS machine's CPU, under another weight seed
    where one is given.  A forward mode: fwd_refs.scan_seeds' rows, but from FIRST_SEED on whatever the gradient job's seed is
    (`forward_rows` cuts them there), so that one visit to a machine scans both."""
    cid, mode, count, sd_seed = job
    if sd_seed is not None:
        G.OTHER_SD_SEEDS[cid] = sd_seed
        G.weights.cache_clear()
    if mode not in R.MODES:
        return G.scan_seeds((cid, mode, count))
    return [[seed, R.worst_e32(R.build_ref(BY_ID[cid], mode, seed)), 1.0] for seed in range(FIRST_SEED, FIRST_SEED + count)]


def forward_rows(cid, mode, rows):
    """the rows fwd_refs.pick_seed reads: from the gradient job's seed on"""
    first = G.seed_of(cid, "fused" if mode == "train" else "autograd")
    return [r for r in rows if r[0] >= first]


# ---------------------------------------------------------------------------------------------------------------------------
# the bf16 shadow at two of the widths (tests/test_gpu_geom_fp64.py runs test_gpu_bf16_families' four checks on them)
# ---------------------------------------------------------------------------------------------------------------------------
# w33: a 66-byte shadow row; w64b: 128 bytes behind the srfrd_long:: backward.  `seed` / `fused_seed` by that file's rule, on the
# CPU oracle (tests/test_geom_refs.py): from 6 / 50 on the first seeds at which every user's top-11 gaps exceed 3 TOL, the bf16
# and the fp32 oracle's positive logits differ by 20 TOL and relu_margin exceeds 2 RELU_MARGIN (fused: at both steps' batches).
BF16_SEEDS = {"w33": (6, 50), "w64b": (6, 51)}         # (w64b's fused batch 50: a ReLU input 4.4e-6 from zero)
BF16_CASES = [BY_ID[cid]._replace(seed=s, fused_seed=fs) for cid, (s, fs) in BF16_SEEDS.items()]


def bf16_conditions(c, seed=None, fused_seed=None):
    """-> (smallest top-11 gap, max |pos logits bf16 - fp32|, ReLU margin at `seed`, the smaller ReLU margin of the two fused
    steps) of a bf16 case on the CPU oracle alone, with the weights test_gpu_bf16_families._setup builds"""
    import numpy as np
    import srfrd_amd
    import torch
    from tests.gpu_util import random_sd
    seed, fused_seed = seed or c.seed, fused_seed or c.fused_seed
    cfg = F.cfg_of(c)
    sd = random_sd(cfg, 7)
    batch = srfrd_amd.synthetic_batch(F.I, c.L, c.B, seed=seed, device="cpu")[1:]
    ref = O.predict(cfg, sd, batch[0], batch[1], torch.arange(1, F.I + 1))
    top = -np.sort(-ref.numpy(), axis=1)[:, :11]
    gap = float((top[:, :-1] - top[:, 1:]).min())
    _, pl, _ = O.forward(cfg, sd, *batch)
    _, pl32, _ = O.forward(F.cfg_of(c, bf16=False), sd, *batch)
    margin = F.relu_margin(cfg, sd, batch)
    # the two fused steps as that file's test takes them: the second batch meets the weights the oracle's first step left
    from tests.helpers import oracle_step_with_grads
    cfg5, sd5, fused = F.cfg_of(c, dropout=0.5), {k: v.clone() for k, v in sd.items()}, float("inf")
    opt = O.Adam(sd5)
    for s in range(2):
        step = srfrd_amd.synthetic_batch(F.I, c.L, c.B, seed=fused_seed + s, device="cpu")[1:]
        fused = min(fused, F.relu_margin(cfg5, sd5, step, train=True, seed=O.step_seed(G.BASE, s + 1)))
        oracle_step_with_grads(cfg5, sd5, opt, step, train=True, seed=O.step_seed(G.BASE, s + 1), b0=0)
    return gap, float((pl - pl32).abs().max()), margin, fused


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness: the same weights and batch under another head split, on the fp64 oracle alone
# ---------------------------------------------------------------------------------------------------------------------------
MULTI_HEAD = [c for c in CASES if c.heads > 1]
SHARP_BOUNDS = 100.0      # a wrong split lies at least this many bounds from the case's own reference


def wrong_splits(c):
    """the head counts a broken window would amount to: one head, and for even H > 2 half as many"""
    return [1] + ([c.heads // 2] if c.heads > 2 and c.heads % 2 == 0 else [])


def attention_weights(ref):
    return [k for k in ref.g64 if k.endswith("in_proj_weight") or k.endswith("out_proj.weight")]


@functools.lru_cache(maxsize=None)
def split_distances(cid, heads):
    """(worst forward output, least-affected attention weight gradient) of case `cid` computed with `heads` heads, each as a
    multiple of the bound of the case's own reference (eval mode / autograd mode)"""
    import torch
    fref, gref = R.reference(cid, "eval"), G.reference(cid, "autograd")
    cfg = dataclasses.replace(fref.cfg, num_heads=heads)
    sd64 = {k: v.detach().double() for k, v in fref.sd.items()}
    with torch.no_grad():
        h, pl, nl = O.forward(cfg, sd64, *fref.batch)
    x = {"hidden": h, "pos_logits": pl, "neg_logits": nl}
    fwd = max(R.row_errors_inf(x[k], fref.x64[k]) / R.bound(fref.e32[k], fref.clamp) for k in fref.x64)
    g = G.fp64_grads(dataclasses.replace(gref.cfg, num_heads=heads), gref.sd, gref.batch)
    grad = min(G.row_errors(g[k], gref.g64[k]) / G.bound(gref.e32[k], gref.clamp) for k in attention_weights(gref))
    return fwd, grad
