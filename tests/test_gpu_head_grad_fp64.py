"""-m gpu, fp32 item table: the gradient inside the first FusedTrainer(loss="softmax" | "sampled_softmax" | "token_softmax" |
"gbce") step against the fp64 oracle, relative to each row's own size (tests/grad_refs.py, mode "head": reference, jobs, seeds;
tests/test_grad_refs_head.py: their CPU side).

The four catalog-loss steps met an oracle only through stepped weights (tests/helpers.assert_post_adam), which cannot show a
gradient's scale: a lost 1 / count, head rows mis-scaled against the encoder's input rows inside one item row, or a leak into
item row 0 all pass there.  As tests/test_gpu_grad_fp64.py does for the BCE step, the gradient is read from Adam's moments after
ONE step from fresh moments (exp_avg / (1 - beta1), exp_avg_sq / (1 - beta2)) and held to grad_refs.head_grads: O.forward in
training mode under the step's seed word, the materialised loss on its hidden state.

The step also runs an encoder combination nothing else holds tightly: the non-training instantiations (plan bits CKPT | DROPOUT
and DROPOUT alone) with dropout masks on and the gradient entering through d_hidden.  Its planned kernel names
(grad_refs.HEAD_NAMES) are asserted before the step.

Jobs (grad_refs.HEAD_JOBS): every loss on the default-geometry cases (ragged pair: the tile-boundary batch, whose rows 5 and 11
keep targets on padded positions, and the duplicate-heavy batch, K = 65 there), every other case of ALL_CASES under one loss
(two on the srfrd_long:: backward's cases), two l2_emb jobs.  "softmax" runs under both `deterministic` values (de_ce + add
versus accumulate in place); the other losses ignore the flag.  Sampled negatives: the device's draw must equal the numpy
restatement bit for bit before the reference computed from the restatement is used.  profiles/grad_fp64_errors.json holds the
measured figures (tools/grad_fp64_report.py calls run_head below).
"""
import pytest
import torch

from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests.test_gpu_grad_fp64 import _model

pytestmark = pytest.mark.gpu

RUNS = [(j, det) for j in G.HEAD_JOBS for det in ((True, False) if j.loss == "softmax" else (False,))]
RUN_IDS = [G.head_id(j) + (("-deterministic" if det else "-atomics") if j.loss == "softmax" else "") for j, det in RUNS]


def run_head(job, det, setenv):
    """-> (figures of exp_avg / (1 - beta1), figures of exp_avg_sq / (1 - beta2) against g64^2) after one step"""
    import srfrd_amd
    from tests.gpu_util import cuda
    c = G.BY_ID[job.cid]
    what = f"head {G.head_id(job)}"
    href = G.head_reference(job)
    ref = href.ref
    G.assert_admissible(ref, what)                              # (e32 is this machine's: the bounds below come from it)
    model = _model(c, ref, setenv)
    kw = {}
    if job.loss == "sampled_softmax":
        kw = dict(num_negatives=job.K, neg_counts=G.sampled_counts(), neg_alpha=G.NEG_ALPHA)
    elif job.loss in G.TOKEN_LOSSES:
        kw = dict(num_negatives=job.K, gbce_beta=G.GBCE_BETA, remove_accidental_hits=job.remove)
    tr = srfrd_amd.FusedTrainer(model, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=False, deterministic=det, l2_emb=job.l2,
                                loss=job.loss, **kw)
    F._assert_plan(c, model, "head", G.HEAD_NAMES[c.id], scratch=tr.n_scratch)
    seq, rsq, pos, prs, _, _ = cuda(*ref.batch)
    if job.loss in G.TOKEN_LOSSES:
        loss = tr.step(None, seq, rsq, pos, prs, href.neg.cuda(), None, log_q=href.log_q.cuda() if job.with_lq else None)
    else:
        loss = tr.step(None, seq, rsq, pos, prs, None, None)
    tr.check()
    if job.loss == "sampled_softmax":                          # the reference was computed from the restatement's draw
        assert torch.equal(tr.negatives.cpu(), href.neg) and torch.equal(tr.log_q.cpu(), href.log_q), what
    got = float(loss)
    print(f"{what}: loss {got:.7f}, fp64 {href.loss64:.7f}")
    assert bool(torch.isfinite(loss).all()), what
    assert abs(got - href.loss64) <= 1e-5 * max(1.0, abs(href.loss64)), (what, got, href.loss64)
    g, g2 = G.fused_gradients(tr, model)
    return G.compare(g, ref), G.compare(g2, ref, squares=True)


@pytest.mark.parametrize("job,det", RUNS, ids=RUN_IDS)
def test_head_step_gradients_meet_the_fp64_oracle(job, det, monkeypatch):
    figs, figs2 = run_head(job, det, monkeypatch.setenv)
    what = f"head {G.head_id(job)} det={det}"
    G.assert_holds(figs, what)
    G.assert_holds(figs2, what + " second moment")
