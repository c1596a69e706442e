"""CPU side of the catalog-loss gradient checks (tests/grad_refs.py mode "head", tests/test_gpu_head_grad_fp64.py): every job's
inputs are admissible on the oracle alone, the job list covers what it claims, the recorded kernel names are the host-only
plan's, head_grads is anchored to O.grads_of, and the metric rejects the wrong gradients that stepped weights accept."""
import pytest
import torch

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests import token_trainer_refs as R
from tests.helpers import assert_post_adam
from tests.test_encoder_plan import N_CU

IDS = [G.head_id(j) for j in G.HEAD_JOBS]


@pytest.mark.parametrize("job", G.HEAD_JOBS, ids=IDS)
def test_head_job_inputs_are_admissible(job):
    """on the oracle alone (the GPU tests assert it again where they compute their bounds); the fp32 oracle itself inside its
    bound; and the negatives carry the edges the job is there for"""
    href = G.head_reference(job)
    ref = href.ref
    G.assert_admissible(ref, f"head {G.head_id(job)}")
    assert ref.train and ref.cfg.dropout == 0.5 and ref.seed == O.step_seed(G.BASE, 1)
    assert all(G.bound(e, ref.clamp) >= G.R_MIN and (not ref.clamp or G.bound(e, True) <= G.CAP) for e in ref.e32.values())
    figs = G.compare(ref.g32, ref)
    assert not any(G.failures(f) for f in figs.values())
    assert any("kbias" in f for f in figs.values()) == (job.l2 == 0.0)
    pos, neg = ref.batch[2], href.neg
    live = pos != 0
    if job.loss in G.TOKEN_LOSSES:
        assert neg.shape == pos.shape + (job.K,) and not bool(neg[~live].any())
        unused, hits = (neg == 0) & live.unsqueeze(-1), (neg == pos.unsqueeze(-1)) & live.unsqueeze(-1)
        assert bool(unused.any()) and bool(hits.any()) and bool(((neg != 0) & ~hits).any())
        assert bool((unused.all(-1) & live).any())                  # a live position with all K slots unused
        assert (href.log_q is not None) == job.with_lq
        if job.with_lq:
            assert not bool(href.log_q[~live].any()) and 0.8 < float(href.log_q[live].std()) < 1.2
        # the step's own key list through the restated addressing of the mixed reduction: every index in range
        T, d = pos.numel(), G.BY_ID[job.cid].d_item
        keys = R.step_keys(ref.batch[0].numpy(), pos.numpy(), neg.numpy(), G.I, job.remove)
        assert keys.shape[0] == T * (2 + job.K)
        R.audit_indices(keys, T, 1 + job.K, T, G.I, d, R.ws_floats(keys.shape[0], d))
    elif job.loss == "sampled_softmax":
        assert neg.shape == (G.K_SAMPLED,) and int(neg.min()) >= 1 and int(neg.max()) <= G.I
        assert bool((neg.unsqueeze(0) == pos[live].unsqueeze(1)).any())             # accidental hits
        assert href.log_q.dtype == torch.float32 and float(href.log_q.std()) > 0.1
    else:
        assert neg is None and href.log_q is None
    if job.cid.startswith("t"):         # targets on padded positions: the head's range begins before the encoder's
        assert all(bool(((ref.batch[0][b] == 0) & (pos[b] != 0)).any()) for b in (5, 11))


def _family(bwd):
    if bwd.startswith("srfrd_long::"):
        return "long"
    for key, fam in (("bwd_slots", "slots"), ("bwd_chunks", "chunks"), ("bwd_ragged", "ragged"), ("encoder_bwd_kernel<", "first")):
        if key in bwd:
            return fam
    raise AssertionError(bwd)


def test_head_jobs_cover_what_they_claim():
    jobs = [j for j in G.HEAD_JOBS if not j.l2]
    pairs = {(j.cid, j.loss) for j in jobs}
    assert len(pairs) == len(jobs) and set(G.HEAD_SEEDS) == pairs
    srfrn = lambda cid: G.BY_ID[cid].kind == "SRFRN"
    default = {(cid, loss) for cid in G.DEFAULT_IDS for loss in G.HEAD_LOSSES if not (loss == "gbce" and srfrn(cid))}
    assert len(default) == 22 and default <= pairs
    assert not any(j.loss == "gbce" and srfrn(j.cid) for j in jobs)
    assert {j.cid for j in jobs} == {c.id for c in G.DEPTH2_CASES}          # (the head mode stays at two blocks)
    assert all(G.HEAD_NAMES[cid][1].startswith("srfrd::encoder_bwd_ragged_kernel<") for cid in G.DEFAULT_IDS)
    met = {(j.loss, _family(G.HEAD_NAMES[j.cid][1])) for j in jobs}
    assert {(loss, fam) for loss in G.HEAD_LOSSES for fam in ("first", "slots", "chunks", "long", "ragged")} <= met
    assert {G.HEAD_NAMES[j.cid][1] for j in jobs} == {c.autograd[1] for c in G.DEPTH2_CASES}      # every non-training backward
    for loss in G.TOKEN_LOSSES:
        mine = [j for j in jobs if j.loss == loss]
        assert {j.remove for j in mine} == {True, False} and {j.with_lq for j in mine} == {True, False}
        assert {j.K for j in mine if j.cid.startswith("u")} == {65} and {j.K for j in mine if not j.cid.startswith("u")} == {5}
    assert all(j.K == 96 for j in jobs if j.loss == "sampled_softmax")
    assert [(j.cid, j.loss, j.l2) for j in G.HEAD_JOBS if j.l2] == [(G.L2_ID, loss, G.L2_EMB) for loss in G.HEAD_L2]
    assert {k for k in G.OVER_CAP if k[1].startswith("head/")} <= {(j.cid, "head/" + j.loss) for j in jobs}


@pytest.mark.parametrize("c", G.DEPTH2_CASES, ids=[c.id for c in G.DEPTH2_CASES])
def test_head_names_are_the_plans(c):
    """the names each GPU job asserts before its step, against the host-only plan under the head launch's mode bits"""
    lay = _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)
    sw = _lib.SWITCHES[c.switch] if c.switch else 0
    assert F._plan_bits()["head"] == (_lib.PLAN_CKPT | _lib.PLAN_DROPOUT, _lib.PLAN_DROPOUT)
    assert F.planned(lay, c.B, c.L, "head", sw, N_CU, *F.case_scratch(lay, c.B, c.L, "head")) == G.HEAD_NAMES[c.id]


# ---------------------------------------------------------------------------------------------------------------------------
# anchor
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["t0", "t1", "t3"])
def test_gbce_k1_beta1_is_the_bce_oracle(cid):
    """K = 1, beta = 1, no hit removal, the batch's own negative plane: head_grads(..., "gbce") is O.grads_of on the same batch
    (training mode, the step seed), in fp64 to 1e-12 of each tensor's largest element - with and without l2_emb"""
    c = G.BY_ID[cid]
    cfg, sd, batch = G.cfg_of(c, "head"), G.weights(cid), G.batch_of(c, G.SEEDS[cid, "fused"])
    pos, neg = batch[2], batch[4]
    assert bool((neg[pos != 0] != 0).all())                         # every target has its negative: no unused slot
    seed = O.step_seed(G.BASE, 1)
    for l2 in (0.0, G.L2_EMB):
        want_loss, want = O.grads_of(cfg, {k: v.double() for k, v in sd.items()}, batch, train=True, seed=seed, b0=0, l2_emb=l2)[:2]
        loss, got = G.head_grads(cfg, sd, batch, "gbce", neg=neg.unsqueeze(-1), beta=1.0, remove=False, seed=seed, l2_emb=l2)
        assert abs(float(loss) - float(want_loss)) <= 1e-12 * abs(float(want_loss))
        assert set(got) == set(want)
        for k in want:
            assert float((got[k] - want[k]).abs().max()) <= 1e-12 * float(want[k].abs().max()), (k, l2)


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------
SHARP_CASE = "t0"         # SASRec, the tile-boundary batch, 17 sequences
# The wrong gradients below that the stepped weights accept (tests/helpers.assert_post_adam after one oracle Adam step with the
# wrong gradient, against the step with the right one): the gap these tests close.  Adam's first step moves an element by
# lr g / (|g| + eps), so a constant factor on the whole gradient - a lost or doubled 1 / count - cannot be seen at all.  What
# the stepped weights make of the other wrong gradients is printed; at these inputs (one exact Adam step in fp64, nothing else
# differing) they reject them, and a value in item row 0 they must reject: that element's tolerance is 1e-7.
POST_ADAM_ACCEPTS = ["whole gradient times 0.5", "whole gradient times the target count"]


def _head_mutations(href):
    ref, job = href.ref, href.job
    item = O.key_item(ref.cfg)
    kw = dict(neg=href.neg, log_q=href.log_q, beta=G.GBCE_BETA, remove=job.remove, seed=ref.seed, l2_emb=job.l2)
    again = lambda **over: G.head_grads(ref.cfg, ref.sd, ref.batch, job.loss, **dict(kw, **over))[1]
    yield "whole gradient times 0.5", {k: 0.5 * v for k, v in ref.g64.items()}
    count = int((ref.batch[2] != 0).sum())
    yield "whole gradient times the target count", {k: count * v for k, v in ref.g64.items()}

    _, g, head_part = G.head_grads(ref.cfg, ref.sd, ref.batch, job.loss, parts=True, **kw)
    assert all(torch.equal(g[k], ref.g64[k]) for k in g) and bool((head_part != 0).any()) and bool((g[item] != head_part).any())
    m = {k: v.clone() for k, v in ref.g64.items()}
    m[item] = m[item] + 0.01 * head_part
    yield "head's part of the item table times 1.01", m

    if job.loss in ("sampled_softmax", "token_softmax"):
        yield "log_q dropped", again(log_q=None)
    if job.loss != "softmax":
        yield "hit removal inverted", again(remove=not job.remove)
    if job.loss == "gbce":
        yield "beta = 1", again(beta=1.0)

    m = {k: v.clone() for k, v in ref.g64.items()}
    m[item][0, 3] = 1e-3 * float(m[item].abs().max())
    yield "a non-zero value in item row 0", m


def _post_adam_accepts(ref, wrong):
    right = {k: v.double().clone() for k, v in ref.sd.items()}
    moved = {k: v.clone() for k, v in right.items()}
    O.Adam(right, lr=1e-3, betas=(G.BETA1, G.BETA2)).step(right, ref.g64)
    O.Adam(moved, lr=1e-3, betas=(G.BETA1, G.BETA2)).step(moved, wrong)
    try:
        assert_post_adam(moved, right, [{k: g.float() for k, g in ref.g64.items()}], ref.cfg.D)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("loss", G.HEAD_LOSSES)
def test_metric_rejects_what_stepped_weights_accept(loss):
    href = G.head_reference(G.head_job(SHARP_CASE, loss))
    ref = href.ref
    assert ref.cfg.kind == "SASRec" and not any(G.failures(f) for f in G.compare(ref.g64, ref).values())
    assert _post_adam_accepts(ref, ref.g64)
    names, accepted = [], []
    for name, mut in _head_mutations(href):
        figs = G.compare(mut, ref)
        bad = {k: G.failures(f) for k, f in figs.items() if G.failures(f)}
        with pytest.raises(AssertionError):
            G.assert_holds(figs, name)
        ok = _post_adam_accepts(ref, mut)
        print(f"{loss}: {name}: rejected on {len(bad)} tensors; stepped weights {'accept' if ok else 'reject'} it")
        assert bad, name
        names.append(name)
        if ok:
            accepted.append(name)
    assert len(names) == {"softmax": 4, "sampled_softmax": 6, "token_softmax": 6, "gbce": 6}[loss]
    assert accepted[:2] == POST_ADAM_ACCEPTS and "a non-zero value in item row 0" not in accepted
