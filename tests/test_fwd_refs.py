"""CPU side of the fp64 forward checks (tests/fwd_refs.py, tests/test_gpu_fwd_fp64.py): every job's inputs are admissible on the
oracle alone, the case list is the gradient suite's and every mode has a kernel name the host-only plan confirms, the fp64
oracle's forward is the REFERENCE's (the golden fixtures), and the metric rejects the wrong forwards the old absolute bar
accepts - a pad row left unwritten among them."""
import pytest
import torch

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests import fwd_refs as R
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests.helpers import DROP_CASES, HEAD_CASES, KINDS, golden_cfg, load_drop, load_golden
from tests.test_encoder_plan import N_CU

JOBS = [(c.id, mode) for c in R.ALL_CASES for mode in R.MODES]


@pytest.mark.parametrize("cid,mode", JOBS, ids=[f"{cid}-{mode}" for cid, mode in JOBS])
def test_job_inputs_are_admissible(cid, mode):
    """on the oracle alone (fwd_refs.assert_admissible; the GPU tests assert it again where they compute their bounds), and the
    fp32 oracle itself inside its bound"""
    ref = R.reference(cid, mode)
    R.assert_admissible(ref, f"case {cid} {mode}")
    assert set(ref.x64) == set(R.OUTPUTS[mode])
    figs = R.compare(ref.x32, ref)
    assert all(R.holds(f) and f["bound"] >= R.R_MIN_FWD and (not ref.clamp or f["bound"] <= R.CAP_FWD) for f in figs.values())
    if mode != "last":
        loss64, e32 = R.loss_reference(ref)
        print(f"case {cid} {mode}: loss {loss64:.6f}, e32 {e32:.1e}")
        assert R.FACTOR_FWD * e32 <= R.CAP_FWD and loss64 > 0.0


def test_case_list_seeds_and_the_over_cap_set():
    assert R.ALL_CASES is G.ALL_CASES
    jobs = set(JOBS)
    assert R.FWD_OVER_CAP <= jobs and len(R.FWD_OVER_CAP) <= R.MAX_OVER_CAP == len(jobs) // 10
    assert set(R.FWD_SEEDS) <= jobs
    assert all(R.seed_of(c.id, "eval") == G.SEEDS[c.id, "autograd"] and R.seed_of(c.id, "train") == G.SEEDS[c.id, "fused"]
               for c in R.ALL_CASES if not {(c.id, m) for m in R.MODES} & set(R.FWD_SEEDS))
    # the tile-boundary batch brings what the metric's pad rows need: an all-pad sequence, an interior pad, targets on pads
    seq, _, pos, _, _, _ = R.reference("t0", "eval").batch
    assert bool((seq[16] == 0).all()) and int(seq[3, 27]) == 0 and bool(((seq[5] == 0) & (pos[5] != 0)).any())
    shared, user = R.reference("k", "last").cands
    assert shared.tolist() == list(range(1, G.I + 1)) and user.shape == (5, R.N_CAND_USER)
    assert all(0 in row and len(set(row)) < len(row) for row in user.tolist())


@pytest.mark.parametrize("c", R.ALL_CASES, ids=[c.id for c in R.ALL_CASES])
def test_every_mode_has_the_plans_kernel_name(c):
    """the name each GPU run asserts before it launches, against the host-only plan under the mode bits the launchers derive"""
    lay = _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)
    sw = _lib.SWITCHES[c.switch] if c.switch else 0
    scratch = _lib.scratch_floats(lay, c.B, c.L)[0]          # (the module path sizes it per direction)
    for mode in R.MODES:
        name = R.plan_name(c, mode)
        assert name and _lib.encoder_plan(lay, c.B, c.L, R.plan_bits(mode), sw, N_CU, scratch)[0][0] == name, (c.id, mode)
    bits = F._plan_bits()
    assert R.plan_bits("eval") == bits["eval"][0] and R.plan_bits("last") == bits["last"][0]
    assert R.plan_bits("train") == bits["autograd"][0] | _lib.PLAN_DROPOUT


def test_loss_reference_is_the_gradient_oracles_loss():
    """fwd_refs.loss_reference on the fused step's batch is ``O.grads_of(...)[0]`` on the double weights, l2_emb term included"""
    for cid, l2 in ((G.L2_ID, 0.0), (G.L2_ID, G.L2_EMB), ("k", 0.0)):
        ref = R.fused_step_reference(cid)
        g = G.reference(cid, "fused", l2)
        assert ref.seed == g.seed and all(torch.equal(a, b) for a, b in zip(ref.batch, g.batch))
        want = O.grads_of(g.cfg, {k: v.double() for k, v in g.sd.items()}, g.batch, train=True, seed=g.seed, b0=0, l2_emb=l2)[0]
        loss64, e32 = R.loss_reference(ref, l2)
        assert abs(loss64 - float(want)) <= 1e-13 * float(want) and e32 < 1e-6
    assert R.loss_reference(R.fused_step_reference(G.L2_ID), G.L2_EMB)[0] > R.loss_reference(R.fused_step_reference(G.L2_ID))[0] + 1e-3


# ---------------------------------------------------------------------------------------------------------------------------
# the fp64 oracle's forward is the reference's
# ---------------------------------------------------------------------------------------------------------------------------
STORAGE = 2.0 ** -23        # one fp32 ulp of the row's maximum: twice what rounding an fp64 result to fp32 storage costs


def _anchor(gold, x64, x32, storage=False):
    """A fixture that holds what the reference's own classes computed in fp32 is held like a device output; its inputs are what
    they are - no seed to choose - so the bound is clamped at CAP_FWD as for a FWD_OVER_CAP job.  storage: the reference ran in
    fp64 and only the stored result is fp32 - held to STORAGE."""
    for k in gold:
        fig = R.figures(torch.from_numpy(gold[k]).reshape(x64[k].shape), x64[k], x32[k], clamp=True)
        limit = STORAGE if storage else fig["bound"]
        print(f"  {k}: {fig['err']:.2e} of {limit:.2e} (e32 {fig['e32']:.2e})")
        assert limit <= R.CAP_FWD and fig["err"] <= limit, (k, fig)


@pytest.mark.parametrize("kind,heads", [(k, 1) for k in KINDS] + list(HEAD_CASES))
def test_reference_forward_meets_the_fp64_oracle(kind, heads):
    """hidden state, both logits and predict()'s candidate logits of tests/golden/<kind>.npz (read by test_oracle_golden.py at
    2e-6 absolute against the fp32 oracle) under the metric and bound the kernels are held to"""
    g, sd, batch = load_golden(kind, heads)
    cfg = golden_cfg(kind, heads=heads)
    cand = torch.from_numpy(g["cands"])

    def run(w):
        h, pl, nl = O.forward(cfg, w, *batch)
        return {"hidden": h, "pos_logits": pl, "neg_logits": nl, "pred_logits": O.predict(cfg, w, batch[0], batch[1], cand)}
    with torch.no_grad():
        x64, x32 = run({k: v.double() for k, v in sd.items()}), G._one_thread(lambda: run(sd))
    _anchor({k: g[k] for k in x64}, x64, x32)


DROP_ANCHORS = [c[0] for c in DROP_CASES if c[3] <= 64 and c[2] <= 50]


@pytest.mark.parametrize("name", DROP_ANCHORS)
def test_reference_train_forward_meets_the_fp64_oracle(name):
    """the train-mode fixtures (the reference's classes under the project's keep masks, step 1's seed; make_golden.py --dropout
    runs them in fp64 and stores fp32): the fp64 oracle with the promoted fp32 keep masks is the reference's dropout forward to
    storage rounding where p = 0.5.  At p = 0.3 the reference scales by the double 1 / 0.7 and the oracle, as the kernels, by
    float32(1 / 0.7) - 2.4e-8 apart at each of seven sites (measured: 1.3e-7): held like a device output there."""
    g, sd, batch, cfg = load_drop(name)
    seed = O.step_seed(int(g["seed"]), 1)

    def run(w):
        h, pl, nl = O.forward(cfg, w, *batch, train=True, seed=seed, b0=0)
        out = {"hidden": h} if "hidden" in g else {"h_last": h[:, -1]}
        return dict(out, pos_logits=pl, neg_logits=nl)
    with torch.no_grad():
        x64, x32 = run({k: v.double() for k, v in sd.items()}), G._one_thread(lambda: run(sd))
    _anchor({k: g[k] for k in x64}, x64, x32, storage=cfg.dropout == 0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------
SHARP_CASES = ("t0", "t2", "k")      # default geometry (SASRec); SRFRN at the default geometry; SRFRN at seq_len 203
SCALED_TO = 6e-5                     # a wrong forward that misses the old bar on a case is scaled down to this, not dropped
OUT = R.OUTPUTS["eval"]


def _run32(ref, sd):
    with torch.no_grad():
        return G._one_thread(lambda: dict(zip(OUT, O.forward(ref.cfg, sd, *ref.batch))))


def _wrong_forwards(ref):
    """(name, {output: tensor}): the fp32 oracle with one thing wrong - what a kernel with that error would hand back"""
    sd = ref.sd
    saved = O.LN_EPS
    try:
        O.LN_EPS = 1e-5                                  # a thousand times the reference's
        x = _run32(ref, sd)
    finally:
        O.LN_EPS = saved
    yield "LN_EPS = 1e-5", x
    k = "attention_layers.0.out_proj.bias"
    yield "block 0 out_proj.bias scaled by 1 + 2e-4", _run32(ref, dict(sd, **{k: sd[k] * (1 + 2e-4)}))
    k = O.key_pos(ref.cfg)
    w = sd[k].clone()
    t = 7 if bool((ref.batch[0][:, 7] != 0).any()) else ref.cfg.max_len - 8      # (a row some sequence reads)
    w[t] *= 1 + 1e-4
    yield f"positional row {t} scaled by 1 + 1e-4", _run32(ref, dict(sd, **{k: w}))
    x = {o: t.clone() for o, t in ref.x32.items()}
    x["hidden"][1, -1, 7] += 3e-5
    x["pos_logits"][2, -1] += 3e-5
    yield "one hidden element and one logit off by 3e-5", x


@pytest.mark.parametrize("cid", SHARP_CASES)
def test_metric_rejects_what_the_old_bar_accepts(cid):
    """Every wrong forward is 2.9e-5 .. 9.8e-5 from the fp32 oracle (under the old bar) and 1.4 .. 7.5 times over the bound on
    its worst output, on both kinds of machine; the narrowest are the single element on case k (hidden 1.41) and LN_EPS on t0
    (hidden 1.70).  On t2 LN_EPS (1.4e-4) and the positional row (2.9e-4) miss the old bar and run scaled to 6e-5."""
    ref = R.reference(cid, "eval")
    assert O.LN_EPS == 1e-8
    seen = 0
    for name, x in _wrong_forwards(ref):
        old = max(float((x[o] - ref.x32[o]).abs().max()) for o in OUT)
        assert old > 0, name
        if not old < R.OLD_BAR:
            x = {o: ref.x32[o] + (x[o] - ref.x32[o]) * (SCALED_TO / old) for o in OUT}
            name += f" (scaled from {old:.1e} to {SCALED_TO:.0e})"
            old = max(float((x[o] - ref.x32[o]).abs().max()) for o in OUT)
        figs = R.compare(x, ref)
        ratio = {o: figs[o]["err"] / figs[o]["bound"] for o in OUT}
        print(f"case {cid}: {name}: old metric {old:.2e}; error / bound " + ", ".join(f"{o} {r:.2f}" for o, r in ratio.items()))
        assert old < R.OLD_BAR, name                                     # the old bar accepts it ...
        assert any(not R.holds(f) for f in figs.values()), name          # ... and the fp64 bound does not
        seen += 1
    assert seen >= 4 and O.LN_EPS == 1e-8


@pytest.mark.parametrize("junk", [0.0, float("nan")], ids=["zeros", "nan-sentinel"])
def test_metric_is_not_fooled_by_a_pad_row(junk):
    """a hidden state whose padded positions were left unwritten (zeros, or the NaN sentinel of a pre-filled buffer) fails -
    every row counts, and the oracle's pad row is the last LayerNorm's bias"""
    for cid in ("t0", "k"):
        ref = R.reference(cid, "eval")
        seq = ref.batch[0]
        b, t = (int(i[0]) for i in torch.where(seq == 0))
        assert torch.equal(ref.x64["hidden"][b, t], ref.sd["last_layernorm.bias"].double())
        x = {o: v.clone() for o, v in ref.x32.items()}
        assert all(R.holds(f) for f in R.compare(x, ref).values())
        x["hidden"][b, t] = junk                                         # ONE pad row of B L
        fig = R.compare(x, ref)["hidden"]
        assert not R.holds(fig) and fig["err"] > 0.5, fig
        x = {o: v.clone() for o, v in ref.x32.items()}
        x["hidden"][seq == 0] = junk                                     # all of them
        assert not R.holds(R.compare(x, ref)["hidden"])
