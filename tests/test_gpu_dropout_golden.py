"""-m gpu: train mode (dropout p > 0) against the reference - fixtures made from the reference's own classes with the
project's coordinate-hash keep masks in place of torch's dropout (tests/golden/make_golden.py --dropout, tests.helpers
DROP_CASES; tests/test_oracle_dropout_golden.py pins the oracle to the same fixtures).  The cases reach the instantiations
that run only with dropout on:

  * seq_len 20: the <50, 32, 8> specialised kernels (SASRec, SRFRN's [item | fake] targets, SRFU_B's label channel) and,
    with two heads, the generic instantiation with one mask per head;
  * seq_len 50: the ragged pair, variants 0-3 (SASRec, SRFR, SRFRN, SRFU_B), train = 1 through FusedTrainer and train = 0
    with masks through the module path; batch 512 is C2's launch shape; p = 0.3: a non-power-of-two scale and threshold;
  * seq_len 100, batch 300 (above one round of CUs): the 16-wave training forward and the slot-placed backward's c4 form;
  * seq_len 200: the row-owner forward and the row-chunked backward (SASRec, and SRFRN's 45 + 5).

Per case: (a) three graph-replayed FusedTrainer(seed=S) steps - the per-step seed advances inside the captured graph -
against the reference's loss curve and weights after steps 1 and 3; (b) the module forward in .train() with step 1's
seed, the reference's BCE loss and loss.backward(): outputs, loss, every gradient; (c) the same through the registered
torch.ops.srfrd.encoder_fwd and its backward (library_ops).  Tolerances: 1e-4 absolute for outputs, losses, gradients and
step-1 weights, 2e-4 for step-3 weights; at seq_len >= 50 the weights are held element-wise to tests/helpers.adam_tolerance
(Adam turns a gradient at rounding-noise level into a +-lr step of either sign), as the C4 tests do."""
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.helpers import DROP_NAMES, assert_post_adam, drop_case, drop_kbias, load_drop, oracle_step_with_grads, sub

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _loss(pl, nl, pos):
    idx = torch.where(pos != 0)
    crit = torch.nn.BCEWithLogitsLoss()
    return crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])


@pytest.mark.parametrize("name", DROP_NAMES)
def test_fused_trainer_graph_steps_match_reference(name):
    import srfrd_amd
    from tests.gpu_util import build_model, cuda, maxerr
    g, sd, batch, cfg = load_drop(name)
    B, L = batch[0].shape
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}).train()
    tr = srfrd_amd.FusedTrainer(model, B, L, lr=1e-3, betas=(0.9, 0.98), seed=int(g["seed"]), use_graph=True)
    ids = cuda(*batch)
    w1, w3 = sub(g, "w1/"), sub(g, "w3/")
    msd1 = None
    for step in range(3):
        loss = tr.step(None, *ids)
        assert abs(float(loss.cpu()) - float(g[f"loss{step}"])) < TOL, step
        if step == 0:
            msd1 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert tr.graph_form == "one" and tr.captured, tr.graph_capture_error
    msd3 = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if L == 20:
        for k in w1:
            assert maxerr(drop_kbias(k, msd1[k], cfg.D), drop_kbias(k, w1[k], cfg.D)) < TOL, k
        for k in w3:
            assert maxerr(drop_kbias(k, msd3[k], cfg.D), drop_kbias(k, w3[k], cfg.D)) < 2e-4, k
        return
    # element-wise Adam bound from the gradients of the three steps (the float64 oracle, pinned to the reference by
    # tests/test_oracle_dropout_golden.py); the K slice of in_proj_bias excluded (drop_kbias)
    sd64 = {k: v.double() for k, v in sd.items()}
    opt = O.Adam(sd64)
    hist = [{k: v.float() for k, v in oracle_step_with_grads(cfg, sd64, opt, batch, train=True,
                                                            seed=O.step_seed(int(g["seed"]), t + 1), b0=0)[1].items()}
            for t in range(3)]
    # (seq_len >= 100: millions of ReLU units per step - a unit at its threshold may flip, as in tests/test_gpu_c4_c5.py)
    outliers = 2e-3 if L >= 100 else 0.0
    assert_post_adam(msd1, w1, hist[:1], cfg.D, outliers=outliers)
    assert_post_adam(msd3, w3, hist, cfg.D, outliers=outliers)


def _module_case(name, library_ops):
    from tests.gpu_util import build_model, cuda, maxerr
    g, sd, batch, cfg = load_drop(name)
    model = build_model(cfg, sd).train()
    model.library_ops = library_ops
    seed1 = O.step_seed(int(g["seed"]), 1)
    model._next_seed = lambda: seed1
    seq, rsq, pos, prs, neg, nrs = cuda(*batch)
    h, pl, nl = model(None, seq, rsq, pos, prs, neg, nrs)
    if "hidden" in g:
        assert maxerr(h, torch.from_numpy(g["hidden"])) < TOL
    else:
        assert maxerr(h[:, -1], torch.from_numpy(g["h_last"])) < TOL
    assert maxerr(pl, torch.from_numpy(g["pos_logits"])) < TOL
    assert maxerr(nl, torch.from_numpy(g["neg_logits"])) < TOL
    loss = _loss(pl, nl, pos)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss0"])) < TOL
    gg = sub(g, "g/")
    errs = {k: maxerr(p.grad, gg[k]) for k, p in model.named_parameters()}
    assert set(errs) == set(gg)
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", DROP_NAMES)
def test_module_train_forward_backward_match_reference(name):
    _module_case(name, library_ops=False)


@pytest.mark.parametrize("name", DROP_NAMES)
def test_library_ops_train_forward_backward_match_reference(name):
    _module_case(name, library_ops=True)
