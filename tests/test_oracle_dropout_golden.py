"""The CPU oracle in train mode (dropout p > 0) against fixtures generated from the reference's own classes with the
project's coordinate-hash keep masks in place of torch's dropout (tests/golden/make_golden.py --dropout, tests.helpers
DROP_CASES).  The mask values are the project's; which tensor each mask multiplies, its layout, its 1 / (1 - p) scale and
everything downstream - forward, backward, three Adam steps - are the reference's."""
import hashlib

import numpy as np
import pytest

from oracle import srfrd_oracle as O
from tests.helpers import DROP_NAMES, drop_kbias, load_drop, sub

TOL = 2e-6           # tests/test_oracle_golden.py's tolerances
W1_TOL, W3_TOL = 2e-5, 1e-4


def _load64(name):
    """the fixture with the initial weights in float64: the reference ran in float64 (make_golden.py --dropout), so does
    the oracle here - both sides are free of float32 summation-order noise and agree to the fixture's float32 storage"""
    g, sd, batch, cfg = load_drop(name)
    return g, {k: v.double() for k, v in sd.items()}, batch, cfg


def _step_seed(g, t):
    return O.step_seed(int(g["seed"]), t)


@pytest.mark.parametrize("name", DROP_NAMES)
def test_mask_digests_reproduce(name):
    """every (step, site) keep mask of the fixture, rebuilt from O.keep_mask: a failure here means the hash changed
    (regenerate the fixtures on purpose), not that a mask is misplaced"""
    g, _, batch, cfg = load_drop(name)
    B, L = batch[0].shape
    p, b0 = float(g["p"]), int(g["b0"])
    assert b0 == 0
    site_cols = [(O.SITE_EMB, cfg.D)] if cfg.kind == "SASRec" else []         # (site, mask columns) in call order
    for i in range(cfg.num_blocks):
        site_cols += [(O.site_attn(i, h), L) for h in range(cfg.num_heads)] + [(O.site_ffn1(i), cfg.D), (O.site_ffn2(i), cfg.D)]
    assert [int(s) for s in g["mask_sites"]] == [s for s, _ in site_cols]
    for t in range(3):
        seed = _step_seed(g, t + 1)
        for j, (site, cols) in enumerate(site_cols):
            keep = (O.keep_mask(seed, site, b0, B, L, cols, p) > 0).numpy()
            assert int(keep.sum()) == int(g["mask_kept"][t, j]), (t, site)
            sha = np.frombuffer(hashlib.sha256(np.packbits(keep.ravel()).tobytes()).digest(), np.uint8)
            assert (sha == g["mask_sha256"][t, j]).all(), (t, site)


@pytest.mark.parametrize("name", DROP_NAMES)
def test_train_forward_matches_reference(name):
    g, sd, batch, cfg = _load64(name)
    h, pl, nl = O.forward(cfg, sd, *batch, train=True, seed=_step_seed(g, 1), b0=int(g["b0"]))
    if "hidden" in g:
        assert h.shape == g["hidden"].shape
        np.testing.assert_allclose(h.numpy(), g["hidden"], atol=TOL, rtol=0)
    else:
        np.testing.assert_allclose(h[:, -1].numpy(), g["h_last"], atol=TOL, rtol=0)
    np.testing.assert_allclose(pl.numpy(), g["pos_logits"], atol=TOL, rtol=0)
    np.testing.assert_allclose(nl.numpy(), g["neg_logits"], atol=TOL, rtol=0)


@pytest.mark.parametrize("name", DROP_NAMES)
def test_train_grads_match_reference(name):
    g, sd, batch, cfg = _load64(name)
    loss, grads, *_ = O.grads_of(cfg, sd, batch, train=True, seed=_step_seed(g, 1), b0=int(g["b0"]))
    assert abs(float(loss) - float(g["loss0"])) < TOL
    gg = sub(g, "g/")
    assert set(gg) == set(grads)
    for k in gg:
        np.testing.assert_allclose(grads[k].numpy(), gg[k].numpy(), atol=TOL, rtol=0, err_msg=k)


@pytest.mark.parametrize("name", DROP_NAMES)
def test_train_steps_match_reference(name):
    """three Adam steps, each with its own step seed: loss curve, weights after steps 1 and 3"""
    g, sd, batch, cfg = _load64(name)
    opt = O.Adam(sd)
    w1, w3 = sub(g, "w1/"), sub(g, "w3/")
    for step in range(3):
        loss = O.train_step(cfg, sd, opt, batch, train=True, seed=_step_seed(g, step + 1), b0=int(g["b0"]))
        assert abs(float(loss) - float(g[f"loss{step}"])) < 5e-6, step
        if step == 0:
            for k in w1:
                np.testing.assert_allclose(drop_kbias(k, sd[k], cfg.D).numpy(), drop_kbias(k, w1[k], cfg.D).numpy(),
                                           atol=W1_TOL, rtol=0, err_msg=k)
    for k in w3:
        np.testing.assert_allclose(drop_kbias(k, sd[k], cfg.D).numpy(), drop_kbias(k, w3[k], cfg.D).numpy(),
                                   atol=W3_TOL, rtol=0, err_msg=k)
