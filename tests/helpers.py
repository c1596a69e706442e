"""Shared test helpers: golden-fixture loading and oracle configuration."""
import hashlib
import math
import os

import numpy as np
import torch

from oracle import srfrd_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = O.KINDS
G_I, G_L, G_B = 1000, 20, 8


HEAD_CASES = (("SASRec", 2), ("SRFRN", 5), ("SRFU_B", 2))      # tests/golden/<kind>_h<heads>.npz (make_golden.py --heads)


def golden_cfg(kind, dropout=0.0, heads=1):
    if kind == "SASRec":
        return O.Cfg(kind, G_I, G_L, 50, dropout=dropout, num_heads=heads)
    if kind in ("SRFR", "SRFRN"):
        return O.Cfg(kind, G_I, G_L, 45, d_fake=5, dropout=dropout, num_heads=heads)
    nl = {"SRFU_B": 3, "SRFU_F": G_L + 1, "SRFU_R": 11}[kind]
    return O.Cfg(kind, G_I, G_L, 50, n_labels=nl, dropout=dropout, num_heads=heads)


def load_golden(kind, heads=1, l2=False):
    z = np.load(os.path.join(GOLDEN, f"{kind}_l2.npz" if l2 else (f"{kind}.npz" if heads == 1 else f"{kind}_h{heads}.npz")))
    g = {k: z[k] for k in z.files}
    sd = {k[2:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("w/")}
    batch = tuple(torch.from_numpy(g[k]) for k in ("seq", "rsq", "pos", "prs", "neg", "nrs"))
    return g, sd, batch


# Train-mode (dropout > 0) fixtures tests/golden/<name>.npz (make_golden.py --dropout): the reference's own classes in
# .train() with torch.nn.functional.dropout replaced by the project's coordinate-hash keep masks.
# (name, class, seq_len, batch, items, num_heads, p).  seq_len 20: the inputs and initial weights are those of the
# dropout-free fixture <class>.npz / <class>_h<heads>.npz (not stored twice).
DROP_CASES = (
    ("drop_SASRec_L20", "SASRec", 20, 8, 1000, 1, 0.5),
    ("drop_SRFRN_L20", "SRFRN", 20, 8, 1000, 1, 0.5),
    ("drop_SRFU_B_L20", "SRFU_B", 20, 8, 1000, 1, 0.5),
    ("drop_SASRec_L20_h2", "SASRec", 20, 8, 1000, 2, 0.5),
    ("drop_SASRec_L50", "SASRec", 50, 512, 400, 1, 0.5),
    ("drop_SRFR_L50", "SRFR", 50, 64, 400, 1, 0.5),
    ("drop_SRFRN_L50", "SRFRN", 50, 64, 400, 1, 0.5),
    ("drop_SRFU_B_L50", "SRFU_B", 50, 64, 400, 1, 0.5),
    ("drop_SASRec_L50_p03", "SASRec", 50, 64, 400, 1, 0.3),
    ("drop_SASRec_L100", "SASRec", 100, 300, 400, 1, 0.5),
    ("drop_SASRec_L200", "SASRec", 200, 64, 400, 1, 0.5),
    ("drop_SRFRN_L200", "SRFRN", 200, 64, 400, 1, 0.5),
)
DROP_NAMES = tuple(c[0] for c in DROP_CASES)


def drop_case(name):
    return next(c for c in DROP_CASES if c[0] == name)


def drop_cfg(name):
    _, kind, L, _, I, heads, p = drop_case(name)
    if kind == "SASRec":
        return O.Cfg(kind, I, L, 50, dropout=p, num_heads=heads)
    if kind in ("SRFR", "SRFRN"):
        return O.Cfg(kind, I, L, 45, d_fake=5, dropout=p, num_heads=heads)
    nl = {"SRFU_B": 3, "SRFU_F": L + 1, "SRFU_R": 11}[kind]
    return O.Cfg(kind, I, L, 50, n_labels=nl, dropout=p, num_heads=heads)


def drop_init_weights(seed, shapes):
    """Initial weights of the seq_len >= 50 DROP_CASES fixtures, regenerated from the fixture's ``init_seed`` rather than
    stored.  shapes: {state_dict name: shape}; one numpy RandomState draws the tensors in sorted-name order:
    xavier_normal_'s standard deviation for >= 2-D tensors, 1 + 0.05 N(0, 1) for LayerNorm weights, 0.05 N(0, 1) for the
    other 1-D tensors."""
    rs = np.random.RandomState(seed)
    out = {}
    for k in sorted(shapes):
        shp = tuple(int(n) for n in shapes[k])
        z = rs.standard_normal(shp)
        if len(shp) >= 2:
            rf = int(np.prod(shp[2:]))
            a = z * math.sqrt(2.0 / (shp[1] * rf + shp[0] * rf))
        elif "layernorm" in k and k.endswith("weight"):
            a = 1.0 + 0.05 * z
        else:
            a = 0.05 * z
        out[k] = torch.from_numpy(a.astype(np.float32))
    return out


def weights_sha256(sd):
    """SHA-256 (uint8 (32,)) of a state_dict's float32 bytes in sorted-name order"""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(np.ascontiguousarray(sd[k].numpy() if hasattr(sd[k], "numpy") else sd[k], np.float32).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def load_drop(name):
    """-> (fixture dict, initial state_dict, batch (6 x int64 (B, L)), oracle Cfg) of one DROP_CASES fixture.
    The weights after steps 1 and 3 are stored as the XOR of their float32 bit patterns with the previous weights'
    (``x1/``, ``x3/``); they are returned decoded as ``w1/`` and ``w3/`` entries of the fixture dict."""
    _, kind, L, B, _, heads, p = drop_case(name)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    assert float(g["p"]) == p
    if L == G_L:
        _, sd, batch = load_golden(kind, heads)
    else:
        sd = drop_init_weights(int(g["init_seed"]), {k[2:]: v.shape for k, v in g.items() if k.startswith("g/")})
        batch = tuple(torch.from_numpy(g[k].astype(np.int64)) for k in ("seq", "rsq", "pos", "prs", "neg", "nrs"))
    assert (weights_sha256(sd) == g["w_sha256"]).all(), "initial weights differ from the generator's"
    assert batch[0].shape == (B, L)
    prev = {k: v.numpy() for k, v in sd.items()}
    for s in (1, 3):
        for k in prev:
            prev[k] = (prev[k].view(np.int32) ^ g[f"x{s}/" + k]).view(np.float32)
            g[f"w{s}/" + k] = prev[k]
    return g, sd, batch, drop_cfg(name)


def sub(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


def drop_kbias(name, a, D):
    """Post-Adam weights are compared with the K slice of ``in_proj_bias`` removed.

    The key bias adds the same q.b_k to every score of a softmax row, so its true gradient is
    identically 0 and the outputs do not depend on it; what autograd returns is rounding noise
    (~1e-9) whose SIGN Adam's g/sqrt(v) normalisation turns into a +-O(lr) update.  No two
    summation orders (the reference on CPU vs on a GPU, or the oracle) agree on it.
    """
    a = a.clone() if hasattr(a, "clone") else a.copy()
    if name.endswith("in_proj_bias"):
        a[D:2 * D] = 0
    return a


def oracle_step_with_grads(cfg, sd, opt, batch, **kw):
    """O.train_step that also hands back the gradients it stepped with (for adam_tolerance)."""
    loss, grads, *_ = O.grads_of(cfg, sd, batch, **kw)
    opt.step(sd, grads)
    return loss, grads


def adam_tolerance(grad_hist, lr=1e-3, noise=5e-6, base=1e-5):
    """Element-wise bound on |w_gpu - w_oracle| after len(grad_hist) Adam steps.

    Adam moves an element by lr * m_hat / (sqrt(v_hat) + eps): the MAGNITUDE of the gradient cancels, so an absolute
    gradient error d on an element whose gradient is g changes the step by about lr * d / |g| - nothing for a real
    gradient, a full +-lr when |g| is itself rounding noise (the sign is then noise).  With `noise` the absolute
    gradient agreement the gradient tests establish (observed ~1e-6; tests/test_gpu_grad_fp64.py holds every gradient, the
    fused step's included, to the fp64 oracle within 2e-5 .. 1e-4 of its own row's norm - the stepped weights compared here
    cannot see a gradient's scale, those tests do) the bound per element is
        base + steps * lr * min(1, 4 * noise / min_t |g_t|):
    1e-4 or tighter wherever every step's |gradient| exceeds ~5e-4 (at two steps), relaxing continuously to steps * lr
    only for elements whose gradient is at noise level.  A blanket `max < steps * lr` would also pass a real 1e-3
    error on an element with a real gradient; this does not.
    """
    steps = len(grad_hist)
    gabs = torch.stack([g.detach().abs().double() for g in grad_hist])
    gmin = gabs.min(0).values
    tol = base + steps * lr * torch.clamp(4.0 * noise / gmin.clamp_min(1e-300), max=1.0)
    # an element whose gradient is EXACTLY zero at every step (an item row no sequence touched) must not move at all
    return torch.where(gabs.max(0).values == 0, torch.full_like(tol, 1e-7), tol)


def assert_post_adam(msd, sd, grad_hists, D, lr=1e-3, noise=5e-6, outliers=0.0):
    """every parameter of `msd` (GPU) within adam_tolerance of `sd` (oracle); grad_hists = list (per step) of {name: grad}.
    Returns the fraction of elements that were held to 1e-4 or tighter.

    `outliers` (default 0: none): the fraction of a tensor's elements allowed outside the bound (each still within
    2 * steps * lr: opposite Adam steps).  For tests with millions of ReLU units per step only: fp32 training through ReLU is discontinuous - a
    unit whose pre-activation is within rounding of zero takes derivative 1 in one implementation and 0 in the other, and
    the gradient of THAT token (its item rows, a few per cent of them) differs while every forward output agrees to 1e-7.
    At 300 x 144 x 50 x 2 units about one such unit per step is expected (tests/diag_grad.py shows it: identical "error"
    from two independent backward kernels, gone with another batch seed).  A wrong kernel moves whole tensors, not a
    handful of elements of one item row."""
    tight = total = 0
    for k in sd:
        a, b = drop_kbias(k, msd[k].detach().cpu(), D), drop_kbias(k, sd[k], D)
        tol = adam_tolerance([drop_kbias(k, gh[k], D) if k.endswith("in_proj_bias") else gh[k] for gh in grad_hists], lr, noise)
        if k.endswith("in_proj_bias"):
            tol[D:2 * D] = 1.0          # (K-bias slice: excluded, see drop_kbias)
        d = (a.double() - b.double()).abs()
        bad = d > tol
        if outliers > 0.0 and bool(bad.any()):
            assert int(bad.sum()) <= max(1, int(outliers * bad.numel())) and float(d.max()) <= 2 * len(grad_hists) * lr * 1.1 + 1e-5, \
                (k, float(d[bad].max()), int(bad.sum()), bad.numel())
            bad = torch.zeros_like(bad)
        assert not bool(bad.any()), (k, float(d[bad].max()), float(tol[bad].min()), int(bad.sum()))
        tight += int((tol <= 1e-4).sum())
        total += tol.numel()
    return tight / max(total, 1)
