"""BASELINE configs[1] / [2] at FULL size against the REFERENCE's own outputs (tests/golden/c2_reference_outputs.npz,
written by ``make_golden.py --c2`` in the build container: the reference classes at 50 000 items, seq_len 50, batch 512).

The weights (10 MB per kind) are not stored: under the same ``torch.manual_seed`` the drop-in classes create their
parameter containers in the reference's construction order, so the trainer's ``xavier_normal_`` loop (reference
trainer.py:364-369) yields the reference's weights bit for bit - checked through stored per-tensor checksums on CPU - and
the -m gpu test compares the HIP forward with the reference's full pos / neg logits and last-position hidden states."""
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import GOLDEN

KINDS = ("SASRec", "SRFRN", "SRFU_B")


def _fixture():
    z = np.load(os.path.join(GOLDEN, "c2_reference_outputs.npz"))
    return {k: z[k] for k in z.files}


def _exact_sum(t):
    """the correctly rounded float64 sum, the same on every host (torch's parallel sum() depends on the thread count)"""
    return math.fsum(t.double().flatten().tolist())


def _build(kind, g, device):
    import srfrd_amd
    I, L, B = (int(x) for x in g["meta"])
    seed, data_seed = (int(x) for x in g[f"{kind}/seed"])
    torch.manual_seed(seed)
    if kind == "SASRec":
        m = srfrd_amd.SASRec(I, L, 50, 0.5, 2, 1, device)
    elif kind == "SRFRN":
        m = srfrd_amd.SRFRN(I, L, 45, 5, 0.5, 2, 1, device)
    else:
        m = srfrd_amd.SRFU_B(I, L, 50, 3, 0.5, 2, 1, device)
    for _, p in m.named_parameters():          # reference trainer.py:364-369
        try:
            torch.nn.init.xavier_normal_(p.data)
        except Exception:
            pass
    batch = srfrd_amd.synthetic_batch(I, L, B, seed=data_seed)
    return m, batch


@pytest.mark.parametrize("kind", KINDS)
def test_same_seed_reproduces_the_reference_weights(kind):
    g = _fixture()
    m, _ = _build(kind, g, "cpu")
    sd = m.state_dict()
    assert len(sd) == len(g[f"{kind}/w_sum"])
    for j, v in enumerate(sd.values()):
        assert _exact_sum(v) == g[f"{kind}/w_sum"][j] and _exact_sum(v.abs()) == g[f"{kind}/w_abs"][j], j


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_full_size_forward_matches_the_reference(kind):
    g = _fixture()
    m, batch = _build(kind, g, "cuda")
    m = m.cuda().eval()
    u, seq, rsq, pos, prs, neg, nrs = (t.cuda() for t in batch)
    with torch.no_grad():
        h, pl, nl = m(u, seq, rsq, pos, prs, neg, nrs)
    assert float((pl.cpu() - torch.from_numpy(g[f"{kind}/pos_logits"])).abs().max()) < 1e-4
    assert float((nl.cpu() - torch.from_numpy(g[f"{kind}/neg_logits"])).abs().max()) < 1e-4
    assert float((h[:, -1].cpu() - torch.from_numpy(g[f"{kind}/h_last"])).abs().max()) < 1e-4
    hs = h.double()
    # whole-tensor checksums over 1.28 M elements (each within ~1e-6 of the reference's): sum to 0.05, sum of squares to 1e-5 relative
    assert abs(float(hs.sum()) - g[f"{kind}/h_sum"][0]) < 0.05
    assert abs(float((hs ** 2).sum()) - g[f"{kind}/h_sum"][1]) < 1e-5 * g[f"{kind}/h_sum"][1]
