#!/usr/bin/env python3
"""Generate golden fixtures from the REFERENCE's own classes (run in the build container only).

    SRFRD_REFERENCE=<reference checkout> python -B tests/golden/make_golden.py      # writes tests/golden/*.npz

Imports ``$SRFRD_REFERENCE/SRFR_model.py`` (torch + numpy only), applies the trainer's
xavier_normal_ init (reference trainer.py:364-369) under a fixed seed, and records, per class:
inputs, the full state_dict, eval-mode ``forward`` outputs, ``predict`` logits, and - with
``dropout_rate=0`` - the restated train step of reference trainer.py:31-41: loss, every parameter
gradient, and weights after 1 and 3 ``torch.optim.Adam(lr=1e-3, betas=(0.9, 0.98))`` steps.
Only inputs/outputs are stored; no reference source text is copied.  The reference does not exist
on the GPU box, so nothing at test time imports it.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REFERENCE = os.environ.get("SRFRD_REFERENCE")     # a checkout of github.com/oss0430/SRFRD
if not REFERENCE:
    sys.exit("set SRFRD_REFERENCE to a checkout of the reference (github.com/oss0430/SRFRD)")
sys.path.insert(0, REFERENCE)
import SRFR_model as ref  # noqa: E402

I, L, B = 1000, 20, 8            # C1's catalog (BASELINE configs[0]: 1k items, seq_len 20)
D_ITEM, D_FAKE, NB, NH = 45, 5, 2, 1


def make_inputs(seed, I=I, L=L, B=B):
    g = np.random.RandomState(seed)
    seq = np.zeros((B, L), np.int64)
    rsq = np.zeros((B, L), np.int64)
    pos = np.zeros((B, L), np.int64)
    prs = np.zeros((B, L), np.int64)
    neg = np.zeros((B, L), np.int64)
    nrs = np.zeros((B, L), np.int64)
    lens = g.randint(2, L + 1, size=B)
    lens[0] = L            # one full sequence
    lens[1] = 1            # one very short sequence
    for b in range(B):
        n = int(lens[b])
        items = g.randint(1, I + 1, size=n + 1)
        revs = g.choice([1, 2], size=n + 1, p=[0.3, 0.7])
        if b == 2:          # fake/real tie (even count) for the label rounding edge
            n2 = (n // 2) * 2
            revs[:n2] = np.tile([1, 2], n2 // 2)
        if b == 3:
            revs[:] = 1     # all fake
        seq[b, L - n:] = items[:n]
        rsq[b, L - n:] = revs[:n]
        pos[b, L - n:] = items[1:n + 1]
        prs[b, L - n:] = revs[1:n + 1]
        neg[b, L - n:] = g.randint(1, I + 1, size=n)
        nrs[b, L - n:] = 1
    return seq, rsq, pos, prs, neg, nrs


def build(kind, dropout, nh=NH):
    if kind == "SASRec":
        return ref.SASRec(I, L, D_ITEM + D_FAKE, dropout, NB, nh, "cpu")
    if kind == "SRFR":
        return ref.SRFR(I, L, D_ITEM, D_FAKE, dropout, NB, nh, "cpu")
    if kind == "SRFRN":
        return ref.SRFRN(I, L, D_ITEM, D_FAKE, dropout, NB, nh, "cpu")
    nl = {"SRFU_B": 3, "SRFU_F": L + 1, "SRFU_R": 11}[kind]
    return getattr(ref, kind)(I, L, D_ITEM + D_FAKE, nl, dropout, NB, nh, "cpu")


def trainer_init(model):
    for _, p in model.named_parameters():          # reference trainer.py:364-369
        try:
            torch.nn.init.xavier_normal_(p.data)
        except Exception:
            pass
    # 1-D params keep defaults (zeros/ones): perturb them too so that bias/LN paths are pinned
    # (a fixture-only choice; still the reference's forward on these weights)
    g = torch.Generator().manual_seed(99)
    for _, p in model.named_parameters():
        if p.dim() == 1:
            p.data.add_(0.05 * torch.randn(p.shape, generator=g))


def t64(a):
    return torch.from_numpy(a)


HEAD_CASES = (("SASRec", 2), ("SRFRN", 5), ("SRFU_B", 2))      # num_heads > 1: <kind>_h<heads>.npz (--heads)


L2_CASES = (("SRFRN", 1),)      # l2_emb = 0.05 (reference trainer.py:39 with a non-zero config.l2_emb): <kind>_l2.npz (--l2)


def main(cases=None, l2_emb=0.0):
    torch.set_num_threads(1)
    all_kinds = ["SASRec", "SRFR", "SRFRN", "SRFU_B", "SRFU_F", "SRFU_R"]
    for kind, nh in (cases or [(k, NH) for k in all_kinds]):
        k_i = all_kinds.index(kind)
        torch.manual_seed(1234 + k_i + 100 * (nh - 1) + (7 if l2_emb else 0))
        model = build(kind, 0.0, nh)
        trainer_init(model)
        seq, rsq, pos, prs, neg, nrs = make_inputs(7 + k_i)
        out = {"seq": seq, "rsq": rsq, "pos": pos, "prs": prs, "neg": neg, "nrs": nrs}
        sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in sd0.items():
            out["w/" + k] = v.numpy()
        model.eval()
        u = torch.zeros(B, dtype=torch.int64)
        h, pl, nl = model(u, t64(seq), t64(rsq), t64(pos), t64(prs), t64(neg), t64(nrs))
        out["hidden"], out["pos_logits"], out["neg_logits"] = h.detach().numpy(), pl.detach().numpy(), nl.detach().numpy()
        # predict: one user at a time over 101 candidates (reference utils.py:576-589)
        g = np.random.RandomState(5)
        cands = g.randint(1, I + 1, size=(B, 101)).astype(np.int64)
        pred = np.stack([model.predict(u[b:b + 1], t64(seq[b:b + 1]), t64(rsq[b:b + 1]), t64(cands[b])).detach().numpy()
                         for b in range(B)])
        out["cands"], out["pred_logits"] = cands, pred
        if kind.startswith("SRFU"):
            out["labels"] = model.get_Labels(t64(rsq)).numpy().astype(np.int64)
        # train step restated from reference trainer.py:31-41 (model.train(), dropout_rate = 0)
        model.train()
        crit = torch.nn.BCEWithLogitsLoss()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.98))
        for step in range(3):
            h, pl, nl = model(user_ids=u, input_ids=t64(seq), fake_ids=t64(rsq), positive_ids=t64(pos),
                              positive_fake_ids=t64(prs), negative_ids=t64(neg), negative_fake_ids=t64(nrs))
            opt.zero_grad()
            idx = torch.where(t64(pos) != 0)
            loss = crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])
            for p in model.parameters():
                loss = loss + l2_emb * torch.norm(p)
            loss.backward()
            if step == 0:
                out["loss0"] = np.float32(loss.item())
                for k, p in model.named_parameters():
                    out["g/" + k] = p.grad.detach().numpy().copy()
            opt.step()
            if step in (0, 2):
                for k, v in model.state_dict().items():
                    out[f"w{step + 1}/" + k] = v.detach().numpy().copy()
            out[f"loss{step}"] = np.float32(loss.item())
        path = os.path.join(HERE, f"{kind}_l2.npz" if l2_emb else (f"{kind}.npz" if nh == 1 else f"{kind}_h{nh}.npz"))
        out["l2_emb"] = np.float64(l2_emb)
        np.savez_compressed(path, **out)
        print(kind, "->", path, os.path.getsize(path) // 1024, "KiB")
    if cases:
        return

    # get_Labels edge-case matrix (integer, bit-exact): ties, all-pad, all-fake, all-real
    edge = np.array([[0] * 10, [1] * 10, [2] * 10, [1, 2] * 5, [0, 0, 0, 0, 1, 1, 1, 2, 2, 2],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0, 2], [0, 0, 1, 2, 2, 2, 2, 2, 2, 2],
                     [1, 1, 1, 1, 1, 1, 1, 2, 2, 2], [0, 1, 1, 1, 1, 1, 1, 1, 1, 2]], np.int64)
    lab = {"fake_ids": edge}
    for kind, nl in (("SRFU_B", 3), ("SRFU_F", 11), ("SRFU_R", 11)):
        m = getattr(ref, kind)(I, 10, 50, nl, 0.0, 1, 1, "cpu")
        rows = edge if kind != "SRFU_R" else edge[1:]     # all-pad row is 0/0 -> NaN -> INT_MIN in the reference
        lab[kind] = m.get_Labels(t64(rows)).numpy().astype(np.int64)
    m = ref.SRFRN(I, 10, 45, 5, 0.0, 1, 1, "cpu")
    fi = t64(edge)
    lab["SRFRN_predict"] = (torch.sign(torch.count_nonzero(fi == 1, dim=1) - torch.count_nonzero(fi == 2, dim=1))
                            * 0.5 + 1.5).int().numpy().astype(np.int64)
    np.savez_compressed(os.path.join(HERE, "labels_edge.npz"), **lab)
    print("labels_edge done")


def c2_checksum():
    """BASELINE configs[1] / [2] at FULL size (50 000 items, seq_len 50, batch 512) through the REFERENCE's forward: the
    weights are too large to store (10 MB per kind), so the fixture pins the construction instead - under
    ``torch.manual_seed(seed)`` the drop-in classes create their parameter containers in the reference's order, so the
    same seed + ``xavier_normal_`` loop reproduces the reference's weights bit for bit (verified through the stored
    weight checksums) - and stores the reference's outputs on the seeded synthetic batch: full pos / neg logits and the
    last-position hidden states."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from srfrd_amd.sampler import synthetic_batch
    I2, L2, B2 = 50_000, 50, 512
    out = {"meta": np.array([I2, L2, B2], np.int64)}
    for k_i, kind in enumerate(["SASRec", "SRFRN", "SRFU_B"]):
        seed = 700 + k_i
        torch.manual_seed(seed)
        if kind == "SASRec":
            model = ref.SASRec(I2, L2, 50, 0.5, NB, NH, "cpu")
        elif kind == "SRFRN":
            model = ref.SRFRN(I2, L2, 45, 5, 0.5, NB, NH, "cpu")
        else:
            model = ref.SRFU_B(I2, L2, 50, 3, 0.5, NB, NH, "cpu")
        for _, p in model.named_parameters():          # reference trainer.py:364-369
            try:
                torch.nn.init.xavier_normal_(p.data)
            except Exception:
                pass
        model.eval()
        u, seq, rsq, pos, prs, neg, nrs = synthetic_batch(I2, L2, B2, seed=11 + k_i)
        with torch.no_grad():
            h, pl, nl = model(u, seq, rsq, pos, prs, neg, nrs)
        out[f"{kind}/seed"] = np.array([seed, 11 + k_i], np.int64)
        # correctly rounded sums (math.fsum): torch's parallel sum() depends on the host's thread count
        out[f"{kind}/w_sum"] = np.array([math.fsum(v.double().flatten().tolist()) for v in model.state_dict().values()], np.float64)
        out[f"{kind}/w_abs"] = np.array([math.fsum(v.double().abs().flatten().tolist()) for v in model.state_dict().values()], np.float64)
        out[f"{kind}/pos_logits"] = pl.numpy()
        out[f"{kind}/neg_logits"] = nl.numpy()
        out[f"{kind}/h_last"] = h[:, -1].numpy()
        out[f"{kind}/h_sum"] = np.array([float(h.double().sum()), float((h.double() ** 2).sum())], np.float64)
    path = os.path.join(HERE, "c2_reference_outputs.npz")
    np.savez_compressed(path, **out)
    print("c2 ->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if "--c2" in sys.argv:
        c2_checksum()
    elif "--heads" in sys.argv:
        main(HEAD_CASES)
    elif "--l2" in sys.argv:
        main(L2_CASES, l2_emb=0.05)
    else:
        main()
