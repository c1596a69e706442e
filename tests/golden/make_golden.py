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

    SRFRD_REFERENCE=<reference checkout> python -B tests/golden/make_golden.py --dropout   # tests/golden/drop_*.npz

``--dropout``: the train-mode fixtures of ``tests.helpers.DROP_CASES`` (dropout p > 0, the configuration every bench
workload trains).  The reference's classes run in ``.train()`` with ``torch.nn.functional.dropout`` replaced, for the
duration of the run, by ``SiteDropout``: it returns the project's counter-hash keep masks (``oracle.srfrd_oracle.keep_mask``
at the ``SITE_EMB`` / ``site_*`` coordinates), because torch's RNG stream cannot be reproduced by a device kernel.  The
masks are a project convention; everything around them is the reference's: which tensor each mask multiplies, its layout
(mapped from torch's documented layouts only), the ``1 / (1 - p)`` scale and all arithmetic downstream, forward and
backward.  The reference runs in float64 from the float32 initial weights and every result is stored as float32, so a
fixture carries no float32 summation-order noise: the oracle, run in float64, must agree to storage rounding.  Three Adam
steps draw their masks from ``step_seed(S, t)``, t = 1, 2, 3, with b0 = 0 - what ``FusedTrainer(seed=S)`` draws on one
rank.  Stored: S, p, b0, step-1 logits, hidden states (the last position only above 1000 sequence positions: size), loss
of steps 1-3, every step-1 gradient, the weights after steps 1 and 3 (as the XOR of their float32 bits with the previous
weights': lossless, and unchanged elements compress away), and a digest of every (step, site) keep mask (kept count,
SHA-256 of the packed keep bits in oracle coordinates) so that a failing test tells a changed hash from a misplaced mask.
The seq_len-20 cases start from the inputs and weights of <class>.npz / <class>_h2.npz; the longer ones store their inputs
and regenerate their initial weights from ``init_seed`` (tests.helpers.drop_init_weights, checked by ``w_sha256``).
If the hash of srfrd_amd/csrc/srfrd_rng.h and the oracle is ever changed on purpose, these fixtures must be regenerated.
The output is bit-for-bit reproducible (fixed zip timestamps, one CPU thread).
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

sys.path.insert(1, os.path.dirname(os.path.dirname(HERE)))
from oracle import srfrd_oracle as O  # noqa: E402
from tests.helpers import DROP_CASES, drop_init_weights, load_golden, weights_sha256  # noqa: E402

I, L, B = 1000, 20, 8            # C1's catalog (BASELINE configs[0]: 1k items, seq_len 20)
D_ITEM, D_FAKE, NB, NH = 45, 5, 2, 1


def make_inputs(seed, I=I, L=L, B=B, edges=False):
    """edges (the --dropout fixtures at seq_len >= 50): the batch also holds lengths 2 and L - 1 and one interior pad
    (item id 0 between items) besides lengths L and 1 and the SRFU tie / all-fake rows."""
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
    if edges:
        lens[4] = 2
        lens[5] = L - 1
        lens[6] = max(int(lens[6]), 4)
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
        if edges and b == 6:   # interior pad: the sequence's second item is a padding id
            seq[b, L - n + 1] = rsq[b, L - n + 1] = 0
    return seq, rsq, pos, prs, neg, nrs


def build(kind, dropout, nh=NH, I=I, L=L):
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


# ---- --dropout: train-mode fixtures (tests.helpers.DROP_CASES) ---------------------------------------------------------
class SiteDropout:
    """Stand-in for ``torch.nn.functional.dropout`` during one reference forward.

    Both of the reference's dropout call sites resolve through that module attribute: ``nn.Dropout.forward`` calls
    ``F.dropout``, and torch's explicit multi-head attention path (``need_weights=True``, the reference's default: no fast
    path) calls the module-global ``dropout`` on the attention weights.  Calls are mapped to sites by their order in one
    forward - SASRec: the embedding, then per block attention, FFN 1, FFN 2; SRFR / SRFRN / SRFU_*: attention, FFN 1,
    FFN 2 per block (their embedding Dropout modules are never called) - and each call's shape, p and training flag are
    asserted against the site's.  Layouts, from torch's documentation:
      * embedding: (B, L, D), the oracle's (sequence, position, channel);
      * attention weights: (B * H, L, L) indexed [b * H + h, query, key] (q.view(L, B * H, head_dim).transpose(0, 1));
      * FFN: the Conv1d layout (B, D, L), the oracle's (position, channel) mask transposed.
    Kept elements are scaled as torch's dropout scales them: keep mask divided by (1 - p), multiplied into the input."""

    def __init__(self, kind, B, L, D, H, p, nb=NB):
        self.B, self.L, self.D, self.H, self.p = B, L, D, H, p
        self.order = [("emb", O.SITE_EMB)] if kind == "SASRec" else []
        for i in range(nb):
            self.order += [("attn", i), ("ffn", O.site_ffn1(i)), ("ffn", O.site_ffn2(i))]
        self.sites = [O.SITE_EMB] if kind == "SASRec" else []
        for i in range(nb):
            self.sites += [O.site_attn(i, h) for h in range(H)] + [O.site_ffn1(i), O.site_ffn2(i)]

    def begin(self, seed):
        self.seed, self.calls, self.keep = seed, 0, {}

    def end(self):
        assert self.calls == len(self.order), (self.calls, len(self.order))

    def _keep(self, site, R, C):
        k = O.keep_mask(self.seed, site, 0, self.B, R, C, self.p) > 0          # (B, R, C) bool, oracle coordinates
        self.keep[site] = k.numpy()
        return k

    def __call__(self, input, p=0.5, training=True, inplace=False):
        assert self.calls < len(self.order), "more dropout calls than sites in one forward"
        what, i = self.order[self.calls]
        self.calls += 1
        assert training is True and p == self.p and not inplace, (what, i, p, training, inplace)
        B, L, D, H = self.B, self.L, self.D, self.H
        if what == "emb":
            assert tuple(input.shape) == (B, L, D), (what, tuple(input.shape))
            keep = self._keep(i, L, D)
        elif what == "attn":
            assert tuple(input.shape) == (B * H, L, L), (what, tuple(input.shape))
            keep = torch.stack([self._keep(O.site_attn(i, h), L, L) for h in range(H)], dim=1).reshape(B * H, L, L)
        else:
            assert tuple(input.shape) == (B, D, L), (what, tuple(input.shape))
            keep = self._keep(i, L, D).transpose(1, 2)
        mask = keep.to(input.dtype).div_(1.0 - p)
        return input * mask


def savez_fixed(path, **arrays):
    """np.savez_compressed with fixed zip timestamps: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue())


def dropout_main():
    import hashlib
    torch.set_num_threads(1)
    for c_i, (name, kind, Lc, Bc, Ic, nh, p) in enumerate(DROP_CASES):
        S = 4000 + 37 * c_i
        model = build(kind, p, nh, I=Ic, L=Lc)
        out = {"seed": np.int64(S), "p": np.float64(p), "b0": np.int64(0)}
        if Lc == L:
            _, sd, batch = load_golden(kind, nh)          # the dropout-free fixture's inputs and initial weights
            model.load_state_dict(sd, strict=True)
            seq, rsq, pos, prs, neg, nrs = (b.numpy() for b in batch)
        else:                                             # weights regenerated at test time from init_seed (size)
            assert set(model.state_dict()) == {k for k, _ in model.named_parameters()}
            out["init_seed"] = np.int64(5000 + c_i)
            model.load_state_dict(drop_init_weights(5000 + c_i, {k: v.shape for k, v in model.state_dict().items()}),
                                  strict=True)
            seq, rsq, pos, prs, neg, nrs = make_inputs(300 + c_i, Ic, Lc, Bc, edges=True)
            for k, v in (("seq", seq), ("rsq", rsq), ("pos", pos), ("prs", prs), ("neg", neg), ("nrs", nrs)):
                out[k] = v.astype(np.int32)
        out["w_sha256"] = weights_sha256({k: v.detach() for k, v in model.state_dict().items()})
        model.double()           # float64 run: the fixture carries the reference's arithmetic without float32 rounding
        assert seq.shape == (Bc, Lc)
        D = model.state_dict()["last_layernorm.weight"].shape[0] if kind != "SRFR" else D_ITEM + D_FAKE
        hook = SiteDropout(kind, Bc, Lc, D, nh, p)
        u = torch.zeros(Bc, dtype=torch.int64)
        crit = torch.nn.BCEWithLogitsLoss()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.98))
        kept = np.zeros((3, len(hook.sites)), np.int64)
        sha = np.zeros((3, len(hook.sites), 32), np.uint8)
        prev = {k: v.detach().float().numpy() for k, v in model.state_dict().items()}
        model.train()
        saved = torch.nn.functional.dropout
        torch.nn.functional.dropout = hook
        try:
            for step in range(3):
                hook.begin(O.step_seed(S, step + 1))
                h, pl, nl = model(user_ids=u, input_ids=t64(seq), fake_ids=t64(rsq), positive_ids=t64(pos),
                                  positive_fake_ids=t64(prs), negative_ids=t64(neg), negative_fake_ids=t64(nrs))
                hook.end()
                for j, site in enumerate(hook.sites):
                    kept[step, j] = int(hook.keep[site].sum())
                    sha[step, j] = np.frombuffer(hashlib.sha256(np.packbits(hook.keep[site].ravel()).tobytes()).digest(), np.uint8)
                opt.zero_grad()
                idx = torch.where(t64(pos) != 0)
                loss = crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])
                loss.backward()
                if step == 0:
                    out["pos_logits"], out["neg_logits"] = pl.detach().float().numpy(), nl.detach().float().numpy()
                    hd = h.detach().float().numpy()
                    if Bc * Lc > 1000:       # (size: the logits still cover every position)
                        out["h_last"] = hd[:, -1].copy()
                    else:
                        out["hidden"] = hd.copy()
                    for k, prm in model.named_parameters():
                        out["g/" + k] = prm.grad.detach().float().numpy()
                opt.step()
                if step in (0, 2):          # bit pattern XOR the previous weights' (lossless; unchanged elements -> 0)
                    for k, v in model.state_dict().items():
                        w = v.detach().float().numpy()
                        out[f"x{step + 1}/" + k] = w.view(np.int32) ^ prev[k].view(np.int32)
                        prev[k] = w
                out[f"loss{step}"] = np.float32(loss.item())
        finally:
            torch.nn.functional.dropout = saved
        out["mask_sites"] = np.array(hook.sites, np.int64)
        out["mask_kept"], out["mask_sha256"] = kept, sha
        path = os.path.join(HERE, name + ".npz")
        savez_fixed(path, **out)
        print(name, "->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    if "--dropout" in sys.argv:
        dropout_main()
    elif "--c2" in sys.argv:
        c2_checksum()
    elif "--heads" in sys.argv:
        main(HEAD_CASES)
    elif "--l2" in sys.argv:
        main(L2_CASES, l2_emb=0.05)
    else:
        main()
