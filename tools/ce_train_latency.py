"""Step time of the fused train step under each loss (FusedTrainer(loss=...), one HIP graph per step) against the module-level
loop on the same loss (model(...) -> loss -> backward -> srfrd_amd.Adam).

    python tools/ce_train_latency.py [--reps 20] [--out profiles/ce_train_latency.json]

Workload C2: SASRec, 50k items, B = 512, L = 50, hidden 50, dropout 0.2 (bench.py's model), one synthetic batch resident
in the trainer's input ring.  Losses: "bce" (the reference's masked BCE), "sampled_softmax" with K = 256, 1024 and 8192
shared negatives (uniform, log-Q corrected, accidental hits removed), "softmax" (the full catalog).  The module-level loop
draws its negatives with srfrd_amd.sample_negatives, the trainer draws them in the graph.  "token_softmax" / "gbce" with
K = 16, 64 and 256 negatives per position: both sides draw batch and negatives with
DeviceSampler(num_negatives=K) over a synthetic interaction set of the C2 shape, inside the timed step - the fused side
straight into the trainer's rings (``step_slot``), the module side into ``model(...)`` -> ``token_negatives_loss``.

    python tools/ce_train_latency.py --configs token_softmax_K16,...,gbce_K256 --out profiles/token_train_latency.json
    rocprofv3 --kernel-trace --stats -- python tools/ce_train_latency.py --child token_softmax_K64 --fused-only

Per configuration and path: ``*_step_ms`` = median over ``--reps`` single steps, each bracketed by CUDA events and waited
for (what one step costs from launch to finish); ``*_pipelined_ms`` = CUDA events around ``--reps`` back-to-back steps,
divided by their number (the rate of a training loop that never synchronises).  Warm-up first; each configuration runs in
a fresh child process with its own time limit.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"bce": dict(loss="bce", K=0), "sampled_K256": dict(loss="sampled_softmax", K=256),
           "sampled_K1024": dict(loss="sampled_softmax", K=1024), "sampled_K8192": dict(loss="sampled_softmax", K=8192),
           "softmax": dict(loss="softmax", K=0)}
CONFIGS.update({f"{loss}_K{K}": dict(loss=loss, K=K) for loss in ("token_softmax", "gbce") for K in (16, 64, 256)})
TOKEN = ("token_softmax", "gbce")
I, L, B, D = 50_000, 50, 512, 50


def _time(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return round(ts[len(ts) // 2], 4), round(a.elapsed_time(b) / reps, 4)


def _model():
    import torch
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, D, 0.2, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _interactions(n_users=20_000, seed=7):
    """a synthetic interaction set over the C2 catalog: histories of 3..60 uniform items"""
    import numpy as np
    import srfrd_amd
    rng = np.random.RandomState(seed)
    lens = rng.randint(3, 61, n_users)
    users = np.repeat(np.arange(1, n_users + 1), lens)
    items = rng.randint(1, I + 1, users.size)
    items[0] = I                                    # itemnum is the largest id seen
    return srfrd_amd.partition(users, items, rng.rand(users.size) < 0.3)


def child_token(name: str, reps: int, warmup: int, fused_only: bool = False) -> dict:
    """the token-negatives losses: the sampler's two launches are part of both timed steps"""
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    loss, K = CONFIGS[name]["loss"], CONFIGS[name]["K"]
    objective = "softmax" if loss == "token_softmax" else "gbce"
    beta = srfrd_amd.gbce_beta(I, K, 0.75) if loss == "gbce" else 1.0
    data = _interactions()
    out = {"config": name, "loss": loss, "K": K, "n_items": I, "B": B, "L": L, "reps": reps}

    tr = srfrd_amd.FusedTrainer(_model(), B, L, loss=loss, num_negatives=K, gbce_beta=beta)
    sampler = srfrd_amd.DeviceSampler(data, B, L, seed=3, num_negatives=K, model=tr)

    def fused():
        sampler.next_batch(packed=True, out=tr.ids_ring[0], neg_out=tr.neg_ring[0], log_q_out=tr.log_q_ring[0])
        tr.step_slot(0)

    for _ in range(warmup):
        fused()
    torch.cuda.synchronize()
    out["tokens"] = int((tr.ids_ring[0][2] != 0).sum())
    out["fused_graph_step_ms"], out["fused_graph_pipelined_ms"] = _time(fused, reps)
    out["fused_loss_last"] = round(float(tr.loss), 5)
    del tr
    if fused_only:
        return out

    m = _model()
    opt = srfrd_amd.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.98))
    sampler = srfrd_amd.DeviceSampler(data, B, L, seed=3, num_negatives=K, model=m)

    def module():
        opt.zero_grad()
        _, seq, rsq, pos, _, _, _ = sampler.next_batch()
        h, _, _ = m(None, seq, rsq)
        lq = sampler.log_q if objective == "softmax" else None
        lo = m.token_negatives_loss(h, pos, sampler.negatives, objective, lq, beta)
        lo.backward()
        opt.step()

    for _ in range(warmup):
        module()
    torch.cuda.synchronize()
    out["module_step_ms"], out["module_pipelined_ms"] = _time(module, reps)
    out["speedup_step"] = round(out["module_step_ms"] / out["fused_graph_step_ms"], 2)
    return out


def child(name: str, reps: int, warmup: int, fused_only: bool = False) -> dict:
    if CONFIGS[name]["loss"] in TOKEN:
        return child_token(name, reps, warmup, fused_only)
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    cfg = CONFIGS[name]
    loss, K = cfg["loss"], cfg["K"]
    packed = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda", packed=True)[1]
    out = {"config": name, "loss": loss, "K": K, "n_items": I, "B": B, "L": L, "reps": reps,
           "tokens": int((packed[2] != 0).sum())}

    tr = srfrd_amd.FusedTrainer(_model(), B, L, loss=loss, num_negatives=max(K, 1))
    tr.ids_ring[0].copy_(packed)
    fused = lambda: tr.step_slot(0)
    for _ in range(warmup):
        fused()
    torch.cuda.synchronize()
    out["fused_graph_step_ms"], out["fused_graph_pipelined_ms"] = _time(fused, reps)
    out["fused_loss_last"] = round(float(tr.loss), 5)
    del tr

    m = _model()
    opt = srfrd_amd.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.98))
    seq, rsq, pos, prs, neg, nrs = packed.unbind(0)
    crit = torch.nn.BCEWithLogitsLoss()
    gen = torch.Generator(device="cuda").manual_seed(2)

    def module():
        opt.zero_grad()
        if loss == "bce":
            h, pl, nl = m(None, seq, rsq, pos, prs, neg, nrs)
            idx = torch.where(pos != 0)
            lo = crit(pl[idx], torch.ones_like(pl)[idx]) + crit(nl[idx], torch.zeros_like(nl)[idx])
        else:
            h, _, _ = m(None, seq, rsq)
            if loss == "softmax":
                lo = m.full_catalog_loss(h, pos)
            else:
                negs, log_q = srfrd_amd.sample_negatives(I, K, generator=gen)
                lo = m.sampled_softmax_loss(h, pos, negs, log_q)
        lo.backward()
        opt.step()

    for _ in range(warmup):
        module()
    torch.cuda.synchronize()
    out["module_step_ms"], out["module_pipelined_ms"] = _time(module, reps)
    out["speedup_step"] = round(out["module_step_ms"] / out["fused_graph_step_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--fused-only", action="store_true", help="with --child, a token-negatives config: the graph step alone (a profiler run)")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: at least 10")
    if a.child:
        print(json.dumps(child(a.child, a.reps, a.warmup, a.fused_only)))
        return
    results = []
    for name in a.configs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                                "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            results.append({"config": name, "error": "timeout"})
            print(json.dumps(results[-1]), flush=True)
            break                                   # a step that hung: start nothing more on the GPU
        if p.returncode != 0:
            results.append({"config": name, "error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]})
            print(json.dumps(results[-1]), flush=True)
            break
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    if any("error" in r for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
