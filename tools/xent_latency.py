"""Latency of the full-catalog softmax cross-entropy (model.full_catalog_loss: srfrd_xent_fwd / srfrd_xent_bwd).

    python tools/xent_latency.py [--reps 10] [--out profiles/xent_latency.json]

Configurations: C2 (SASRec, 50k items, B = 512, L = 50) and C5 (1M items, L = 200, B = 64 and 512), hidden width 50, the
hidden states of a real encoder forward over a synthetic batch (lengths as the sampler draws them) and its next-item
targets.  Per configuration: forward and backward of the fused op, and - where its (tokens x items) fp32 logits fit
comfortably - torch's materialised fp32 path (logits = h @ E.T, F.cross_entropy, autograd).  Median over ``--reps`` after
warm-up, CUDA events.  ``*_tflops`` counts the logit-GEMM-sized passes (forward 1, backward 4) at 2 * tokens * items * 50
flop each; ``*_of_peak`` divides by the 155 TF measured fp32 matrix peak.  Each configuration runs in a fresh child process
with its own time limit.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"C2": dict(I=50_000, L=50, B=512), "C5_B64": dict(I=1_000_000, L=200, B=64),
           "C5_B512": dict(I=1_000_000, L=200, B=512)}
PEAK_TF = 155.0
TORCH_LIMIT_BYTES = 40e9            # the materialised path holds about four (tokens x items) fp32 matrices


def child(name: str, reps: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import srfrd_amd
    from srfrd_amd.loss_heads import XENT, launch_bwd, launch_fwd
    from srfrd_amd._lib import ptr
    cfg = CONFIGS[name]
    I, L, B = cfg["I"], cfg["L"], cfg["B"]
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    _, seq, rsq, pos, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda")
    with torch.no_grad():
        h, _, _ = m(None, seq, rsq)
    lay, tab = m.layout, ptr(m.flat_parameters())
    tokens = int((pos != 0).sum())
    tl, lse, stats = launch_fwd(XENT, lay, tab, h, pos)
    g = (torch.ones((), device="cuda") / stats[1]).expand(B, L).contiguous()
    runs = {"fwd": lambda: launch_fwd(XENT, lay, tab, h, pos),
            "bwd": lambda: launch_bwd(XENT, lay, tab, h, pos, (), lse, g)}
    if 4.0 * tokens * I * 4 <= TORCH_LIMIT_BYTES:
        E = m.item_emb.weight.detach().clone().requires_grad_(True)
        hv = h.detach().clone().requires_grad_(True)
        y = pos - 1

        def torch_step():
            logits = hv @ E.T
            loss = F.cross_entropy(logits[..., 1:].reshape(-1, I), y.reshape(-1), ignore_index=-1)
            loss.backward()
        runs["torch_fp32_fwd_bwd"] = torch_step
    out = _time(runs, {"config": name, **cfg, "tokens": tokens, "reps": reps}, reps)
    pass_flop = 2.0 * tokens * I * 50
    for k, passes in (("fwd", 1), ("bwd", 4)):
        tf = passes * pass_flop / (out[k + "_ms"] * 1e-3) / 1e12
        out[k + "_tflops"] = round(tf, 2)
        out[k + "_of_peak"] = round(tf / PEAK_TF, 4)
    out["fwd_bwd_ms"] = round(out["fwd_ms"] + out["bwd_ms"], 4)
    return out


def _time(runs, out, reps):
    import torch
    for label, fn in runs.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ts.sort()
        out[label + "_ms"] = round(ts[len(ts) // 2], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.reps)))
        return
    results = []
    for name in a.configs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)],
                               capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
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
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    if any("error" in r for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
