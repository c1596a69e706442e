"""Latency of the sampled softmax cross-entropy with shared negatives (model.sampled_softmax_loss: srfrd_sxent_fwd /
srfrd_sxent_bwd).

    python tools/sxent_latency.py [--reps 10] [--out profiles/sxent_latency.json]

Configurations: C2 (SASRec, 50k items, B = 512, L = 50) with K = 256, 1024 and 8192 shared negatives, and C5 (1M items,
L = 200, B = 64 and 512) with K = 8192; hidden width 50, the hidden states of a real encoder forward over a synthetic batch
(lengths as the sampler draws them), its next-item targets, and negatives with their log-Q correction from
srfrd_amd.sample_negatives (uniform).  Per configuration: forward and backward of the fused op (the backward includes the
key sort and the table reduction of the host layer), and - where its (tokens x (1 + K)) fp32 logits fit comfortably -
torch's materialised fp32 path (gathered rows, logits, logsumexp, autograd).  Median over ``--reps`` after warm-up, CUDA
events.  ``*_tflops`` counts the logit-GEMM-sized passes (forward 1, backward 4) at 2 * tokens * K * 50 flop each;
``*_of_peak`` divides by the 155 TF measured fp32 matrix peak.  Each configuration runs in a fresh child process with its
own time limit.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"C2_K256": dict(I=50_000, L=50, B=512, K=256), "C2_K1024": dict(I=50_000, L=50, B=512, K=1024),
           "C2_K8192": dict(I=50_000, L=50, B=512, K=8192), "C5_B64_K8192": dict(I=1_000_000, L=200, B=64, K=8192),
           "C5_B512_K8192": dict(I=1_000_000, L=200, B=512, K=8192)}
PEAK_TF = 155.0
TORCH_LIMIT_BYTES = 40e9            # the materialised path holds about four (tokens x (1 + K)) fp32 matrices


def child(name: str, reps: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    from srfrd_amd.loss_heads import SXENT, launch_bwd, launch_fwd
    from srfrd_amd._lib import ptr
    cfg = CONFIGS[name]
    I, L, B, K = cfg["I"], cfg["L"], cfg["B"], cfg["K"]
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    _, seq, rsq, pos, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda")
    with torch.no_grad():
        h, _, _ = m(None, seq, rsq)
    neg, log_q = srfrd_amd.sample_negatives(I, K, generator=torch.Generator(device="cuda").manual_seed(2))
    lay, tab = m.layout, ptr(m.flat_parameters())
    tokens = int((pos != 0).sum())
    tl, lse, stats = launch_fwd(SXENT, lay, tab, h, pos, (neg, log_q, True))
    g = (torch.ones((), device="cuda") / stats[1]).expand(B, L).contiguous()
    runs = {"fwd": lambda: launch_fwd(SXENT, lay, tab, h, pos, (neg, log_q, True)),
            "bwd": lambda: launch_bwd(SXENT, lay, tab, h, pos, (neg, log_q, True), lse, g)}
    if 4.0 * tokens * (K + 1) * 4 <= TORCH_LIMIT_BYTES:
        E = m.item_emb.weight.detach().clone().requires_grad_(True)
        hv = h.detach().clone().requires_grad_(True)
        tok = (pos != 0).view(-1)
        t = pos.view(-1)[tok]

        def torch_step():
            H = hv.view(-1, 50)[tok]
            sp = (H * E[t]).sum(1)
            sn = (H @ E[neg].T - log_q).masked_fill((neg == 0).unsqueeze(0) | (neg.unsqueeze(0) == t.unsqueeze(1)), -float("inf"))
            loss = (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()
            loss.backward()
        runs["torch_fp32_fwd_bwd"] = torch_step
    out = _time(runs, {"config": name, **cfg, "tokens": tokens, "reps": reps}, reps)
    pass_flop = 2.0 * tokens * K * 50
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
