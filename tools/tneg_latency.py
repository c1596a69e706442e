"""Latency of the losses with K negatives per position (model.token_negatives_loss: srfrd_tneg_fwd / srfrd_tneg_bwd and
srfrd_table_reduce_rank1).

    python tools/tneg_latency.py [--reps 10] [--out profiles/tneg_latency.json]

Configurations: C2 (SASRec, 50k items, B = 512, L = 50) with K = 16, 64 and 256 negatives per position, and the C5 shape
(1M items, L = 200, B = 64) with K = 128; both objectives; hidden width 50, the hidden states of a real encoder forward over
a synthetic batch (lengths as the sampler draws them), its next-item targets, and negatives with their log-Q correction from
srfrd_amd.sample_token_negatives (uniform).  Per configuration and objective: forward and backward of the fused op (the
backward includes the key sort and the rank-1 table reduction of the host layer; ``bwd_kernel_ms`` / ``sort_ms`` /
``reduce_ms`` time its three parts on their own), and torch's materialised fp32 path for the same loss (gather E[neg] as
(tokens, K, 50), einsum, masking, logsumexp / softplus, autograd), which is what a user would write without the op.  Median
over ``--reps`` after warm-up, CUDA events.  ``*_gather_tbs``: tokens * (1 + K) * 200 bytes over the time of the pass, the
rate at which table rows are gathered, to set beside the 8.6 TB/s measured for rows gathered from the Infinity Cache.  Each
configuration runs in a fresh child process with its own time limit.

    python tools/tneg_latency.py --sampler [--reps 10] [--out profiles/tneg_sampler_latency.json]

times what feeds that loss instead: DeviceSampler.token_negatives (srfrd_token_negatives, one launch into preallocated
outputs) at the C2 shape (B = 512, L = 50, 50k items; 4096 synthetic users with 5..200 training items each) for K = 16, 64
and 256, uniform and by popularity (alias table, counts ** 0.75), with and without history exclusion; beside each,
srfrd_amd.sample_token_negatives (torch.randint / torch.multinomial, no exclusion) on the same positions in the same process.
``store_gbs``: the bytes of the two outputs (12 per slot) over the kernel's time.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"C2_K16": dict(I=50_000, L=50, B=512, K=16), "C2_K64": dict(I=50_000, L=50, B=512, K=64),
           "C2_K256": dict(I=50_000, L=50, B=512, K=256), "C5_B64_K128": dict(I=1_000_000, L=200, B=64, K=128)}
OBJECTIVES = ("softmax", "gbce")


def child(name: str, reps: int, only: str | None = None) -> list:
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import srfrd_amd
    from srfrd_amd import _lib
    from srfrd_amd.loss_heads import TNEG, launch_bwd, launch_fwd
    from srfrd_amd._lib import check, ptr
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
    neg, log_q = srfrd_amd.sample_token_negatives(I, pos, K, generator=torch.Generator(device="cuda").manual_seed(2))
    lay, tab = m.layout, ptr(m.flat_parameters())
    tokens = int((pos != 0).sum())
    beta = srfrd_amd.gbce_beta(I, K, 0.75)
    L_ = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    results = []
    for objective in OBJECTIVES:
        if only and objective != only:
            continue
        code = _lib.TNEG_OBJECTIVES[objective]
        lq = log_q if objective == "softmax" else None
        tl, lse, stats = launch_fwd(TNEG, lay, tab, h, pos, (neg, lq, code, beta, True))
        g = (torch.ones((), device="cuda") / stats[1]).expand(B, L).contiguous()
        # the backward's three parts on buffers of their own
        ws = torch.empty(L_.srfrd_tneg_workspace_floats(C.byref(lay), B, L, K), device="cuda", dtype=torch.float32)
        dh = torch.empty(B, L, lay.d_out, device="cuda", dtype=torch.float32)
        coef = torch.empty(B * L * (1 + K), device="cuda", dtype=torch.float32)
        keys = torch.empty(B * L * (1 + K), device="cuda", dtype=torch.int64)
        de = torch.zeros(I + 1, 50, device="cuda", dtype=torch.float32)

        def bwd_kernel():
            check(L_.srfrd_tneg_bwd(C.byref(lay), tab, ptr(h), ptr(pos), ptr(neg), ptr(lq), K, code, beta, 1, ptr(lse), ptr(g), B,
                                    L, ptr(dh), ptr(coef), ptr(keys), ptr(ws), ws.numel(), stream), "srfrd_tneg_bwd")
        bwd_kernel()
        skeys, order = torch.sort(keys, stable=True)

        def reduce():
            check(L_.srfrd_table_reduce_rank1(ptr(skeys), ptr(order), ptr(coef), ptr(h), lay.d_out, 1 + K, skeys.numel(), 50,
                                              ptr(de), ptr(ws), ws.numel(), stream), "srfrd_table_reduce_rank1")
        E = m.item_emb.weight.detach().clone().requires_grad_(True)
        hv = h.detach().clone().requires_grad_(True)
        tok = (pos != 0).view(-1)
        t = pos.view(-1)[tok]
        N = neg.view(-1, K)[tok]
        LQ = log_q.view(-1, K)[tok]
        mask = (N == 0) | (N == t.unsqueeze(1))

        def torch_step():
            H = hv.view(-1, 50)[tok]
            sp = (H * E[t]).sum(1)
            sn = torch.einsum("td,tkd->tk", H, E[N])
            if objective == "softmax":
                sn = (sn - LQ).masked_fill(mask, -float("inf"))
                loss = (torch.logsumexp(torch.cat([sp.unsqueeze(1), sn], 1), 1) - sp).mean()
            else:
                f = torch.nn.functional.softplus
                loss = (beta * f(-sp) + f(sn).masked_fill(mask, 0.0).sum(1)).mean()
            loss.backward()
        runs = {"fwd": lambda: launch_fwd(TNEG, lay, tab, h, pos, (neg, lq, code, beta, True)),
                "bwd": lambda: launch_bwd(TNEG, lay, tab, h, pos, (neg, lq, code, beta, True), lse, g),
                "bwd_kernel": bwd_kernel, "sort": lambda: torch.sort(keys, stable=True), "reduce": reduce,
                "torch_fp32_fwd_bwd": torch_step}
        out = _time(runs, {"config": name, "objective": objective, **cfg, "tokens": tokens, "reps": reps}, reps)
        gather_bytes = tokens * (1 + K) * 200.0
        out["fwd_gather_tbs"] = round(gather_bytes / (out["fwd_ms"] * 1e-3) / 1e12, 3)
        out["bwd_kernel_gather_tbs"] = round(gather_bytes / (out["bwd_kernel_ms"] * 1e-3) / 1e12, 3)
        out["fwd_bwd_ms"] = round(out["fwd_ms"] + out["bwd_ms"], 4)
        out["speedup_vs_torch"] = round(out["torch_fp32_fwd_bwd_ms"] / out["fwd_bwd_ms"], 2)
        results.append(out)
    return results


def sampler_child(reps: int) -> list:
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import srfrd_amd
    I, L, B, U = 50_000, 50, 512, 4096
    rng = np.random.RandomState(0)
    lens = rng.randint(5, 201, U)
    users = np.repeat(np.arange(1, U + 1), lens)
    data = srfrd_amd.partition(users, np.concatenate([rng.randint(1, I + 1, users.size - 1), [I]]), rng.rand(users.size) < 0.3)
    counts = np.bincount(data.train_items, minlength=I + 1).astype(np.float64)
    results = []
    for K in (16, 64, 256):
        for dist in ("uniform", "alias"):
            kw = dict(neg_counts=counts, neg_alpha=0.75) if dist == "alias" else {}
            out = {"config": f"C2_K{K}", "distribution": dist, "I": I, "L": L, "B": B, "K": K, "reps": reps,
                   "max_hist": int(data.train_len().max()), "out_bytes": B * L * K * 12}
            runs = {}
            for exclude in (True, False):
                s = srfrd_amd.DeviceSampler(data, B, L, seed=1, num_negatives=K, exclude_history=exclude, **kw)
                user, _, _, pos, *_ = s.next_batch()
                neg, lq = torch.empty_like(s.negatives), torch.empty_like(s.log_q)
                runs["kernel_exclude" if exclude else "kernel_no_exclude"] = (
                    lambda s=s, user=user, pos=pos, neg=neg, lq=lq: s.token_negatives(user, pos, index=1, out=neg, out_log_q=lq))
            cnt = counts if dist == "alias" else None
            runs["torch_no_exclude"] = lambda: srfrd_amd.sample_token_negatives(I, pos, K, counts=cnt, alpha=0.75)
            _time(runs, out, reps)
            out["tokens"] = int((pos != 0).sum())
            out["store_gbs"] = round(out["out_bytes"] / (out["kernel_exclude_ms"] * 1e-3) / 1e9, 1)
            out["torch_over_kernel"] = round(out["torch_no_exclude_ms"] / out["kernel_exclude_ms"], 2)
            results.append(out)
    return results


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
    ap.add_argument("--objective", default=None, choices=OBJECTIVES)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--sampler", action="store_true", help="time the per-position negative sampler instead of the loss")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(sampler_child(a.reps) if a.sampler else child(a.child, a.reps, a.objective)))
        return
    results = []
    for name in (["sampler"] if a.sampler else a.configs.split(",")):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)]
        if a.sampler:
            cmd.append("--sampler")
        if a.objective:
            cmd += ["--objective", a.objective]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout, cwd=ROOT)
        except subprocess.TimeoutExpired:
            results.append({"config": name, "error": "timeout"})
            print(json.dumps(results[-1]), flush=True)
            break                                   # a step that hung: start nothing more on the GPU
        if p.returncode != 0:
            results.append({"config": name, "error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]})
            print(json.dumps(results[-1]), flush=True)
            break
        for r in json.loads(p.stdout.strip().splitlines()[-1]):
            results.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
    if any("error" in r for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
