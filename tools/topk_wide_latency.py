"""Latency of the wide full-catalog top-k (srfrd::logits_topk_wide) beside the k <= 64 op and beside materialise-then-torch.topk.

    python tools/topk_wide_latency.py [--reps 15] [--out profiles/topk_wide_latency.json]

Configurations: SASRec hidden 50, B = 512, the C2 (50k items) and C5 (1M items) catalogs, fp32 table and bf16 shadow.  Per
configuration, the ranking op only (the last-position encoder state is computed once, outside the timed region):
  narrow_k64           srfrd::logits_topk at k = 64
  wide_k{64,100,256,1024}   srfrd::logits_topk_wide
  torch_k{64,100,256,1024}  hidden[:, -1] @ table.T (the (B, n_items) logits in memory), then torch.topk; on the bf16
                       configurations the product is a bf16 matmul on the bf16 shadow, its bf16 result widened to fp32
                       before torch.topk (half the logits bytes of the fp32 configurations' product)
  wide_k{100,1024}_fallback  the wide op with user 0's hidden state zeroed: all of its scores tie, its candidates overflow,
                       its list comes from the fallback workgroup
Protocol: all variants interleaved in one process - every window times each variant once, in order - and the figure of a
variant is the median over ``--reps`` windows after three warm-up windows, CUDA events.  Every configuration runs in a fresh
child process with its own time limit; a child that fails or hangs ends the run.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"C2": dict(I=50_000, L=50, B=512, bf16=False), "C2_bf16": dict(I=50_000, L=50, B=512, bf16=True),
           "C5": dict(I=1_000_000, L=200, B=512, bf16=False), "C5_bf16": dict(I=1_000_000, L=200, B=512, bf16=True)}
KS = (64, 100, 256, 1024)


def child(name: str, reps: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    from srfrd_amd import ops
    cfg = CONFIGS[name]
    I, L, B = cfg["I"], cfg["L"], cfg["B"]
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    if cfg["bf16"]:
        m.use_bf16_table()
    _, seq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda")
    m._ensure_flat()
    with torch.no_grad():
        h = m._launch_fwd_last(seq, None)
    key = ops.register_model(m)
    hi = I + 1
    h_tied = h.clone()
    h_tied[0] = 0.0
    last = h[:, -1].contiguous()
    if cfg["bf16"]:
        table, last = m._table16.view(torch.bfloat16).reshape(hi, -1), last.to(torch.bfloat16)
    else:
        table = m._item_param().detach()

    def baseline(k):
        return torch.topk((last @ table.T).float(), k, dim=1)

    wide = lambda hid, k: torch.ops.srfrd.logits_topk_wide(hid, None, key, 0, hi, k, True, None, None, 0)
    runs = {"narrow_k64": lambda: torch.ops.srfrd.logits_topk(h, None, key, 0, hi, 64, True)}
    for k in KS:
        runs[f"wide_k{k}"] = lambda k=k: wide(h, k)
        runs[f"torch_k{k}"] = lambda k=k: baseline(k)
    for k in (100, 1024):
        runs[f"wide_k{k}_fallback"] = lambda k=k: wide(h_tied, k)
    # the lists agree before anything is timed (ids; near ties may swap between the two arithmetics)
    wi, _ = wide(h, 100)
    ti = baseline(100).indices
    agree = float((wi == ti).float().mean()) if not cfg["bf16"] else None
    fi, fv = wide(h_tied, 100)
    assert bool((fi[0] == torch.arange(1, 101, device="cuda")).all()) and bool((fv[0] == 0).all()), "fallback list"
    out = {"config": name, **cfg, "reps": reps, "id_agreement_k100_vs_torch": agree}
    times = {label: [] for label in runs}
    for w in range(reps + 3):
        for label, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if w >= 3:
                times[label].append(a.elapsed_time(b))
    for label, ts in times.items():
        ts.sort()
        out[label + "_ms"] = round(ts[len(ts) // 2], 4)
    for k in KS:
        out[f"wide_over_torch_k{k}"] = round(out[f"wide_k{k}_ms"] / out[f"torch_k{k}_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=240)
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


if __name__ == "__main__":
    main()
