"""Latency of full-catalog ranking with and without per-user exclusion sets, and of the exact target rank.

    python tools/rank_latency.py [--reps 20] [--out profiles/rank_latency.json]

Configurations: C2 (50k items, B = 512, L = 50, fp32 table) and C5 (1M items, B = 512, L = 200, fp32 table and bf16
shadow).  Per configuration: ``topk`` (k = 10), ``topk`` excluding each user's input window ("input": up to L ids), ``topk``
excluding 200 random ids per user, and ``target_rank`` with the input window excluded.  Times cover the ranking op only
(the last-position encoder state is computed once, outside the timed region), median over ``--reps`` launches after
warm-up, CUDA events.  Every configuration runs in a fresh child process with its own time limit.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"C2": dict(I=50_000, L=50, B=512, bf16=False), "C5": dict(I=1_000_000, L=200, B=512, bf16=False),
           "C5_bf16": dict(I=1_000_000, L=200, B=512, bf16=True)}


def child(name: str, reps: int, unmasked_only: bool = False) -> dict:
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
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda")
    m._ensure_flat()
    with torch.no_grad():
        h = m._launch_fwd_last(seq, None)
    key = ops.register_model(m)
    hi = I + 1
    if unmasked_only:
        runs = {"topk": lambda: torch.ops.srfrd.logits_topk(h, None, key, 0, hi, 10, True)}
        return _time(runs, {"config": name, **cfg, "k": 10, "reps": reps}, reps)
    inp = ops.excl_csr("input", seq, B, h.device)
    rnd = torch.randint(1, I + 1, (B, 200), device="cuda")
    r200 = (torch.arange(0, B * 200 + 1, 200, device="cuda", dtype=torch.int64), rnd.reshape(-1).to(torch.int32), 200)
    t = seq[:, -1].clone()
    runs = {
        "topk": lambda: torch.ops.srfrd.logits_topk(h, None, key, 0, hi, 10, True),
        "topk_excl_input": lambda: torch.ops.srfrd.logits_topk_excl(h, None, key, 0, hi, 10, True, *inp),
        "topk_excl_200": lambda: torch.ops.srfrd.logits_topk_excl(h, None, key, 0, hi, 10, True, *r200),
        "target_rank_excl_input": lambda: torch.ops.srfrd.target_rank(h, None, t, key, 0, hi, True, *inp),
    }
    out = _time(runs, {"config": name, **cfg, "k": 10, "reps": reps}, reps)
    out["excl_input_overhead"] = round(out["topk_excl_input_ms"] / out["topk_ms"] - 1.0, 4)
    out["excl_200_overhead"] = round(out["topk_excl_200_ms"] / out["topk_ms"] - 1.0, 4)
    return out


def _time(runs, out, reps):
    import torch
    for label, fn in runs.items():
        for _ in range(3):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--unmasked-only", action="store_true", help="time topk alone (also runs on trees without exclusion sets)")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.reps, a.unmasked_only)))
        return
    results = []
    for name in a.configs.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)]
                               + (["--unmasked-only"] if a.unmasked_only else []),
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
