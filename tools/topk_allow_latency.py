"""Latency of the filtered full-catalog top-k (srfrd::logits_topk_allow) beside the unfiltered wide call and beside
materialise, masked_fill, torch.topk.

    python tools/topk_allow_latency.py [--reps 15] [--out profiles/topk_allow_latency.json]

Configurations: SASRec hidden 50, B = 512, the C2 (50k items) and C5 (1M items) catalogs, fp32 table and bf16 shadow.  Per
configuration, the ranking op only (the last-position encoder state is computed once, outside the timed region), k = 10, 100
and 1024, one filter row shared by the batch:
  allow_k{k}_{filter}  srfrd::logits_topk_allow; filters: d100 / d50 / d5 - random masks of density 1.0, 0.5 and 0.05 - and
                       block5, a contiguous allowed block of 5 % of the catalog
  torch_k{k}_{filter}  hidden[:, -1] @ table.T (the (B, n_items) logits in memory; a bf16 matmul widened to fp32 on the bf16
                       configurations), masked_fill with the filter, torch.topk
  wide_k{k}            srfrd::logits_topk_wide, unfiltered
  allow_k{100,1024}_d50_fallback   the filtered op with user 0's hidden state zeroed: all of its allowed scores tie, its
                       candidates overflow, its list comes from the fallback workgroup
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
KS = (10, 100, 1024)
FILTERS = ("d100", "d50", "d5", "block5")


def masks(n_rows: int):
    import torch
    g = torch.Generator().manual_seed(3)
    u = torch.rand(n_rows, generator=g)
    out = {"d100": torch.ones(n_rows, dtype=torch.bool), "d50": u < 0.5, "d5": u < 0.05, "block5": torch.zeros(n_rows, dtype=torch.bool)}
    out["block5"][n_rows // 3: n_rows // 3 + n_rows // 20] = True
    return out


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
    host = masks(hi)
    filt = {f: m.item_filter(host[f]) for f in FILTERS}
    off = {}
    for f in FILTERS:                                   # what masked_fill removes: the disallowed ids and the pad row
        o = ~host[f]
        o[0] = True
        off[f] = o.cuda()

    def baseline(k, f):
        return torch.topk((last @ table.T).float().masked_fill_(off[f], float("-inf")), k, dim=1)

    allow = lambda hid, k, f: torch.ops.srfrd.logits_topk_allow(hid, None, key, 0, hi, k, True, None, None, 0, filt[f].words, None)
    runs = {}
    for k in KS:
        runs[f"wide_k{k}"] = lambda k=k: torch.ops.srfrd.logits_topk_wide(h, None, key, 0, hi, k, True, None, None, 0)
        for f in FILTERS:
            runs[f"allow_k{k}_{f}"] = lambda k=k, f=f: allow(h, k, f)
            runs[f"torch_k{k}_{f}"] = lambda k=k, f=f: baseline(k, f)
    for k in (100, 1024):
        runs[f"allow_k{k}_d50_fallback"] = lambda k=k: allow(h_tied, k, "d50")
    # the lists agree before anything is timed (ids; near ties may swap between the two arithmetics)
    ai, _ = allow(h, 100, "d50")
    agree = float((ai == baseline(100, "d50").indices).float().mean()) if not cfg["bf16"] else None
    assert bool(host["d50"][ai.cpu()].all()), "a disallowed id in a filtered list"
    fi, fv = allow(h_tied, 100, "d50")
    first = torch.nonzero(host["d50"][1:]).reshape(-1)[:100] + 1
    assert bool((fi[0].cpu() == first).all()) and bool((fv[0] == 0).all()), "fallback list"
    out = {"config": name, **cfg, "reps": reps, "id_agreement_k100_d50_vs_torch": agree,
           "allowed": {f: int(filt[f].counts[0]) for f in FILTERS}}
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
        for f in FILTERS:
            out[f"allow_over_torch_k{k}_{f}"] = round(out[f"allow_k{k}_{f}_ms"] / out[f"torch_k{k}_{f}_ms"], 3)
        out[f"allow_d100_over_wide_k{k}"] = round(out[f"allow_k{k}_d100_ms"] / out[f"wide_k{k}_ms"], 3)
    for k in (100, 1024):
        out[f"fallback_user_k{k}_ms"] = round(out[f"allow_k{k}_d50_fallback_ms"] - out[f"allow_k{k}_d50_ms"], 4)
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
