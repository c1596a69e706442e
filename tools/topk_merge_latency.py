"""Latency of the merge of sorted top-k lists (srfrd::topk_merge_runs) and of the sharded ranking at k > 64 and within filters.

    python tools/topk_merge_latency.py [--reps 15] [--out profiles/topk_merge_latency.json]

One MI355X, B = 512.  Configuration "merge" (the kernel alone, inputs resident):
  runs_S{S}_k{k}       (a) srfrd::topk_merge_runs on S sorted runs of k slots, (S, k) in (8, 64), (8, 100), (8, 1024), (2, 1024),
                       (16, 1024): every user merges (path 0, asserted)
  sort_S{S}_k{k}       (b) the same lists with the first two slots of run 0 exchanged for every user: every user takes the full
                       sort (path 1, asserted)
  narrow_S8_k64        (c) srfrd::topk_merge on the (B, 512) concatenation
  torch_S{S}_k{k}      (d) torch on the concatenation: a stable sort on id, a stable descending sort on value, a slice
Configurations "C5" / "C5_bf16" (1 M items, L = 200, fp32 table / bf16 shadow), end to end, encoder pass included in both:
  whole_k{100,1024}[_allow]     model.topk
  sharded_k{100,1024}[_allow]   ShardedRanker(n_shards=8).topk; _allow: a density-0.5 filter
Protocol: all variants of a configuration interleaved in one process - every window times each variant once, in order - and
the figure of a variant is the median over ``--reps`` windows after three warm-up windows, CUDA events.  Every configuration
runs in a fresh child process with its own time limit; a child that fails or hangs ends the run.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 512
CELLS = ((8, 64), (8, 100), (8, 1024), (2, 1024), (16, 1024))
CONFIGS = {"merge": None, "C5": dict(I=1_000_000, L=200, bf16=False), "C5_bf16": dict(I=1_000_000, L=200, bf16=True)}


def _median_ms(runs, reps):
    import torch
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
    out = {}
    for label, ts in times.items():
        ts.sort()
        out[label + "_ms"] = round(ts[len(ts) // 2], 4)
    return out


def sorted_runs(S, k, seed):
    """(S, B, k) lists sorted by the order law: distinct ids per user, standard-normal values"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    ids = torch.argsort(torch.rand(B, S * k, device="cuda", generator=g), dim=1).view(B, S, k)
    val = torch.randn(B, S, k, device="cuda", generator=g)
    ids, perm = ids.sort(dim=2, stable=True)
    val = val.gather(2, perm)
    val, perm = val.sort(dim=2, descending=True, stable=True)
    ids = ids.gather(2, perm)
    return ids.permute(1, 0, 2).contiguous(), val.permute(1, 0, 2).contiguous()


def merge_child(reps: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd  # noqa: F401

    def baseline(ci, cv, k):
        ci, perm = ci.sort(dim=1, stable=True)
        cv, perm = cv.gather(1, perm).sort(dim=1, descending=True, stable=True)
        return ci.gather(1, perm)[:, :k], cv[:, :k]

    runs, out = {}, {"config": "merge", "B": B, "reps": reps}
    for S, k in CELLS:
        idx, val = sorted_runs(S, k, 1000 * S + k)
        bad_i, bad_v = idx.clone(), val.clone()
        bad_i[0, :, [0, 1]], bad_v[0, :, [0, 1]] = idx[0][:, [1, 0]], val[0][:, [1, 0]]
        cat_i, cat_v = (t.permute(1, 0, 2).reshape(B, S * k).contiguous() for t in (idx, val))
        # every variant gives the same list, and each takes the path its label says, before anything is timed
        mi, mv, path = torch.ops.srfrd.topk_merge_runs(idx, val, k)
        si, sv, spath = torch.ops.srfrd.topk_merge_runs(bad_i, bad_v, k)
        ti, tv = baseline(cat_i, cat_v, k)
        assert int(path.sum()) == 0 and int(spath.sum()) == B, (S, k, int(path.sum()), int(spath.sum()))
        assert torch.equal(mi, si) and torch.equal(mv, sv) and torch.equal(mi, ti) and torch.equal(mv, tv), (S, k)
        runs[f"runs_S{S}_k{k}"] = lambda a=idx, b=val, k=k: torch.ops.srfrd.topk_merge_runs(a, b, k)
        runs[f"sort_S{S}_k{k}"] = lambda a=bad_i, b=bad_v, k=k: torch.ops.srfrd.topk_merge_runs(a, b, k)
        runs[f"torch_S{S}_k{k}"] = lambda a=cat_i, b=cat_v, k=k: baseline(a, b, k)
        if (S, k) == (8, 64):
            ni, nv = torch.ops.srfrd.topk_merge(cat_i, cat_v, k)
            assert torch.equal(mi, ni) and torch.equal(mv, nv)
            runs["narrow_S8_k64"] = lambda a=cat_i, b=cat_v: torch.ops.srfrd.topk_merge(a, b, 64)
    out.update(_median_ms(runs, reps))
    for S, k in CELLS:
        out[f"runs_over_sort_S{S}_k{k}"] = round(out[f"runs_S{S}_k{k}_ms"] / out[f"sort_S{S}_k{k}_ms"], 3)
        out[f"runs_over_torch_S{S}_k{k}"] = round(out[f"runs_S{S}_k{k}_ms"] / out[f"torch_S{S}_k{k}_ms"], 3)
    out["runs_over_narrow_S8_k64"] = round(out["runs_S8_k64_ms"] / out["narrow_S8_k64_ms"], 3)
    return out


def e2e_child(name: str, reps: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    cfg = CONFIGS[name]
    I, L = cfg["I"], cfg["L"]
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    m = m.cuda().eval()
    if cfg["bf16"]:
        m.use_bf16_table()
    _, seq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda")
    filt = m.item_filter(torch.rand(I + 1, generator=torch.Generator().manual_seed(5)) < 0.5)
    r = srfrd_amd.ShardedRanker(m, n_shards=8)
    runs, out = {}, {"config": name, **cfg, "B": B, "n_shards": 8, "reps": reps}
    for k in (100, 1024):
        for tag, kw in (("", {}), ("_allow", dict(allow=filt))):
            a, b = r.topk(None, seq, None, k=k, **kw), m.topk(None, seq, None, k=k, **kw)
            out[f"same_bits_k{k}{tag}"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
            runs[f"whole_k{k}{tag}"] = lambda k=k, kw=kw: m.topk(None, seq, None, k=k, **kw)
            runs[f"sharded_k{k}{tag}"] = lambda k=k, kw=kw: r.topk(None, seq, None, k=k, **kw)
    out.update(_median_ms(runs, reps))
    for k in (100, 1024):
        for tag in ("", "_allow"):
            out[f"sharded_over_whole_k{k}{tag}"] = round(out[f"sharded_k{k}{tag}_ms"] / out[f"whole_k{k}{tag}_ms"], 3)
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
        print(json.dumps(merge_child(a.reps) if a.child == "merge" else e2e_child(a.child, a.reps)))
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
