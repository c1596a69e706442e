"""What lazy Adam of the item table costs and saves per train step: the fused BCE step, one HIP graph per
step, as

    lazy           FusedTrainer(lazy_table=True)      sorted keys -> srfrd_table_reduce_adam, dense Adam over the dense part only
    deterministic  FusedTrainer(deterministic=True)   sorted keys -> srfrd_table_reduce, dense Adam over the whole flat vector
    atomic         FusedTrainer()                     float atomics, dense Adam over the whole flat vector

at the C2, C4 and C5 workloads of bench.py (50 k / 200 k / 1 M items at seq_len 50 / 100 / 200, B = 512, SASRec hidden 50) and
at one 4 M-item catalog with C5's batch.

    python tools/lazy_adam_latency.py [--windows 10] [--steps 20] [--warmup 60] [--out profiles/lazy_adam_latency.json]

The three trainers of a workload live in ONE process on the same synthetic batch and are timed interleaved: a round times one
window of ``--steps`` back-to-back graph replays of every variant in turn (device events around the window, nothing
synchronised inside it), and a variant's figure is the median of its ``--windows`` windows, with their minimum and maximum
beside it.  The three are different optimizers after the first step, so nothing is compared but time; the number of DISTINCT
item rows the batch names - what the lazy step's table work is proportional to - is recorded per workload.

Reads nothing outside the repository; exits non-zero without a GPU.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"C2": dict(n_items=50_000, L=50, B=512), "C4": dict(n_items=200_000, L=100, B=512),
             "C5": dict(n_items=1_000_000, L=200, B=512), "C5_4M_items": dict(n_items=4_000_000, L=200, B=512)}
VARIANTS = {"lazy": dict(lazy_table=True), "deterministic": dict(deterministic=True), "atomic": {}}
D = 50


def _model(n_items, L):
    import torch
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(n_items, L, D, 0.5, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _window(tr, steps):
    """ms per step over `steps` back-to-back steps"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        tr.step_slot(0)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(name, n_items, L, B, windows, steps, warmup):
    import torch
    import srfrd_amd
    packed = srfrd_amd.synthetic_batch(n_items, L, B, seed=1, device="cuda", packed=True)[1]
    ids = torch.cat([packed[0].reshape(-1), packed[2].reshape(-1), packed[4].reshape(-1)])
    keys = int(ids.numel())
    distinct = int(torch.unique(ids[ids != 0]).numel())
    trainers = {}
    for variant, kw in VARIANTS.items():
        tr = srfrd_amd.FusedTrainer(_model(n_items, L), B, L, **kw)
        tr.ids_ring[0].copy_(packed)
        for _ in range(warmup):
            tr.step_slot(0)
        assert tr.captured and tr.lazy_table == (variant == "lazy")
        trainers[variant] = tr
    torch.cuda.synchronize()
    ms = {v: [] for v in trainers}
    for _ in range(windows):
        for v, tr in trainers.items():
            ms[v].append(_window(tr, steps))
    med = {v: statistics.median(x) for v, x in ms.items()}
    losses = {v: float(tr.loss) for v, tr in trainers.items()}
    assert all(x == x and abs(x) < 1e6 for x in losses.values()), losses
    lazy = trainers["lazy"]
    res = {"workload": name, "n_items": n_items, "L": L, "B": B, "n_flat": lazy.n_flat, "n_table_pad": lazy.n_tab,
           "row_keys_per_batch": keys, "distinct_touched_rows": distinct,
           "touched_share_of_table": round(distinct / (n_items + 1), 6),
           "step_us": {v: round(1e3 * med[v], 2) for v in med},
           "step_us_min_max": {v: [round(1e3 * min(x), 2), round(1e3 * max(x), 2)] for v, x in ms.items()},
           "lazy_minus_deterministic_us": round(1e3 * (med["lazy"] - med["deterministic"]), 2),
           "lazy_minus_atomic_us": round(1e3 * (med["lazy"] - med["atomic"]), 2),
           "loss_after_timing": {v: round(x, 5) for v, x in losses.items()}}
    del trainers, lazy, tr
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/lazy_adam_latency.py measures on the GPU: none found")
    res = {"method": f"median of {a.windows} windows of {a.steps} back-to-back graph replays per variant, variants interleaved, "
                     f"after {a.warmup} warm-up steps each; device events", "d_item": D, "workloads": []}
    for name in a.workloads.split(","):
        w = WORKLOADS[name]
        res["workloads"].append(measure(name, w["n_items"], w["L"], w["B"], a.windows, a.steps, a.warmup))
        print(json.dumps(res["workloads"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
