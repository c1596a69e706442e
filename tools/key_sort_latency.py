"""What the device key sort costs against ``torch.sort``, alone and inside the train step.

    (a) the sort alone   torch.sort(keys, stable=True, out=...)  against  srfrd_sort_keys  (eager calls, and one call held in a
                         graph), on the key lists the sorted steps build: the token step's of C2 at K = 16 / 64 / 256 (the clamped
                         input ids, then target + K negatives per position) and the deterministic BCE step's of C2, C4 and C5 (the
                         positive, negative and input ids)
    (b) the step         FusedTrainer(key_sort="torch")  against  key_sort="device":  C2 loss="token_softmax" at K = 64 (two graphs
                         around an eager sort against one graph) and C5 lazy_table=True (one graph either way)

    python tools/key_sort_latency.py [--windows 10] [--steps 20] [--warmup 40] [--out profiles/key_sort_latency.json]

Everything of a comparison lives in ONE process on the same data and is timed interleaved: a round times one window of
``--steps`` back-to-back calls (or steps) of every variant in turn (device events around the window, nothing synchronised inside
it); a variant's figure is the median of its ``--windows`` windows, its spread their maximum minus their minimum.  The sorts' outputs
are compared once, in bits, before anything is timed.  ``condition``: on the 1 689 600-key list the device sort's median is below
torch.sort's by more than the larger of the two spreads - stated as found, nothing is gated on it.

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
             "C5": dict(n_items=1_000_000, L=200, B=512)}
D = 50
CONDITION_KEYS = 1_689_600


def _model(n_items, L):
    import torch
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(n_items, L, D, 0.5, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _window(fn, steps):
    """us per call over `steps` back-to-back calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def _interleaved(variants, windows, steps, warmup):
    """{name: fn} -> {name: {median_us, min_us, max_us, spread_us}}"""
    import torch
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {v: [] for v in variants}
    for _ in range(windows):
        for v, fn in variants.items():
            us[v].append(_window(fn, steps))
    return {v: {"median_us": round(statistics.median(x), 2), "min_us": round(min(x), 2), "max_us": round(max(x), 2),
                "spread_us": round(max(x) - min(x), 2)} for v, x in us.items()}


def _key_lists():
    """name -> (keys on the device, key_max): the lists the sorted steps build, from the synthetic batch of each workload"""
    import torch
    import srfrd_amd
    out = {}
    w = WORKLOADS["C2"]
    b = srfrd_amd.synthetic_batch(w["n_items"], w["L"], w["B"], seed=1, device="cuda")[1:]
    for K in (16, 64, 256):
        neg = srfrd_amd.sample_token_negatives(w["n_items"], b[2], K, generator=torch.Generator("cuda").manual_seed(40))[0]
        head = torch.cat([b[2].unsqueeze(-1), neg], dim=-1).reshape(-1)
        out[f"C2 token K={K}"] = (torch.cat([b[0].reshape(-1).clamp(0, w["n_items"]), head]).contiguous(), w["n_items"])
    for name, w in WORKLOADS.items():
        b = srfrd_amd.synthetic_batch(w["n_items"], w["L"], w["B"], seed=1, device="cuda")[1:]
        out[f"{name} deterministic BCE"] = (torch.stack((b[2], b[4], b[0])).reshape(-1).contiguous(), w["n_items"])
    return out


def measure_sort(name, keys, key_max, windows, steps, warmup):
    import torch
    from srfrd_amd._lib import call, query
    n = keys.numel()
    ws = torch.empty(query("srfrd_sort_keys_workspace_bytes", n=n, key_max=key_max), device="cuda", dtype=torch.uint8)
    out_t = (torch.empty_like(keys), torch.empty_like(keys))
    out_d = (torch.empty_like(keys), torch.empty_like(keys))
    args = dict(keys=keys, n=n, key_max=key_max, sorted_keys=out_d[0], order=out_d[1], workspace=ws, ws_bytes=ws.numel())

    def by_torch():
        torch.sort(keys, stable=True, out=out_t)

    def by_device():
        call("srfrd_sort_keys", **args)

    by_torch()
    by_device()
    torch.cuda.synchronize()
    assert torch.equal(out_t[0], out_d[0]) and torch.equal(out_t[1], out_d[1]), f"{name}: the two sorts differ"
    g = torch.cuda.CUDAGraph()                           # (only the device sort: torch's must not be captured over 2^20 keys)
    with torch.cuda.graph(g):
        by_device()
    res = _interleaved({"torch_sort": by_torch, "device_sort": by_device, "device_sort_in_graph": g.replay}, windows, steps, warmup)
    bits = int(key_max + 2).bit_length()
    return {"list": name, "n_keys": n, "key_max": key_max, "pad_share": round(float((keys == 0).float().mean()), 4),
            "passes": -(-bits // 8), **res}


def measure_step(name, n_items, L, B, kw, windows, steps, warmup):
    import torch
    import srfrd_amd
    packed = srfrd_amd.synthetic_batch(n_items, L, B, seed=1, device="cuda", packed=True)[1]
    trainers = {}
    for sort in ("torch", "device"):
        tr = srfrd_amd.FusedTrainer(_model(n_items, L), B, L, key_sort=sort, **kw)
        tr.ids_ring[0].copy_(packed)
        if tr.token:
            tr.ids_ring[0][4:].zero_()                   # (what step() leaves there: the token step reads no negative-id plane)
            neg, lq = srfrd_amd.sample_token_negatives(n_items, packed[2], tr.K, generator=torch.Generator("cuda").manual_seed(40))
            tr.neg_ring[0].copy_(neg)
            tr.log_q_ring[0].copy_(lq)
        trainers[sort] = tr
    res = _interleaved({s: (lambda t=t: t.step_slot(0)) for s, t in trainers.items()}, windows, steps, warmup)
    losses = {s: float(t.loss) for s, t in trainers.items()}
    assert losses["torch"] == losses["device"] and abs(losses["torch"]) < 1e6, losses       # (same bits, step for step)
    out = {"step": name, "n_items": n_items, "L": L, "B": B, "n_keys": trainers["device"].n_keys,
           "graph_form": {s: t.graph_form for s, t in trainers.items()},
           "stages": {s: [kind for kind, _, _ in t._program] for s, t in trainers.items()}, **res,
           "device_minus_torch_us": round(res["device"]["median_us"] - res["torch"]["median_us"], 2)}
    del trainers, tr
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tools/key_sort_latency.py measures on the GPU: none found")
    res = {"method": f"median of {a.windows} windows of {a.steps} back-to-back calls (steps) per variant, variants interleaved, after "
                     f"{a.warmup} warm-up calls each; device events; spread = max - min of the windows", "d_item": D,
           "sorts": [], "steps": []}
    for name, (keys, key_max) in _key_lists().items():
        res["sorts"].append(measure_sort(name, keys, key_max, a.windows, a.steps, a.warmup))
        print(json.dumps(res["sorts"][-1]), flush=True)
    c2, c5 = WORKLOADS["C2"], WORKLOADS["C5"]
    for name, w, kw in (("C2 token_softmax K=64", c2, dict(loss="token_softmax", num_negatives=64)),
                        ("C5 lazy_table", c5, dict(lazy_table=True))):
        res["steps"].append(measure_step(name, w["n_items"], w["L"], w["B"], kw, a.windows, a.steps, a.warmup))
        print(json.dumps(res["steps"][-1]), flush=True)
    big = next(s for s in res["sorts"] if s["n_keys"] == CONDITION_KEYS)
    gap = big["torch_sort"]["median_us"] - big["device_sort"]["median_us"]
    spread = max(big["torch_sort"]["spread_us"], big["device_sort"]["spread_us"])
    res["condition"] = {"list": big["list"], "torch_minus_device_us": round(gap, 2), "larger_spread_us": spread, "holds": gap > spread}
    print(json.dumps(res["condition"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
