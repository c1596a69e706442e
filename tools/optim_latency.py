"""What the optimizer options of the fused train step cost: the C2 step - SASRec, 50 k items, seq_len 50,
B = 512, hidden 50, dropout 0.2, loss "bce", one HIP graph per step - with the options off, with gradient-norm clipping,
decoupled weight decay and a learning-rate schedule on one at a time, and with all three.

    python tools/optim_latency.py [--rounds 15] [--steps 200] [--out profiles/optim_options_latency.json]

The variants live in ONE process, each a FusedTrainer of its own on the same synthetic batch, and are timed interleaved: a
round times ``--steps`` back-to-back steps of every variant in turn (device events around the window, no synchronisation
inside it: the rate of a training loop), ``--rounds`` rounds, and a variant's figure is the median of its rounds.  "off" is
in the rotation twice ("off" and "off_again"): two trainers that issue the very same launches, so their difference is the
noise of the measurement, reported beside the costs.

``srfrd_grad_norm`` is also timed alone, ``--steps`` back-to-back calls between two events: over the C2 gradient (4 n_flat
bytes, 10 MB: it stays in the Infinity Cache from call to call, so this is the call's latency, not a memory rate) and over a
512 MiB vector that no cache holds (its achieved bytes per second, against the 6.3 TB/s a float4 copy attains on this chip).

Reads nothing outside the repository; exits non-zero without a GPU.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, L, B, D = 50_000, 50, 512, 50
HBM_ATTAINABLE = 6.3e12          # bytes / s: measured float4 copy rate of the MI355X
SCHED = dict(lr_schedule="cosine", warmup_steps=100, total_steps=100_000, final_lr_ratio=0.1)
VARIANTS = {"off": {}, "clip": dict(max_grad_norm=1.0), "decay": dict(weight_decay=0.01), "schedule": SCHED,
            "all": dict(SCHED, max_grad_norm=1.0, weight_decay=0.01), "off_again": {}}


def _model():
    import torch
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, D, 0.2, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    return m.cuda().train()


def _window(fn, steps):
    """ms per call over `steps` back-to-back calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def _grad_norm_alone(n, steps, rounds):
    """us per srfrd_grad_norm call over n floats, and the bytes per second that is"""
    import torch
    from srfrd_amd import _lib
    from srfrd_amd._lib import ptr
    g = torch.randn(n, device="cuda")
    part = torch.zeros(_lib.GRAD_NORM_PARTIALS, device="cuda", dtype=torch.float64)
    out = torch.zeros(2, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = _lib.lib().srfrd_grad_norm(ptr(g), n, None, 1.0, ptr(part), ptr(out), st)
        assert rc == 0, rc

    _window(call, 20)
    ms = statistics.median(_window(call, steps) for _ in range(rounds))
    want = float(torch.sqrt((g.double() ** 2).sum()))
    assert abs(float(out[0]) - want) <= 2.0 ** -23 * want
    return {"n": n, "bytes": 4 * n, "us_per_call": round(ms * 1e3, 3), "bytes_per_s": round(4 * n / (ms * 1e-3), 0),
            "share_of_attainable_hbm": round(4 * n / (ms * 1e-3) / HBM_ATTAINABLE, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import srfrd_amd
    if not torch.cuda.is_available():
        sys.exit("tools/optim_latency.py measures on the GPU: none found")
    packed = srfrd_amd.synthetic_batch(I, L, B, seed=1, device="cuda", packed=True)[1]
    trainers = {}
    for name, kw in VARIANTS.items():
        tr = srfrd_amd.FusedTrainer(_model(), B, L, **kw)
        tr.ids_ring[0].copy_(packed)
        for _ in range(a.warmup):
            tr.step_slot(0)
        trainers[name] = tr
    torch.cuda.synchronize()
    ms = {name: [] for name in trainers}
    for _ in range(a.rounds):
        for name, tr in trainers.items():
            ms[name].append(_window(lambda: tr.step_slot(0), a.steps))
    med = {name: statistics.median(v) for name, v in ms.items()}
    res = {"workload": {"n_items": I, "B": B, "L": L, "loss": "bce", "n_flat": trainers["off"].n_flat},
           "rounds": a.rounds, "steps_per_window": a.steps,
           "step_us": {name: round(1e3 * med[name], 2) for name in med},
           "step_us_min_max": {name: [round(1e3 * min(v), 2), round(1e3 * max(v), 2)] for name, v in ms.items()},
           "noise_us_off_vs_off_again": round(1e3 * (med["off_again"] - med["off"]), 2),
           "cost_us": {name: round(1e3 * (med[name] - med["off"]), 2) for name in ("clip", "decay", "schedule", "all")},
           "grad_norm_of_all": round(float(trainers["all"].grad_norm), 5), "next_lr_of_all": float(trainers["all"].next_lr),
           "losses": {name: round(float(tr.loss), 5) for name, tr in trainers.items()}}
    n_flat = trainers["off"].n_flat
    del trainers
    res["grad_norm_c2"] = _grad_norm_alone(n_flat, a.steps, a.rounds)
    res["grad_norm_512MiB"] = _grad_norm_alone(1 << 27, 50, a.rounds)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
