#!/usr/bin/env python3
"""Measured agreement of every encoder forward output with the fp64 oracle (GPU box) -> profiles/fwd_fp64_errors.json.

    python tools/fwd_fp64_report.py [--out profiles/fwd_fp64_errors.json] [--cases depth | ID ...]
    python tools/fwd_fp64_report.py --scan OUT.json   # CPU only, once per kind of machine the suite runs on, then
    python tools/fwd_fp64_report.py --pick A.json B.json       # ... the entries of tests/fwd_refs.FWD_SEEDS / FWD_OVER_CAP

Runs what tests/test_gpu_fwd_fp64.py runs (its run_eval / run_last / run_train / run_wave) and records per case, mode and
output (arrays in the order of `outputs`): e32 (the fp32 oracle's row error against the fp64 oracle), the bound, the device's
row error and the former metric max|x - x_oracle32|; for the train mode also the loss's relative error and its bound.  Exit
code 1 if an output misses its bound.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.grad_fp64_report import _num, _one_thread, _setenv, selected_cases  # noqa: E402


def _record(figs, names):
    return {k: [_num(figs[n][k]) for n in names] for k in ("e32", "bound", "err", "old")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_fp64_errors.json"))
    ap.add_argument("--cases", nargs="+", metavar="ID", help="only these cases of fwd_refs.ALL_CASES (\"depth\": grad_refs.DEPTH), "
                    "without the wave batch; every other entry of an existing --out file is kept")
    ap.add_argument("--scan", metavar="OUT", help="CPU only: worst e32 of every job's candidate seeds, here")
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--pick", nargs="+", metavar="SCAN", help="the seed of every job from one --scan file per kind of machine")
    a = ap.parse_args()
    from tests import fwd_refs as R
    from tests import grad_refs as G
    if a.scan:
        import multiprocessing as mp
        jobs = [(c.id, m, a.count) for c in selected_cases(G, a.cases) for m in R.MODES]
        with mp.get_context("spawn").Pool(a.workers, initializer=_one_thread) as pool:
            rows = pool.map(R.scan_seeds, jobs, chunksize=1)
        with open(a.scan, "w") as f:
            json.dump({f"{cid}/{m}": r for (cid, m, _), r in zip(jobs, rows)}, f)
        return 0
    if a.pick:
        scans = [json.load(open(p)) for p in a.pick]
        for key in scans[0]:
            seed, found = R.pick_seed([s[key] for s in scans])
            worst = max(next(r[1] for r in s[key] if r[0] == seed) for s in scans)
            first = scans[0][key][0][0]
            print(f"{key}: {seed}" + ("" if seed == first else "   <-- not the gradient suite's: FWD_SEEDS")
                  + f"   worst-machine e32 {worst:.3e}" + ("" if found else "   <-- no seed with headroom: FWD_OVER_CAP"))
        return 0
    from tests import test_gpu_fwd_fp64 as T
    runs = [(G.case_ids([c])[0], mode, lambda env, c=c, fn=fn: fn(c, env))
            for c in selected_cases(G, a.cases) for mode, fn in (("eval", T.run_eval), ("last", T.run_last), ("train", T.run_train))]
    runs += [] if a.cases else [("wave-" + "-".join(f"{k}{R.WAVE[k]}" for k in ("kind", "B", "L")), mode, lambda env, mode=mode: T.run_wave(mode, env))
             for mode in ("eval", "last")]
    report, missed = {}, 0
    if a.cases and os.path.exists(a.out):
        report = {cid: modes for cid, modes in json.load(open(a.out))["cases"].items() if cid not in {r[0] for r in runs}}
    for cid, mode, fn in runs:
        changed = {}
        try:
            out = fn(_setenv(changed))
        finally:
            for name, old in changed.items():
                os.environ.pop(name, None) if old is None else os.environ.__setitem__(name, old)
        figs, loss = (out[0], out[1:]) if isinstance(out, tuple) else (out, None)
        entry = _record(figs, R.OUTPUTS[mode])
        if loss:
            entry["loss_err"], entry["loss_bound"] = _num(loss[0]), _num(loss[1])
        report.setdefault(cid, {})[mode] = entry
        bad = sum(not R.holds(f) for f in figs.values())
        missed += bad
        worst = max(f["err"] / f["bound"] for f in figs.values())
        print(f"{cid:40s} {mode:6s} worst err / bound {worst:.3f}" + (f"   <-- {bad} outputs miss" if bad else ""), flush=True)
    with open(a.out, "w") as f:
        f.write("{\n")
        f.write(' "metric": ' + json.dumps(
            "tests/fwd_refs.py: row_errors_inf, bound(e32) = max(16 e32, 4e-6); arrays follow `outputs` of the mode; "
            "old = max|x - x_oracle32|; loss_err = |loss - loss64| / loss64 of the BCE loss of the device's logits, "
            "loss_bound = max(16 e32, 1e-6); wave-...: fwd_refs.WAVE") + ",\n")
        f.write(' "outputs": ' + json.dumps(R.OUTPUTS) + ',\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(cid)}: {{\n" + ",\n".join(f"   {json.dumps(m)}: {json.dumps(r)}" for m, r in modes.items())
                           + "\n  }" for cid, modes in report.items()))
        f.write("\n }\n}\n")
    print(f"{missed} outputs miss their bound; wrote {a.out}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
