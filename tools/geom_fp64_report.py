#!/usr/bin/env python3
"""Measured agreement of the generic encoder kernels with the fp64 oracle at the widths and head splits of tests/geom_refs.py
(GPU box) -> profiles/geom_fp64_errors.json.

    python tools/geom_fp64_report.py [--out profiles/geom_fp64_errors.json] [--cases ID ...]
    python tools/geom_fp64_report.py --scan OUT.json [--modes grad | fwd] [--count N] [--jobs CASE/MODE ...] [--sd-seed S]
    python tools/geom_fp64_report.py --pick A.json B.json ...

Without --scan / --pick: runs what tests/test_gpu_geom_fp64.py runs (run_autograd / run_fused of test_gpu_grad_fp64, run_eval /
run_last / run_train of test_gpu_fwd_fp64) and records per job the worst tensor's error as a fraction of its bound, with its
name, e32 and bound; exit code 1 if a tensor misses its bound.

--scan is CPU only, once per kind of machine and BLAS code path the suite runs on (the gradient jobs first: the forward jobs
start from geom_refs.GEOM_SEEDS); --pick prints geom_refs' seed tables from one scan file per machine.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.grad_fp64_report import _num, _one_thread, _setenv  # noqa: E402


def _worst(figs):
    k = max(figs, key=lambda k: figs[k]["err"] / figs[k]["bound"])
    f = figs[k]
    return {"worst": k, "err_of_bound": _num(f["err"] / f["bound"]), "err": _num(f["err"]), "e32": _num(f["e32"]),
            "bound": _num(f["bound"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geom_fp64_errors.json"))
    ap.add_argument("--cases", nargs="+", metavar="ID")
    ap.add_argument("--scan", metavar="OUT", help="CPU only: worst e32 and ReLU margin of every job's candidate seeds, here")
    ap.add_argument("--modes", choices=["grad", "fwd"], default="grad")
    ap.add_argument("--count", type=int, default=200)
    ap.add_argument("--jobs", nargs="*", metavar="CASE/MODE")
    ap.add_argument("--sd-seed", type=int, help="--scan: under this weight seed, not geom_refs'")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--pick", nargs="+", metavar="SCAN")
    a = ap.parse_args()
    from tests import fwd_refs as R
    from tests import geom_refs as W
    from tests import grad_refs as G
    if a.scan:
        import multiprocessing as mp
        jobs = [(cid, m, a.count, a.sd_seed) for cid, m in (W.GRAD_JOBS if a.modes == "grad" else W.FWD_JOBS)]
        jobs = [j for j in jobs if not a.jobs or f"{j[0]}/{j[1]}" in a.jobs]
        with mp.get_context("spawn").Pool(a.workers, initializer=_one_thread) as pool:
            rows = pool.map(W.scan_job, jobs, chunksize=1)
        with open(a.scan, "w") as f:
            json.dump({f"{j[0]}/{j[1]}": r for j, r in zip(jobs, rows)}, f)
        return 0
    if a.pick:
        scans = [json.load(open(p)) for p in a.pick]
        for key in scans[0]:
            cid, mode = key.split("/")
            fwd = mode in R.MODES
            seed, found = (R if fwd else G).pick_seed([W.forward_rows(cid, mode, s[key]) if fwd else s[key] for s in scans])
            at = [next(r[1] for r in s[key] if r[0] == seed) for s in scans]
            print(f"{key}: {seed}   e32 " + " ".join(f"{e:.3e}" for e in at) + ("" if found else "   <-- no seed with headroom: over the cap"))
        return 0
    from tests import test_gpu_fwd_fp64 as TF
    from tests import test_gpu_grad_fp64 as TG
    report, missed = {}, 0
    for c in [c for c in W.CASES if not a.cases or c.id in a.cases]:
        runs = [("autograd", lambda env: (TG.run_autograd(c, env),))]
        runs += [("fused-" + ("deterministic" if det else "atomics"), lambda env, det=det: TG.run_fused(c, det, env)) for det in (True, False)]
        runs += [("eval", lambda env: (TF.run_eval(c, env),)), ("last", lambda env: (TF.run_last(c, env),)),
                 ("train", lambda env: TF.run_train(c, env)[:1])]
        entry = report.setdefault(W.case_ids([c])[0], {})
        for mode, fn in runs:
            changed = {}
            try:
                out = fn(_setenv(changed))
            finally:
                for name, old in changed.items():
                    os.environ.pop(name, None) if old is None else os.environ.__setitem__(name, old)
            entry[mode] = _worst(out[0])
            fails = lambda f: bool(G.failures(f)) if "zero_leaks" in f else not R.holds(f)
            bad = sum(fails(f) for figs in out for f in figs.values())
            if len(out) == 2:
                entry[mode]["second_moment"] = _worst(out[1])
            missed += bad
            print(f"{c.id:5s} {mode:20s} worst err / bound {entry[mode]['err_of_bound']:.3f} ({entry[mode]['worst']})"
                  + (f"   <-- {bad} tensors miss" if bad else ""), flush=True)
    worst = max(((r["err_of_bound"], cid, m) for cid, modes in report.items() for m, r in modes.items()), default=None)
    with open(a.out, "w") as f:
        f.write("{\n")
        f.write(' "metric": ' + json.dumps(
            "tests/geom_refs.py through the runners of tests/test_gpu_grad_fp64.py (row_errors, bound max(64 e32, 2e-5), clamped at "
            "1e-4 for geom_refs.GEOM_OVER_CAP) and tests/test_gpu_fwd_fp64.py (row_errors_inf, bound max(16 e32, 4e-6)); per job the "
            "tensor or output with the largest err / bound; second_moment: g^2 under twice the bound") + ",\n")
        f.write(' "worst": ' + json.dumps(worst) + ',\n "cases": {\n')
        f.write(",\n".join(f"  {json.dumps(cid)}: {{\n" + ",\n".join(f"   {json.dumps(m)}: {json.dumps(r)}" for m, r in modes.items())
                           + "\n  }" for cid, modes in report.items()))
        f.write("\n }\n}\n")
    print(f"{missed} tensors miss their bound; worst {worst}; wrote {a.out}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
