#!/usr/bin/env python3
"""Measured agreement of every encoder gradient with the fp64 oracle (GPU box) -> profiles/grad_fp64_errors.json.

    python tools/grad_fp64_report.py [--out profiles/grad_fp64_errors.json] [--modes encoder | head] [--cases depth | ID ...]
    python tools/grad_fp64_report.py --wave [--cases ID ...]   # tests/test_gpu_wave_fp64.py -> profiles/wave_fp64_errors.json
    python tools/grad_fp64_report.py --scan OUT.json  # CPU only, once per kind of machine the suite runs on, then
    python tools/grad_fp64_report.py --pick A.json B.json      # ... the batch-seed table of tests/grad_refs.py

Runs what tests/test_gpu_grad_fp64.py runs (its run_autograd / run_fused) and what tests/test_gpu_head_grad_fp64.py runs (its
run_head: the first step of the four catalog losses, modes "head-LOSS...") and records per case, mode and tensor (one array
per line, in the order of `tensors`): e32 (the fp32 oracle's row error against the fp64 oracle), the bound, the
device's row error, and the former metric max|g - g_oracle32|.  --modes: only that half, the other half's entries of an
existing --out file kept.  Exit code 1 if a tensor misses its bound.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _setenv(changed):
    def setenv(name, value):
        changed.setdefault(name, os.environ.get(name))
        os.environ[name] = value
    return setenv


def _one_thread():
    import torch
    torch.set_num_threads(1)


def _num(x):
    return float(f"{x:.2g}")


def _record(figs, names, shared):
    """one run -> arrays in the order of `names`; e32 and bound only where no earlier run of the case has the same reference"""
    out = {} if shared else {"e32": [_num(figs[k]["e32"]) for k in names], "bound": [_num(figs[k]["bound"]) for k in names]}
    if shared:
        out["e32_and_bound_as"] = shared
    out["err"] = [_num(figs[k]["err"]) for k in names]
    out["old"] = [_num(figs[k]["old"]) for k in names]
    kb = [f["kbias"] / f["kbias_limit"] for f in figs.values() if "kbias" in f]
    if kb:
        out["kbias_of_limit"] = _num(max(kb))
    out["zero_leaks"] = sum(f["zero_leaks"] for f in figs.values())
    return out


def _dump(report, f):
    """json with one array per line"""
    f.write("{\n")
    f.write(f' "metric": {json.dumps(report["metric"])},\n "tensors": {{\n')
    f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(report["tensors"].items())))
    f.write("\n },\n \"cases\": {\n")
    cases = []
    for cid, modes in report["cases"].items():
        runs = ",\n".join(f"   {json.dumps(m)}: " + (json.dumps(r) if not isinstance(r, dict) else
                          "{\n" + ",\n".join(f"    {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items()) + "}")
                          for m, r in modes.items())
        cases.append(f"  {json.dumps(cid)}: {{\n{runs}\n  }}")
    f.write(",\n".join(cases))
    f.write("\n }\n}\n")


def selected_cases(G, ids):
    """--cases: the cases of grad_refs.ALL_CASES with these ids ("depth": grad_refs.DEPTH); all of them without the option"""
    if not ids:
        return list(G.ALL_CASES)
    want = {c.id for c in G.DEPTH} if ids == ["depth"] else set(ids)
    assert want <= set(G.BY_ID), sorted(want - set(G.BY_ID))
    return [c for c in G.ALL_CASES if c.id in want]


def wave(out, ids):
    """--wave: what tests/test_gpu_wave_fp64.py runs (batches of more sequences than workgroups) -> profiles/wave_fp64_errors.json:
    per case the forward's differing elements (0 expected) and, per run and tensor, the worst row's error"""
    from tests import grad_refs as G
    from tests import test_gpu_wave_fp64 as T
    from tests import wave_refs as W
    chosen = [c for c in W.CASES if not ids or c.id in ids]
    report, tensors, missed, differing = {}, {}, 0, 0
    for c in chosen:
        runs = [("masks", lambda c, env: T.run_masks(c, env)[0]), ("autograd", T.run_autograd)]
        for det in (True, False):
            name = "fused-" + ("deterministic" if det else "atomics")
            runs.append((name, lambda c, env, det=det: T.run_fused(c, det, env)))
            if c.id in W.TRAIN_KERNEL_IDS:
                runs.append((name + "-two-launches", lambda c, env, det=det: T.run_fused(c, det, env, train_launch=False)))
        kind = c.kind if c.blocks == 2 else f"{c.kind}-b{c.blocks}"
        entry = report.setdefault(G.case_ids([c])[0], {"kind": kind})
        first = None
        for mode, fn in [(m, None) for m in ("eval", "last", "train", "masks-forward")] + runs:
            changed = {}
            try:
                got = T.run_forward_bits(c, mode.split("-")[0], _setenv(changed)) if fn is None else fn(c, _setenv(changed))
            finally:
                for name, old in changed.items():
                    os.environ.pop(name, None) if old is None else os.environ.__setitem__(name, old)
            if fn is None:
                entry.setdefault("forward_differing_elements", {})[mode] = sum(got.values())
                differing += sum(got.values())
                continue
            figs, figs2, copies = got if isinstance(got, tuple) else (got, None, None)
            names = tensors.setdefault(kind, sorted(figs))
            if first is None:           # (B, the copies, e32_tiled and the bounds are the case's: with its first run)
                ref = W.reference(c.id, T._n_cu())
                entry["B"], entry["copies"] = ref.B, ref.k
                entry["exceptions"] = {n: [_num(ref.e32[n]), _num(ref.bounds[n])] for n in W.exceptions_of(ref)}
                entry["e32_tiled"] = [_num(ref.e32[k]) for k in names]
            entry[mode] = _record(figs, names, first)
            first = first or mode
            for k in ("e32", "bound", "old", "e32_and_bound_as"):
                entry[mode].pop(k, None)
            if figs2 is not None:
                w = max(figs2, key=lambda k: figs2[k]["err"] / figs2[k]["bound"])
                entry[mode]["second_moment_worst"] = [w, _num(figs2[w]["err"]), _num(figs2[w]["bound"])]
                entry[mode]["copies_differing_elements"] = sum(copies.values())
                differing += sum(copies.values())
            both = list(figs.values()) + list((figs2 or {}).values())
            bad = sum(bool(G.failures(f)) for f in both)
            missed += bad
            worst = max(f["err"] / f["bound"] for f in both)
            print(f"{c.id:5s} {mode:34s} worst err / bound {worst:.3f}" + (f"   <-- {bad} tensors miss" if bad else ""), flush=True)
        print(f"{c.id:5s} forward: differing elements {entry['forward_differing_elements']}; exceptions {entry['exceptions']}",
              flush=True)
    with open(out, "w") as f:
        _dump({"metric": "tests/wave_refs.py: grad_refs.row_errors (worst row) against the BASE batch's fp64 gradient, bound 1e-4, "
                         "for the tensors of `exceptions` [e32_tiled, bound = min(4 e32_tiled, 1 / (2 B))]; arrays follow "
                         "`tensors` of the case's kind; masks: one tiled launch at dropout 0.5 against the fp64 sum of the "
                         "untiled launches; second_moment_worst = [tensor, row error of g^2, twice the bound]; "
                         "forward_differing_elements / copies_differing_elements: elements of a per-sequence output that "
                         "differ from the untiled launch / from the first copy (0 expected)",
               "tensors": tensors, "cases": report}, f)
    print(f"{missed} tensors miss their bound, {differing} forward elements differ; wrote {out}")
    return 1 if missed or differing else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wave", action="store_true", help="the batches of more sequences than workgroups "
                    "(tests/test_gpu_wave_fp64.py) -> profiles/wave_fp64_errors.json unless --out says otherwise")
    ap.add_argument("--out", help="default: profiles/grad_fp64_errors.json (--wave: profiles/wave_fp64_errors.json)")
    ap.add_argument("--modes", choices=["all", "encoder", "head"], default="all")
    ap.add_argument("--cases", nargs="+", metavar="ID", help="only these cases of grad_refs.ALL_CASES (\"depth\": grad_refs.DEPTH), "
                    "encoder modes only; every other entry of an existing --out file is kept")
    ap.add_argument("--scan", metavar="OUT", help="CPU only: worst e32 and ReLU margin of every job's candidate seeds, here")
    ap.add_argument("--count", type=int, default=48)
    ap.add_argument("--jobs", nargs="*", metavar="CASE/MODE", help="--scan: these only (head: every head/LOSS job)")
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--pick", nargs="+", metavar="SCAN", help="grad_refs.SEEDS from one --scan file per kind of machine")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "wave_fp64_errors.json" if a.wave else "grad_fp64_errors.json")
    from tests import grad_refs as G
    if a.wave:
        return wave(a.out, a.cases)
    if a.scan:
        import multiprocessing as mp
        jobs = [(c.id, m, a.count) for c in G.ALL_CASES for m in ("autograd", "fused")]
        jobs += [(j.cid, "head/" + j.loss, a.count) for j in G.HEAD_JOBS if not j.l2]
        jobs = [j for j in jobs if not a.jobs or f"{j[0]}/{j[1]}" in a.jobs or (a.jobs == ["head"] and j[1].startswith("head/"))]
        # (one thread per worker: e32 is a one-thread figure anyway, and workers x threads would oversubscribe the machine)
        with mp.get_context("spawn").Pool(a.workers, initializer=_one_thread) as pool:
            rows = pool.map(G.scan_seeds, jobs, chunksize=1)
        with open(a.scan, "w") as f:
            json.dump({f"{cid}/{m}": r for (cid, m, _), r in zip(jobs, rows)}, f)
        return 0
    if a.pick:
        scans = [json.load(open(p)) for p in a.pick]
        for key in scans[0]:
            seed, found = G.pick_seed([s[key] for s in scans])
            worst = max(next(r[1] for r in s[key] if r[0] == seed) for s in scans)
            print(f"{key}: {seed}   worst-machine e32 {worst:.3e}" + ("" if found else "   <-- no seed with headroom: OVER_CAP"))
        return 0
    from tests import test_gpu_grad_fp64 as T
    from tests import test_gpu_head_grad_fp64 as H
    runs = []           # (case, mode, the first mode that shares its reference, run)
    chosen = selected_cases(G, a.cases)
    if a.cases:
        a.modes = "encoder"
    for c in chosen if a.modes != "head" else []:
        runs.append((c, "autograd", "autograd", lambda c, env: (T.run_autograd(c, env), None)))
        for det in (True, False):
            name = "fused-" + ("deterministic" if det else "atomics")
            runs.append((c, name, "fused", lambda c, env, det=det: T.run_fused(c, det, env)))
            if c.id in G.TRAIN_KERNEL_IDS:
                runs.append((c, name + "-two-launches", "fused",
                             lambda c, env, det=det: T.run_fused(c, det, env, train_launch=False)))
            if c.id == G.L2_ID:
                runs.append((c, name + "-l2_emb", "fused-l2_emb", lambda c, env, det=det: T.run_fused(c, det, env, l2=G.L2_EMB)))
    for (j, det), rid in zip(H.RUNS, H.RUN_IDS) if a.modes != "encoder" else []:
        name = "head-" + rid.split("-", 1)[1].replace("-l2", "-l2_emb")
        runs.append((G.BY_ID[j.cid], name, "head-" + G.head_id(j), lambda c, env, j=j, det=det: H.run_head(j, det, env)))
    report, missed, tensors, first = {}, 0, {}, {}
    if a.modes != "all" and os.path.exists(a.out):
        kept = json.load(open(a.out))
        tensors = kept["tensors"]
        report = {cid: {m: r for m, r in modes.items() if m == "kind" or m.startswith("head-") != (a.modes == "head")
                        or (a.cases and cid not in G.case_ids(chosen))}
                  for cid, modes in kept["cases"].items()}
    for c, mode, ref, fn in runs:
        changed = {}
        try:
            figs, figs2 = fn(c, _setenv(changed))
        finally:
            for name, old in changed.items():
                os.environ.pop(name, None) if old is None else os.environ.__setitem__(name, old)
        kind = c.kind if c.blocks == 2 else f"{c.kind}-b{c.blocks}"      # (another depth has another tensor list)
        names = tensors.setdefault(kind, sorted(figs))
        shared = first.get((c.id, ref))
        first.setdefault((c.id, ref), mode)
        entry = report.setdefault(G.case_ids([c])[0], {"kind": kind})
        entry[mode] = _record(figs, names, shared)
        if figs2 is not None:       # (the same gradient squared, under twice the bound: the worst tensor only)
            w = max(figs2, key=lambda k: figs2[k]["err"] / figs2[k]["bound"])
            entry[mode]["second_moment_worst"] = [w, _num(figs2[w]["err"]), _num(figs2[w]["bound"])]
        both = list(figs.values()) + list((figs2 or {}).values())
        bad = sum(bool(G.failures(f)) for f in both)
        missed += bad
        worst = max(f["err"] / f["bound"] for f in both)
        print(f"{c.id:3s} {mode:34s} worst err / bound {worst:.3f}" + (f"   <-- {bad} tensors miss" if bad else ""), flush=True)
    with open(a.out, "w") as f:
        _dump({"metric": "tests/grad_refs.py: row_errors, bound(e32) = max(64 e32, 2e-5), clamped at 1e-4 for the OVER_CAP jobs; "
                         "arrays follow `tensors` of the case's kind; old = max|g - g_oracle32|; second_moment_worst = "
                         "[tensor, row error of g^2, twice the bound]; kbias_of_limit is absent under l2_emb, where the K "
                         "slice is an ordinary part of its row; modes head-LOSS...: the first FusedTrainer(loss=LOSS) step against "
                         "grad_refs.head_grads (tests/test_gpu_head_grad_fp64.py)",
               "tensors": tensors, "cases": report}, f)
    print(f"{missed} tensors miss their bound; wrote {a.out}")
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
