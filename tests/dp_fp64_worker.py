#!/usr/bin/env python3
"""The rank program of tests/test_gpu_dp_fp64.py: every job of one world size, one FusedTrainer step each.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        tests/dp_fp64_worker.py OUT.pt

Backend gloo, the ranks sharing one GPU, as tools/dp_parity.py runs them.  For each job of tests/dp_refs.jobs_of(N), in order:
the case's switch into the environment, the model from the case's weights (fp32 table), FusedTrainer on B / N sequences with
seed grad_refs.BASE and the job's exchange / scatter / graph / l2_emb; world, mode and the planned kernel names are asserted; ONE
step on rank r's slice [r B / N, (r + 1) B / N) of the case's batch; grad_refs.fused_gradients (a collective in the sharded
form: every rank calls it); the stepped flat parameters of all ranks gathered.  Rank 0 keeps per job g, g2, the loss, the
kernel names and whether the replicas' parameters are the same bits; dp_refs.REPEATED runs a second time and rank 0 keeps whether
the two runs' moments, loss and parameters are the same bits.  No oracle runs here: the parent compares.

Rank 0 writes everything to OUT.pt (torch.save) and prints one JSON status line.  A rank that sees a failure makes all ranks
exit non-zero after the current job; nothing further is started on the GPU.
"""
import datetime
import json
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_job(job, rank, world, dev):
    """one job on this rank -> (g, g2, loss, names, [every rank's stepped flat parameters])"""
    import torch
    import torch.distributed as dist
    import srfrd_amd
    from srfrd_amd import _lib
    from tests import dp_refs as D
    from tests import grad_refs as G
    from tests import test_gpu_bf16_families as F
    from tests.gpu_util import build_model
    cid, w, exchange, det, graph, l2 = job
    assert w == world
    c, cfg, sd, batch = D.inputs(cid)
    for name in _lib.SWITCHES:
        os.environ.pop(name, None)
    if c.switch:
        os.environ[c.switch] = "1"
        assert _lib.env_switches() == _lib.SWITCHES[c.switch]
    else:
        assert _lib.env_switches() == 0
    model = build_model(cfg, {k: v.clone() for k, v in sd.items()}, device=dev).train()
    assert not model.bf16_table
    Bl = c.B // world
    tr = srfrd_amd.FusedTrainer(model, Bl, c.L, seed=G.BASE, exchange=exchange, deterministic=det, use_graph=graph, l2_emb=l2)
    assert tr.world == world and tr.rank == rank and tr.mode == exchange and tr.use_graph == graph, (tr.world, tr.rank, tr.mode)
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    names = F.planned(model.layout, Bl, c.L, "fused", _lib.env_switches(), n_cu, tr.n_scratch, tr.n_scratch)
    assert names == D.local_names(cid, world), (cid, names)
    mine = tuple(x[rank * Bl:(rank + 1) * Bl].to(dev) for x in batch)
    loss = tr.step(None, *mine)
    tr.check()
    loss = float(loss.detach().cpu())
    g, g2 = G.fused_gradients(tr, model)
    flat = model.flat_parameters().detach().cpu().clone()
    every = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(every, flat)
    torch.cuda.synchronize()
    return g, g2, loss, names, every


def main():
    out_path = sys.argv[1]
    world, rank, local = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist
    dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    torch.cuda.set_device(dev)
    # (a rank that left after a failure must not keep the others waiting in a collective for the default half hour)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
    from tests import dp_refs as D
    t0 = time.time()
    jobs = [(j, False) for j in D.jobs_of(world)]
    again = (D.REPEATED[0], world) + D.REPEATED[1:]
    jobs.insert([j for j, _ in jobs].index(again) + 1, (again, True))
    results, error, done = {}, None, 0
    for job, repeat in jobs:
        ok = 1
        try:
            g, g2, loss, names, every = run_job(job, rank, world, dev)
            if rank == 0:
                same = all(torch.equal(every[0], x) for x in every[1:])
                if repeat:
                    first = results[D.job_id(job)]
                    results["repeat"] = {"job": D.job_id(job), "equal_bits": bool(
                        all(torch.equal(first["g"][k], g[k]) and torch.equal(first["g2"][k], g2[k]) for k in g)
                        and first["loss"] == loss and torch.equal(first["flat"], every[0]))}
                else:
                    results[D.job_id(job)] = {"g": g, "g2": g2, "loss": loss, "names": list(names), "replicas_equal": bool(same),
                                              "flat": every[0]}
        except BaseException:                                   # noqa: BLE001 - whatever it is, every rank must stop here
            ok, error = 0, f"rank {rank}, job {D.job_id(job)}:\n{traceback.format_exc()}"
            print(error, file=sys.stderr, flush=True)
        try:
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = int(flag.item())
        except BaseException:                                   # noqa: BLE001 - a peer is gone
            ok = 0
        if not ok:
            error = error or f"rank {rank}: another rank failed at job {D.job_id(job)}"
            break
        done += 1
    if rank == 0:
        if error is None:
            for r in results.values():
                r.pop("flat", None)
            torch.save(results, out_path)
        print(json.dumps({"ok": error is None, "world": world, "jobs": done, "seconds": round(time.time() - t0, 1),
                          "error": error}), flush=True)
    if error is None:
        dist.barrier()
        dist.destroy_process_group()
    sys.exit(0 if error is None else 1)


if __name__ == "__main__":
    main()
