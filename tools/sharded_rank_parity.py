#!/usr/bin/env python3
"""One-shard-per-rank full-catalog ranking == unsharded ranking (srfrd_amd/ranker.py), N ranks.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29519 \\
        tools/sharded_rank_parity.py [--backend nccl|gloo] [--kind SASRec|SRFRN] [--k K] [--allow]

Every rank holds different users; ShardedRanker all-gathers their last hidden states, ranks all users against the rank's
own rows, all-gathers the (users, k) lists and merges.  Each rank compares its result with model.topk() over the whole
catalog (bit-equal indices and values).  One JSON line on rank 0; exit code 0 = parity.

--k K (default 10): k > 64 takes the wide route - per-shard srfrd_logits_topk_wide, the lists exchanged by all-to-all (a rank
receives its own users' lists only) and merged as sorted runs.  --allow: a two-group random item filter, the same on every rank,
with each user's group drawn by a rank-dependent seed (the filtered route at any k).  With either option the ranks also compare
ShardedRanker.target_rank with model.target_rank (equal counts); without options the run is what it always was.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default=None)
    ap.add_argument("--kind", default="SRFRN", choices=["SASRec", "SRFRN"])
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--allow", action="store_true")
    args = ap.parse_args()
    world, rank, local = int(os.environ["WORLD_SIZE"]), int(os.environ["RANK"]), int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist
    n_dev = torch.cuda.device_count()
    backend = args.backend or ("nccl" if n_dev >= world else "gloo")
    dev = torch.device("cuda", local % max(n_dev, 1))
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)
    import srfrd_amd
    I, L, B, k = 20011, 30, 19, args.k or 10
    extended = args.k is not None or args.allow
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, dev) if args.kind == "SASRec" else srfrd_amd.SRFRN(I, L, 45, 5, 0.0, 2, 1, dev)
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    with torch.no_grad():
        w = m._item_param()
        w[[10000, 10006, 19000]] = w[5].clone()              # exact ties across the shard boundary
    m = m.to(dev).eval()
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=3, rank=rank, device=dev)
    r = srfrd_amd.ShardedRanker(m)
    assert r.world == world and r.n_shards == world
    filt = {}
    if args.allow:
        g = torch.Generator().manual_seed(17)                        # the same bitmap on every rank
        mask = torch.rand(2, I + 1, generator=g) < torch.tensor([[0.5], [0.1]])
        groups = torch.randint(0, 2, (B,), generator=torch.Generator().manual_seed(100 + rank))
        filt = dict(allow=m.item_filter(mask), allow_group=groups.to(dev))
    idx, val = r.topk(None, seq, rsq, k=k, **filt)
    wi, wv = m.topk(None, seq, rsq, k=k, **filt)
    ok = bool(torch.equal(idx, wi) and torch.equal(val, wv))
    if extended:
        targets = torch.randint(1, I + 1, (B,), generator=torch.Generator().manual_seed(200 + rank)).to(dev)
        sharded = r.target_rank(None, seq, rsq, targets, **filt)      # (collectives: every rank calls it, whatever `ok` says)
        ok = bool(torch.equal(sharded, m.target_rank(None, seq, rsq, targets, **filt))) and ok
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN) if backend != "nccl" else None
    if backend == "nccl":
        f = flag.to(dev)
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        flag = f.cpu()
    if rank == 0:
        print(json.dumps({"backend": backend, "world": world, "kind": args.kind, "items": I, "users_per_rank": B, "k": k,
                          "allow": bool(args.allow), "target_rank": extended,
                          "shards": r.shards, "ok": bool(int(flag.item()) == 1)}), flush=True)
    dist.barrier()
    dist.destroy_process_group()
    sys.exit(0 if int(flag.item()) == 1 else 1)


if __name__ == "__main__":
    main()
