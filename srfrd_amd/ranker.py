"""Row-sharded full-catalog ranking (BASELINE configs[4]: 1M items, row-sharded embedding table).

``predict`` over the whole catalog (reference SRFR_model.py:144-152 / :241-259 / :532-540 / :668-681 with every item as a
candidate) is the one part of the path whose cost grows with the catalog: 2 B I d flops, and a (B, I) logits matrix the
reference would materialise.  Here the item rows are split into contiguous shards; each shard is ranked by
``srfrd_logits_topk`` over its own ``[lo, hi)`` (logits never reach HBM) and the per-shard top-k lists are merged by
``srfrd_topk_merge`` into the order one unsharded ranking returns (value desc, item id asc - ties across shard boundaries
included).  The merged list equals the unsharded one bit for bit when both are scored by the same arithmetic; a call whose
candidate lists overflow (include/srfrd_hip.h, ``srfrd_logits_topk``) is re-ranked on the fp32 matrix cores, and then the
ids agree wherever two scores differ by more than an fp32 rounding and the values agree to that rounding.

* one process (``n_shards`` given, no process group): the shards are ranked one after the other on this GPU - bounds the
  ranking workspace at 1M+ items and is what the single-GPU tests exercise;
* data parallel (one process per GPU): every rank owns shard ``rank`` of the rows.  The last-position hidden states of ALL
  ranks' users are all-gathered (B x d_out floats per rank: tiny), every rank ranks all users against its rows only, the
  (users, k) lists are all-gathered and each rank merges the lists of its own users - SURVEY 8e's
  "all-gather h_last -> per-shard top-k -> merge".  Only rows ``[lo, hi)`` of the table are read on a rank, so the same
  code serves a table whose other rows are not resident.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def row_shards(n_rows: int, n_shards: int):
    """contiguous [lo, hi) row ranges, sizes differing by at most one"""
    base, extra = divmod(n_rows, n_shards)
    out, lo = [], 0
    for s in range(n_shards):
        hi = lo + base + (1 if s < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


def topk_merge(cand_idx: torch.Tensor, cand_val: torch.Tensor, k: int):
    """(B, n_cand) candidate lists -> (idx int64 (B,k), val (B,k)) in stable descending order (srfrd::topk_merge)."""
    if cand_idx.device.type != "cuda":
        raise RuntimeError("topk_merge runs on the ROCm GPU only")
    idx, val = torch.ops.srfrd.topk_merge(cand_idx, cand_val, k)
    return idx, val


class ShardedRanker:
    def __init__(self, model, n_shards: int | None = None, process_group=None):
        self.model, self.group = model, process_group
        from .exchange import exchange_forced
        self.dist_on = dist.is_available() and dist.is_initialized() and (dist.get_world_size(process_group) > 1 or exchange_forced())
        self.world = dist.get_world_size(process_group) if self.dist_on else 1
        self.rank = dist.get_rank(process_group) if self.dist_on else 0
        self.n_shards = self.world if self.dist_on else int(n_shards or 1)
        if self.dist_on and n_shards not in (None, self.world):
            raise ValueError("with a process group the number of shards is the world size")
        self.shards = row_shards(model.layout.n_items + 1, self.n_shards)

    def _rank_shard(self, h_last, ulab, lo, hi, k, exclude_pad, excl=None):
        from . import ops
        if excl is None:
            idx, val = torch.ops.srfrd.logits_topk(h_last.unsqueeze(1), ulab, ops.register_model(self.model), lo, hi, k,
                                                   bool(exclude_pad))
        else:
            idx, val = torch.ops.srfrd.logits_topk_excl(h_last.unsqueeze(1), ulab, ops.register_model(self.model), lo, hi, k,
                                                        bool(exclude_pad), *excl)
        return idx, val

    def _gather_excl(self, excl, B, device):
        """data parallel: every rank's exclusion CSR -> the CSR of all world x B users (rows padded to a common width with
        -1, an id outside every range, then re-packed)"""
        xp, xi, mr = excl
        width = torch.tensor([mr], device=device, dtype=torch.int64)
        w_all = torch.empty(self.world, device=device, dtype=torch.int64)
        _all_gather(w_all, width, self.group)
        M = max(int(w_all.max()), 1)
        lens = (xp[1:] - xp[:-1])
        col = torch.arange(M, device=device)
        src = (xp[:-1, None] + col[None, :]).clamp(max=max(xi.numel() - 1, 0))
        pad = torch.where(col[None, :] < lens[:, None], xi[src].to(torch.int32), torch.full_like(src, -1, dtype=torch.int32))
        pad_all = torch.empty(self.world * B, M, device=device, dtype=torch.int32)
        _all_gather(pad_all, pad.contiguous(), self.group)
        ptr_all = torch.arange(0, self.world * B * M + 1, M, device=device, dtype=torch.int64)
        return ptr_all, pad_all.reshape(-1).contiguous(), M

    def _users(self, input_ids, fake_ids, exclude):
        hidden, ulab, excl = self.model._rank_inputs(input_ids, fake_ids, exclude)
        return hidden[:, 0, :], ulab, (excl if exclude is not None else None)          # (B, d_out)

    @torch.no_grad()
    def topk(self, user_ids, input_ids, fake_ids, k: int = 10, exclude_pad: bool = True, check_batch: bool = True, exclude=None):
        """-> (indices int64 (B,k), scores (B,k)) of this rank's users over the WHOLE catalog.  An index is -1 (score -inf) where
        fewer than k items are rankable.  ``check_batch`` (data parallel): verify that every rank passed the same batch size
        (one 8-byte all-gather + host read per call; pass False in a loop whose batches are known to be equal).
        ``exclude``: per-user items never to return, as in the model's ``topk``."""
        return self.topk_hidden(*self._users(input_ids, fake_ids, exclude), k=k, exclude_pad=exclude_pad, check_batch=check_batch)

    @torch.no_grad()
    def topk_hidden(self, h_last, ulab=None, excl=None, k: int = 10, exclude_pad: bool = True, check_batch: bool = True):
        """``topk`` from the users' last-position states themselves: ``h_last`` (B, d_out) fp32, ``ulab`` the int64 (B,) user
        labels of SRFRN (else None), ``excl`` an ``ops.excl_csr`` triple or None.  What ``topk`` calls after its encoder pass;
        also the entry for states computed elsewhere."""
        B = h_last.shape[0]
        if not self.dist_on:
            lists = [self._rank_shard(h_last, ulab, lo, hi, k, exclude_pad, excl) for lo, hi in self.shards if hi > lo]
            return topk_merge(torch.cat([i for i, _ in lists], 1), torch.cat([v for _, v in lists], 1), k)
        # ---- one shard per rank: gather every rank's users, rank them against the own rows, exchange the lists
        self._check_batch(B, h_last.device, check_batch)
        h_all, lab_all = self._gather_users(h_last, ulab)
        lo, hi = self.shards[self.rank]
        excl_all = self._gather_excl(excl, B, h_last.device) if excl is not None else None
        idx, val = self._rank_shard(h_all, lab_all, lo, hi, k, exclude_pad, excl_all)   # (world * B, k) against the own rows
        idx_all = torch.empty(self.world, self.world * B, k, device=idx.device, dtype=torch.int64)
        val_all = torch.empty(self.world, self.world * B, k, device=idx.device, dtype=torch.float32)
        _all_gather(idx_all, idx, self.group)
        _all_gather(val_all, val, self.group)
        mine = slice(self.rank * B, (self.rank + 1) * B)
        ci = idx_all[:, mine].permute(1, 0, 2).reshape(B, self.world * k)
        cv = val_all[:, mine].permute(1, 0, 2).reshape(B, self.world * k)
        return topk_merge(ci, cv, k)

    @torch.no_grad()
    def target_rank(self, user_ids, input_ids, fake_ids, targets, exclude=None, exclude_pad: bool = True, check_batch: bool = True):
        """-> int32 (B,) full-catalog ranks of ``targets`` for this rank's users (as the model's ``target_rank``): the shards'
        strictly-greater counts summed - one after the other on this GPU, or one shard per rank with the counts all-reduced."""
        from . import ops
        m = self.model
        h_last, ulab, excl = self._users(input_ids, fake_ids, exclude)
        B = h_last.shape[0]
        tg = torch.as_tensor(targets).to(device=h_last.device, dtype=torch.int64).reshape(-1).contiguous()
        if tg.numel() != B:
            raise ValueError("targets must hold one item id per user")
        key = ops.register_model(m)
        xargs = excl if excl is not None else (None, None, 0)
        if not self.dist_on:
            rank = torch.zeros(B, device=h_last.device, dtype=torch.int32)
            for lo, hi in self.shards:
                if hi > lo:
                    rank += torch.ops.srfrd.target_rank(h_last.unsqueeze(1), ulab, tg, key, lo, hi, bool(exclude_pad), *xargs)
            return rank
        self._check_batch(B, h_last.device, check_batch)
        h_all, lab_all = self._gather_users(h_last, ulab)
        t_all = torch.empty(self.world * B, device=h_last.device, dtype=torch.int64)
        _all_gather(t_all, tg, self.group)
        xall = self._gather_excl(excl, B, h_last.device) if excl is not None else (None, None, 0)
        lo, hi = self.shards[self.rank]
        if hi > lo:
            part = torch.ops.srfrd.target_rank(h_all.unsqueeze(1), lab_all, t_all, key, lo, hi, bool(exclude_pad), *xall)
        else:
            part = torch.zeros(self.world * B, device=h_last.device, dtype=torch.int32)
        part = part.to(torch.int64)
        if dist.get_backend(self.group) == "nccl":
            dist.all_reduce(part, group=self.group)
        else:
            cpu = part.cpu()
            dist.all_reduce(cpu, group=self.group)
            part = cpu.to(h_last.device)
        return part[self.rank * B:(self.rank + 1) * B].to(torch.int32)

    def _check_batch(self, B, device, check_batch):
        if not check_batch:
            return
        # every rank must bring the same number of users (the gathers below are sized world x B from the LOCAL B: a ragged
        # last evaluation batch would hang or mis-assign rows) - one tiny all-gather, then a clear error on every rank
        nb = torch.tensor([B], device=device, dtype=torch.int64)
        nb_all = torch.empty(self.world, device=device, dtype=torch.int64)
        _all_gather(nb_all, nb, self.group)
        sizes = nb_all.tolist()
        if any(x != B for x in sizes):
            raise ValueError(f"ShardedRanker: ranks passed different batch sizes {sizes}; pad the last batch to a common size "
                             "(rows of padding ids rank like any other user and can be dropped afterwards)")

    def _gather_users(self, h_last, ulab):
        B = h_last.shape[0]
        h_all = torch.empty(self.world * B, h_last.shape[1], device=h_last.device, dtype=torch.float32)
        _all_gather(h_all, h_last, self.group)
        lab_all = None
        if ulab is not None:
            lab_all = torch.empty(self.world * B, device=h_last.device, dtype=torch.int64)
            _all_gather(lab_all, ulab, self.group)
        return h_all, lab_all


def _all_gather(out: torch.Tensor, part: torch.Tensor, group):
    """out (world * n ...) <- concatenation of every rank's `part`; RCCL natively, through the host on gloo"""
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(out, part.contiguous(), group=group)
    else:
        world = dist.get_world_size(group)
        parts = [torch.empty_like(part, device="cpu") for _ in range(world)]
        dist.all_gather(parts, part.detach().cpu().contiguous(), group=group)
        out.copy_(torch.cat([p.reshape(-1) for p in parts]).view_as(out))
