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

k > 64 (``srfrd_logits_topk_wide`` per shard) and item filters (``allow=``: ``srfrd_logits_topk_allow`` per shard at any k, the
whole bitmap passed - it is indexed by absolute id) take a second pair of mechanisms: the shard lists are
sorted runs and ``srfrd_topk_merge_runs`` merges them as such, up to 16 384 slots, from the (shards, B, k) stack as it lies;
data parallel, a rank sends each peer only that peer's users (all-to-all) instead of all-gathering every list to every rank.
The unfiltered k <= 64 path is the one above, launch for launch.
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


MERGE_RUNS_CAP = 16384          # slots one srfrd_topk_merge_runs launch holds: pow2ceil(lists) * pow2ceil(list length)


def _pow2ceil(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


def topk_merge_runs(cand_idx: torch.Tensor, cand_val: torch.Tensor, k: int):
    """(n_lists, B, list_len) lists, each sorted by the order law (value desc, id asc, empty -1 / -inf slots last) ->
    (idx int64 (B,k), val (B,k), path int32 (B,)) (srfrd::topk_merge_runs): k up to TOPK_WIDE_MAX, pow2ceil(n_lists) *
    pow2ceil(list_len) <= 16 384.  The tensors' strides are read: any view with innermost stride 1 merges without a copy.
    ``path[b]`` is 0 where user b's lists were merged as runs, 1 where one of them was out of order and everything was sorted
    (the result is exact either way)."""
    if cand_idx.device.type != "cuda":
        raise RuntimeError("topk_merge_runs runs on the ROCm GPU only")
    idx, val, path = torch.ops.srfrd.topk_merge_runs(cand_idx, cand_val, k)
    return idx, val, path


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

    def _check_args(self, what, k, allow, allow_group):
        """what ``model.topk`` refuses, and the one refusal of the sharded form - all before the first ranking launch"""
        from . import _lib
        if not 1 <= k <= _lib.TOPK_WIDE_MAX:
            raise ValueError(f"{what}: k = {k} is outside 1..srfrd_amd.TOPK_WIDE_MAX ({_lib.TOPK_WIDE_MAX})")
        if allow is None and allow_group is not None:
            raise ValueError(f"{what}: allow_group needs allow")
        n_lists = self.world if self.dist_on else sum(1 for lo, hi in self.shards if hi > lo)
        if (allow is not None or k > 64) and _pow2ceil(n_lists) * _pow2ceil(k) > MERGE_RUNS_CAP:
            raise ValueError(f"{what}: {n_lists} shard lists of k = {k} do not fit one merge: pow2ceil(shards) * pow2ceil(k) = "
                             f"{_pow2ceil(n_lists) * _pow2ceil(k)} exceeds the {MERGE_RUNS_CAP} slots of srfrd_topk_merge_runs "
                             "(use fewer shards or a smaller k)")

    def _rank_shard_wide(self, h_last, ulab, lo, hi, k, exclude_pad, excl, allow):
        """one shard's lists on the wide (k > 64) or, ``allow`` = (words, group), the filtered route"""
        from . import ops
        xargs = excl if excl is not None else (None, None, 0)
        head = (h_last.unsqueeze(1), ulab, ops.register_model(self.model), lo, hi, k, bool(exclude_pad), *xargs)
        if allow is not None:
            return torch.ops.srfrd.logits_topk_allow(*head, *allow)
        return torch.ops.srfrd.logits_topk_wide(*head)

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
    def topk(self, user_ids, input_ids, fake_ids, k: int = 10, exclude_pad: bool = True, check_batch: bool = True, exclude=None,
             *, allow=None, allow_group=None):
        """-> (indices int64 (B,k), scores (B,k)) of this rank's users over the WHOLE catalog, k in 1..TOPK_WIDE_MAX.  An index
        is -1 (score -inf) where fewer than k items are rankable.  ``check_batch`` (data parallel): verify that every rank passed
        the same batch size (one 8-byte all-gather + host read per call; pass False in a loop whose batches are known to be
        equal).  ``exclude``: per-user items never to return, as in the model's ``topk``.
        ``allow`` / ``allow_group``: an ``ItemFilter`` and each user's row of it, as in the model's ``topk``.  Data parallel,
        every rank must pass the same filter: ``check_batch`` also compares its group count and its number of allowed ids across
        the ranks (one more small all-gather) and raises on every rank if they differ; that the bitmaps agree beyond that is the
        caller's contract.  With a filter or k > 64, pow2ceil(shards) * pow2ceil(k) must not exceed 16 384 (ValueError)."""
        self._check_args("topk", k, allow, allow_group)
        return self.topk_hidden(*self._users(input_ids, fake_ids, exclude), k=k, exclude_pad=exclude_pad, check_batch=check_batch,
                                allow=allow, allow_group=allow_group)

    @torch.no_grad()
    def topk_hidden(self, h_last, ulab=None, excl=None, k: int = 10, exclude_pad: bool = True, check_batch: bool = True, *,
                    allow=None, allow_group=None):
        """``topk`` from the users' last-position states themselves: ``h_last`` (B, d_out) fp32, ``ulab`` the int64 (B,) user
        labels of SRFRN (else None), ``excl`` an ``ops.excl_csr`` triple or None.  What ``topk`` calls after its encoder pass;
        also the entry for states computed elsewhere."""
        B = h_last.shape[0]
        self._check_args("topk", k, allow, allow_group)
        if allow is not None or k > 64:
            filt = None if allow is None else self.model._allow_args(allow, allow_group, B, h_last.device, "topk")
            return self._topk_wide(h_last, ulab, excl, k, exclude_pad, check_batch, allow, filt)
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

    def _topk_wide(self, h_last, ulab, excl, k, exclude_pad, check_batch, allow, filt):
        """the wide (k > 64) and the filtered (``filt`` = (words, group)) routes: per-shard lists, merged as sorted runs"""
        B = h_last.shape[0]
        if not self.dist_on:
            lists = [self._rank_shard_wide(h_last, ulab, lo, hi, k, exclude_pad, excl, filt) for lo, hi in self.shards if hi > lo]
            return topk_merge_runs(torch.stack([i for i, _ in lists]), torch.stack([v for _, v in lists]), k)[:2]
        # ---- one shard per rank: rank every rank's users against the own rows, then send each peer its own users' lists only
        self._check_batch(B, h_last.device, check_batch)
        if filt is not None:
            self._check_filter(allow, h_last.device, check_batch)
            filt = (filt[0], self._gather_group(filt[1], B))
        h_all, lab_all = self._gather_users(h_last, ulab)
        lo, hi = self.shards[self.rank]
        excl_all = self._gather_excl(excl, B, h_last.device) if excl is not None else None
        idx, val = self._rank_shard_wide(h_all, lab_all, lo, hi, k, exclude_pad, excl_all, filt)     # (world * B, k)
        ci, cv = _all_to_all(idx, self.group), _all_to_all(val, self.group)   # rows [r B, (r + 1) B): this rank's users on shard r
        return topk_merge_runs(ci.view(self.world, B, k), cv.view(self.world, B, k), k)[:2]

    @torch.no_grad()
    def target_rank(self, user_ids, input_ids, fake_ids, targets, exclude=None, exclude_pad: bool = True, check_batch: bool = True,
                    *, allow=None, allow_group=None):
        """-> int32 (B,) full-catalog ranks of ``targets`` for this rank's users (as the model's ``target_rank``): the shards'
        strictly-greater counts summed - one after the other on this GPU, or one shard per rank with the counts all-reduced.
        ``allow`` / ``allow_group``: as in ``topk`` - only allowed items are counted (``srfrd_target_rank_allow`` per shard:
        ranks over disjoint item ranges add up); a disallowed target is still ranked."""
        from . import ops
        m = self.model
        if allow is None and allow_group is not None:
            raise ValueError("target_rank: allow_group needs allow")
        h_last, ulab, excl = self._users(input_ids, fake_ids, exclude)
        B = h_last.shape[0]
        tg = torch.as_tensor(targets).to(device=h_last.device, dtype=torch.int64).reshape(-1).contiguous()
        if tg.numel() != B:
            raise ValueError("targets must hold one item id per user")
        key = ops.register_model(m)
        xargs = excl if excl is not None else (None, None, 0)
        filt = None if allow is None else m._allow_args(allow, allow_group, B, h_last.device, "target_rank")

        def count(h, lab, t, lo, hi, x, f):
            if f is not None:
                return torch.ops.srfrd.target_rank_allow(h.unsqueeze(1), lab, t, key, lo, hi, bool(exclude_pad), *x, *f)
            return torch.ops.srfrd.target_rank(h.unsqueeze(1), lab, t, key, lo, hi, bool(exclude_pad), *x)

        if not self.dist_on:
            rank = torch.zeros(B, device=h_last.device, dtype=torch.int32)
            for lo, hi in self.shards:
                if hi > lo:
                    rank += count(h_last, ulab, tg, lo, hi, xargs, filt)
            return rank
        self._check_batch(B, h_last.device, check_batch)
        if filt is not None:
            self._check_filter(allow, h_last.device, check_batch)
            filt = (filt[0], self._gather_group(filt[1], B))
        h_all, lab_all = self._gather_users(h_last, ulab)
        t_all = torch.empty(self.world * B, device=h_last.device, dtype=torch.int64)
        _all_gather(t_all, tg, self.group)
        xall = self._gather_excl(excl, B, h_last.device) if excl is not None else (None, None, 0)
        lo, hi = self.shards[self.rank]
        if hi > lo:
            part = count(h_all, lab_all, t_all, lo, hi, xall, filt)
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

    def _check_filter(self, allow, device, check_batch):
        if not check_batch:
            return
        # every rank ranks every rank's users: a rank with another filter would return other items for the same users
        mine = torch.tensor([allow.n_groups, int(allow.counts.sum())], device=device, dtype=torch.int64)
        seen = torch.empty(self.world * 2, device=device, dtype=torch.int64)
        _all_gather(seen, mine, self.group)
        seen = seen.view(self.world, 2).tolist()
        if any(row != seen[0] for row in seen):
            raise ValueError(f"ShardedRanker: ranks passed different item filters (groups, allowed ids) = {seen}; every rank must "
                             "hold the same ItemFilter")

    def _gather_group(self, group, B):
        """``allow_group`` of all world x B users, as ``ulab`` is gathered (None stays None: every user reads row 0)"""
        if group is None:
            return None
        g_all = torch.empty(self.world * B, device=group.device, dtype=torch.int64)
        _all_gather(g_all, group, self.group)
        return g_all

    def _gather_users(self, h_last, ulab):
        B = h_last.shape[0]
        h_all = torch.empty(self.world * B, h_last.shape[1], device=h_last.device, dtype=torch.float32)
        _all_gather(h_all, h_last, self.group)
        lab_all = None
        if ulab is not None:
            lab_all = torch.empty(self.world * B, device=h_last.device, dtype=torch.int64)
            _all_gather(lab_all, ulab, self.group)
        return h_all, lab_all


def _all_to_all(part: torch.Tensor, group):
    """part (world * n, ...) -> out of the same shape: rows [r n, (r + 1) n) of out are rows [rank n, (rank + 1) n) of rank r's
    `part`.  RCCL natively, through the host on gloo"""
    part = part.contiguous()
    if dist.get_backend(group) == "nccl":
        out = torch.empty_like(part)
        dist.all_to_all_single(out, part, group=group)
        return out
    cpu = part.detach().cpu()
    out = torch.empty_like(cpu)
    dist.all_to_all_single(out, cpu, group=group)
    return out.to(part.device)


def _all_gather(out: torch.Tensor, part: torch.Tensor, group):
    """out (world * n ...) <- concatenation of every rank's `part`; RCCL natively, through the host on gloo"""
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(out, part.contiguous(), group=group)
    else:
        world = dist.get_world_size(group)
        parts = [torch.empty_like(part, device="cpu") for _ in range(world)]
        dist.all_gather(parts, part.detach().cpu().contiguous(), group=group)
        out.copy_(torch.cat([p.reshape(-1) for p in parts]).view_as(out))
