"""Fused train step: the MI355X counterpart of the inner loop of reference trainer.py:27-41.

    forward -> masked BCE(pos, 1) + BCE(neg, 0) over pos != 0 -> backward -> Adam(lr, betas=(0.9, 0.98))

as five stream-ordered launches on persistent buffers (encoder_fwd, encoder_bwd, reduce_dense [+ loss], adam_step,
pack_weights [+ optimizer-state advance for the next step]; single rank at seq_len 50: encoder_fwd and encoder_bwd are ONE
launch, srfrd_encoder_train_ranked), captured into one HIP graph when no collective sits in the middle.  Differences from the reference
loop, all behaviour-preserving: the loss is never synchronised to the host (``loss`` stays a device scalar), the
``l2_emb * ||p||`` terms (trainer.py:39: one Frobenius norm per parameter tensor) cost two small launches and one pass over
the gradient when l2_emb != 0 and nothing at the reference's 0.0, and dropout masks come from the coordinate hash of csrc/srfrd_rng.h instead of torch's Bernoulli stream.

``lazy_table=True`` (no reference counterpart) swaps the optimizer of the item table for lazy Adam: only the
rows a batch names are stepped (srfrd_table_reduce_adam, from the sorted row keys), the dense Adam tail covers the dense
parameters alone.

Data parallel (no reference counterpart): one process per GPU, the global batch split by sequence,
parameters replicated, dropout masks keyed by the GLOBAL sequence index.  srfrd_amd/exchange.py holds the two forms of
the per-step exchange; both divide by the GLOBAL count of non-pad targets, so N ranks reproduce the single-process
mean-over-all-targets loss of trainer.py:36-38 (not an average of per-rank means):
  "sharded" (default)  fwd -> [16-byte all-reduce of the loss statistics, overlapped with] bwd -> reduce-scatter of the
                       flat gradient -> Adam on this rank's 1/N slice (moments exist for that slice only) -> all-gather
                       of the stepped parameters -> re-pack of the encoder weights;
  "allreduce"          fwd -> bwd -> one all-reduce of [gradient | statistics] -> the full fused Adam tail on every rank.
"""
from __future__ import annotations

import contextlib
import math
import os

import torch
import torch.distributed as dist

import numpy as np

from . import _lib, loss_heads
from ._lib import call, ptr, query
from .exchange import GradExchange, exchange_active, shard_bounds  # noqa: F401  (shard_bounds re-exported)
from .sampler import alias_table, negative_q

LOSSES = ("bce", "sampled_softmax", "softmax", "token_softmax", "gbce")
TOKEN_LOSSES = {"token_softmax": "softmax", "gbce": "gbce"}      # -> the objective of srfrd_tneg_fwd / _bwd


# The longest key list whose stable sort a graph may hold.  Above rocprim's merge_sort_limit (MergeSortLimit = 1024 * 1024 in
# rocprim/device/device_radix_sort_config.hpp; `size <= limit` takes the merge sort) the radix sort clears its histogram and
# look-back states with hipMemsetAsync, a replayed memset node does not reliably zero its buffer on this runtime, and a captured
# sort of 1 689 600 keys faulted the GPU on replay.  A longer list is sorted eagerly, between two graphs.
SORT_CAPTURE_LIMIT = 1 << 20


def sort_key_count(loss: str, deterministic: bool, lazy: bool, B: int, L: int, K: int = 0) -> int:
    """the length of the key list a train step sorts (0: it sorts nothing - the float-atomic scatter)"""
    T = int(B) * int(L)
    if loss in TOKEN_LOSSES:
        return T * (2 + int(K))              # the input ids, then the head's (1 + K) rank-1 rows per position
    if loss == "sampled_softmax":
        return 2 * T + int(K)                # the input ids, then the head's negatives and targets
    if loss == "softmax":
        return T if deterministic else 0     # the input ids
    return 3 * T if deterministic or lazy else 0      # BCE: the positive, negative and input ids


KEY_SORTS = ("torch", "device")


def sort_plan(mode: str, n_keys: int, use_graph: bool = True, device_sort: bool = False):
    """THE decision where a step's key sort runs, from the length of its list: -> (eager_sort, use_graph, reason).  Up to
    SORT_CAPTURE_LIMIT keys the sort is captured with the step.  A longer list on a single rank: ``eager_sort``, step_program's
    two graphs around the sort.  The exchange programs have no such form: there the step runs without graphs, and ``reason``
    (FusedTrainer.graph_capture_error) says so.  ``device_sort`` (``key_sort="device"``: srfrd_sort_keys, kernel launches and
    nothing else - DESIGN section 24): captured at every length, in every mode."""
    if device_sort:
        return False, use_graph, None
    if n_keys <= SORT_CAPTURE_LIMIT or mode == "single":
        return n_keys > SORT_CAPTURE_LIMIT, use_graph, None
    reason = (f"a sort of {n_keys} keys (more than {SORT_CAPTURE_LIMIT}) is not captured, and the {mode!r} exchange program has no "
              "form with an eager sort: the step runs without graphs")
    return False, False, reason if use_graph else None


def step_program(mode: str, token: bool = False, lazy: bool = False, eager_sort: bool = False, device_sort: bool = False):
    """THE order of a train step under exchange ``mode`` ("single" | "allreduce" | "sharded"; ``token``: a loss with K negatives
    per position; ``lazy``: ``lazy_table``, single rank and BCE only; ``eager_sort``: single rank, a key list too long to sort
    inside a graph - sort_plan; ``device_sort``: the key sort is srfrd_sort_keys, captured wherever it stands - the token step
    is then ONE stage, every other program its form without an eager sort): FusedTrainer's eager step, graph capture, replay and
    spin_up all walk this list of stages (kind, per_slot,
    calls) - FusedTrainer methods called in order, with the input slot where per_slot (the pieces of SLOT_FREE, which read no
    input slot: without it).  "graph": they only enqueue stream work,
    so the stage is captured (per slot where per_slot: the kernels' id pointers are baked in).  "eager" / "collective": a host
    action between two graphs - the key sort of a token step (at every size) or of a long list / the
    exchange."""
    G, E, X = "graph", "eager", "collective"
    if lazy and (mode != "single" or token):
        raise ValueError("lazy_table steps on a single rank under loss='bce'")
    if device_sort and eager_sort:
        raise ValueError("eager_sort and device_sort exclude each other: the device sort is captured at every length")
    if mode == "single" and token and device_sort:
        return [(G, True, ("_enqueue_ce_compute", "_sort_keys", "_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))]
    if mode == "single" and token:
        return [(G, True, ("_enqueue_ce_compute",)), (E, False, ("_sort_keys",)),
                (G, False, ("_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))]
    if eager_sort:       # the pieces of `_enqueue_step_compute`, cut at the sort; then the update
        if mode != "single":
            raise ValueError("the exchange programs have no form with an eager sort")
        return [(G, True, ("_enqueue_to_keys",)), (E, False, ("_sort_keys",)),
                (G, False, ("_enqueue_reduce", "_enqueue_lazy_update" if lazy else "_enqueue_update"))]
    if lazy:
        return [(G, True, ("_enqueue_lazy_step",))]
    if mode == "single":
        return [(G, True, ("_enqueue_compute_update",))]
    if mode == "allreduce":
        return [(G, True, ("_enqueue_compute",)), (X, False, ("_all_reduce_grad",)), (G, False, ("_enqueue_update",))]
    # sharded: the 16-byte statistics all-reduce is in flight under the backward; `_scatter_grad` waits for it
    return [(G, True, ("_enqueue_fwd",)), (X, False, ("_start_stats_reduce",)), (G, True, ("_enqueue_bwd",)),
            (X, False, ("_scatter_grad",)), (G, False, ("_enqueue_shard_update",)), (X, False, ("_gather_params",)),
            (G, False, ("_enqueue_shard_finish",))]


# the pieces that read no input slot: a per-slot stage calls them without one (the token step's one stage under the device sort)
SLOT_FREE = frozenset(("_sort_keys", "_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))

# RCCL collectives are stream work: the whole data-parallel step, collectives included, as one graph per slot
ONE_GRAPH = [("graph", True, ("_enqueue_step",))]


def flat_allreduce(flat: torch.Tensor, group=None):
    """SUM all-reduce of the flat gradient vector (RCCL on GPUs, gloo on CPU tests)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    return flat


def _loss_config(model, loss, num_negatives, neg_counts, neg_alpha, process_group, gbce_beta=1.0, tokens=0):
    """The refusals of FusedTrainer's loss arguments, made before anything is allocated; -> q (fp64 numpy (n_items,)) of the
    popularity sampler, or None.  ``tokens``: B L of the step."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES} (got {loss!r})")
    if loss != "sampled_softmax" and neg_counts is not None:
        raise ValueError("neg_counts belongs to loss='sampled_softmax'" + (
            f": under loss={loss!r} the negatives are batch data and their sampler owns the distribution"
            if loss in TOKEN_LOSSES else ""))
    if loss == "bce":
        return None
    q = None
    if loss == "sampled_softmax" or loss in TOKEN_LOSSES:
        if int(num_negatives) < 1:
            raise ValueError(f"num_negatives must be at least 1 (got {num_negatives})")
        if neg_counts is not None:
            q = negative_q(model.layout.n_items, neg_counts, neg_alpha)
    if loss in TOKEN_LOSSES:
        beta = float(gbce_beta)
        if not (beta >= 0.0) or beta == float("inf"):
            raise ValueError(f"gbce_beta must be finite and >= 0 (got {gbce_beta})")
        if loss == "gbce" and model._kind == "SRFRN":
            raise ValueError("objective='gbce' is not built for SRFRN: its logits include the fake slice, which BCE "
                             "(unlike the softmax) is not invariant to")
        # the step's one key list holds T input rows and T (1 + K) rank-1 rows, indexed with 32-bit ints by the reduction
        if int(tokens) * (2 + int(num_negatives)) >= 2 ** 31:
            raise ValueError(f"num_negatives K = {num_negatives}: B L (2 + K) = {int(tokens) * (2 + int(num_negatives))} "
                             f"must stay below 2^31")
    if model.layout.D > _lib.MAX_D:
        raise ValueError(f"loss={loss!r}: the cross-entropy kernels cover hidden width <= {_lib.MAX_D} (got {model.layout.D})")
    if model.bf16_table:
        raise ValueError(f"loss={loss!r} reads the fp32 item table: call model.use_bf16_table(False) first")
    if exchange_active(process_group):
        raise ValueError(f"loss={loss!r} trains on a single rank: the data-parallel step supports loss='bce' only")
    return q


LR_SCHEDULES = tuple(_lib.SCHEDULES)


def lr_at(step: int, lr: float, schedule: str = "constant", warmup_steps: int = 0, total_steps: int | None = None,
          final_lr_ratio: float = 0.0) -> float:
    """The learning rate of the 1-based ``step``: the host mirror, in Python doubles, of the one formula the device evaluates
    (include/srfrd_hip.h, srfrd_step_begin_sched): linear warmup ``step / warmup_steps``, then ``u = min(1, (step - warmup) /
    max(1, total - warmup))`` and "constant": 1, "linear": ``1 - (1 - r) u``, "cosine": ``r + (1 - r) (1 + cos(pi u)) / 2``,
    ``r = final_lr_ratio`` - which the factor keeps past ``total_steps``."""
    if schedule not in _lib.SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {LR_SCHEDULES} (got {schedule!r})")
    if int(step) < 1:
        raise ValueError(f"step counts from 1 (got {step})")
    t, w = float(int(step)), float(int(warmup_steps))
    if t <= w:
        return float(lr) * (t / w)
    if schedule == "constant":
        return float(lr)
    if total_steps is None:
        raise ValueError(f"lr_schedule={schedule!r} decays towards total_steps: give it")
    u = min(1.0, (t - w) / max(1.0, float(int(total_steps) - int(warmup_steps))))
    r = float(final_lr_ratio)
    if schedule == "linear":
        return float(lr) * (1.0 - (1.0 - r) * u)
    return float(lr) * (r + (1.0 - r) * (0.5 * (1.0 + math.cos(math.pi * u))))


def _optim_config(lr, betas, weight_decay=0.0, max_grad_norm=None, lr_schedule="constant", warmup_steps=0, total_steps=None,
                  final_lr_ratio=0.0, process_group=None):
    """The refusals of FusedTrainer's optimizer options, made on the host before anything is allocated; -> (opts, max_norm):
    ``opts`` the ``_lib.OptimOpts`` of the scheduled entry points, or None where every option is neutral (no decay, no
    clipping, a constant rate without warmup) and the step is the plain Adam step, launch for launch; ``max_norm`` a float or
    None."""
    if lr_schedule not in _lib.SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {LR_SCHEDULES} (got {lr_schedule!r})")
    wd = float(weight_decay)
    if not (wd >= 0.0) or wd == float("inf"):
        raise ValueError(f"weight_decay must be finite and >= 0 (got {weight_decay})")
    max_norm = None if max_grad_norm is None else float(max_grad_norm)
    if max_norm is not None and not (max_norm > 0.0):
        raise ValueError(f"max_grad_norm must be > 0, or None for no clipping (got {max_grad_norm})")
    w = int(warmup_steps)
    if w < 0 or w != warmup_steps:
        raise ValueError(f"warmup_steps must be a whole number >= 0 (got {warmup_steps})")
    r = float(final_lr_ratio)
    if not (0.0 <= r <= 1.0):
        raise ValueError(f"final_lr_ratio must lie in [0, 1] (got {final_lr_ratio})")
    decays = lr_schedule != "constant"
    if decays:
        if total_steps is None:
            raise ValueError(f"lr_schedule={lr_schedule!r} decays towards total_steps: give it")
        if int(total_steps) != total_steps or int(total_steps) < w:
            raise ValueError(f"total_steps must be a whole number >= warmup_steps = {w} (got {total_steps})")
    if wd == 0.0 and max_norm is None and not decays and w == 0:
        return None, None
    if exchange_active(process_group):
        raise ValueError("weight_decay / max_grad_norm / lr_schedule / warmup_steps train on a single rank: the sharded step "
                         "advances the optimizer state inside srfrd_pack_weights and owns a slice of the gradient only, so it "
                         "needs a variant of its own and a collective for the norm (DESIGN section 19); the all-reduce form "
                         "waits for the same work")
    opts = _lib.OptimOpts(float(lr), float(betas[0]), float(betas[1]), wd, r, w, int(total_steps) if decays else 0,
                          _lib.SCHEDULES[lr_schedule], 0)
    return opts, max_norm


def _lazy_config(lazy_table, loss="bce", process_group=None, shadow_gather=False, l2_emb=0.0, weight_decay=0.0,
                 max_grad_norm=None) -> bool:
    """The refusals of FusedTrainer's ``lazy_table`` option, made on the host before anything is allocated; -> the option as a
    bool.  Lazy Adam steps the item rows a batch names and nothing else of the table: whatever needs the
    whole table's gradient, or another rank's, is refused."""
    if not lazy_table:
        return False
    if loss != "bce":
        raise ValueError(f"lazy_table=True trains loss='bce' only (got loss={loss!r}): the catalog losses' table gradients "
                         "reach rows the batch does not name")
    if exchange_active(process_group):
        raise ValueError("lazy_table=True trains on a single rank: the data-parallel step exchanges a dense table gradient")
    if shadow_gather:
        raise ValueError("lazy_table=True and shadow_gather exclude each other: shadow_gather belongs to the sharded exchange")
    if float(l2_emb) != 0.0:
        raise ValueError(f"lazy_table=True needs l2_emb == 0 (got {l2_emb}): the norm term's gradient touches every row")
    if float(weight_decay) != 0.0:
        raise ValueError(f"lazy_table=True needs weight_decay == 0 (got {weight_decay}): the decay multiplies every row")
    if max_grad_norm is not None:
        raise ValueError(f"lazy_table=True needs max_grad_norm=None (got {max_grad_norm}): the table gradient is never "
                         "materialised, so there is nothing to take a norm of")
    return True


class FusedTrainer:
    """Owns optimizer state and step buffers for one model on one GPU (one rank of a DP job)."""

    def __init__(self, model, batch_size: int, seq_len: int | None = None, lr: float = 1e-3, betas=(0.9, 0.98),
                 eps: float = 1e-8, l2_emb: float = 0.0, seed: int = 42, process_group=None, use_graph: bool = True,
                 slots: int = 1, exchange: str = "sharded", deterministic: bool = False, shadow_gather: bool = False,
                 loss: str = "bce", num_negatives: int = 1024, neg_counts=None, neg_alpha: float = 1.0,
                 logq_correction: bool = True, remove_accidental_hits: bool = True, gbce_beta: float = 1.0,
                 weight_decay: float = 0.0, max_grad_norm: float | None = None, lr_schedule: str = "constant",
                 warmup_steps: int = 0, total_steps: int | None = None, final_lr_ratio: float = 0.0,
                 lazy_table: bool = False, key_sort: str = "torch"):
        """``shadow_gather`` (sharded exchange over a bf16 item-table shadow, ``model.use_bf16_table()``; SURVEY 8e's alternative
        for BASELINE configs[4]): the fp32 master of an item row and its Adam moments live on the OWNER rank only; after the
        sharded Adam step the all-gather carries the bf16 SHADOW of the table (2 bytes per element: 90 MB instead of 180 MB at
        1 M items) and a small all-reduce the dense parameters.  Every gather of the step reads the shadow, so the arithmetic
        is that of the bf16-table mode; a rank's fp32 rows OUTSIDE its shard go stale - call ``sync_master()`` (one fp32
        all-gather) before reading ``model.state_dict()`` / saving a checkpoint.
        ``deterministic``: the item-table gradient is scattered by a stable sort + per-item ordered sums instead of float
        atomics - every step bitwise reproducible (the dense gradients already are: fixed slab tree), at the cost of one
        sort of 3 B L keys per step.
        ``loss``: "bce" (the reference's masked BCE on the positive / negative ids), or a softmax cross-entropy over the
        positive ids, mean over the positions with a target: "sampled_softmax" against ``num_negatives``
        shared negatives that every step draws on the device (``srfrd_shared_negatives``), uniformly or by
        ``neg_counts ** neg_alpha`` (``neg_counts`` (n_items + 1,), indexed by item id), with the log-Q correction
        (``logq_correction``) and accidental-hit removal (``remove_accidental_hits``) of ``model.sampled_softmax_loss``;
        "softmax": the full catalog, as ``model.full_catalog_loss``.  The negative-id planes of a batch are not read under
        a cross-entropy loss.  ``negatives`` / ``log_q`` show what the last step drew.  The cross-entropy steps run on one
        rank with the fp32 item table; the sampled step's table gradient is always reduced in a fixed order (bitwise
        reproducible, whatever ``deterministic`` says).
        "token_softmax" / "gbce": ``num_negatives`` = K negatives PER POSITION, the two objectives of
        ``model.token_negatives_loss``, ``gbce_beta`` from ``srfrd_amd.gbce_beta``.  The negatives are
        batch data: ``step(..., negative_ids (B, L, K), nrs, log_q=None)``, or a producer fills ``neg_ring[s]`` /
        ``log_q_ring[s]`` beside ``ids_ring[s]`` (``DeviceSampler(num_negatives=K).next_batch(packed=True, out=..., neg_out=...,
        log_q_out=...)``) and calls ``step_slot(s)``.  ``logq_correction=False``, and "gbce" always, pass no log-Q to the head.
        Single rank, fp32 table, always bitwise reproducible.
        ``weight_decay`` (decoupled, torch.optim.AdamW's: the whole flat vector is one group), ``max_grad_norm``
        (``torch.nn.utils.clip_grad_norm_`` over the whole gradient, ``l2_emb`` term included; ``float("inf")`` only measures),
        ``lr_schedule`` ("constant" | "linear" | "cosine") with ``warmup_steps``, ``total_steps`` and ``final_lr_ratio``
        (``srfrd_amd.lr_at`` is the formula): all three live on the device, inside the captured step -
        ``grad_norm`` and ``next_lr`` show them.  Single rank.  With every one at its default the step issues exactly the
        launches of plain Adam.
        ``lazy_table``: lazy Adam for the item table - a row's value and moments are stepped only on the
        steps whose batch names it (as an input, positive or negative id), with the global step's bias correction; every
        other row keeps its bits, and the dense parameters step as always.  A different optimizer, not a faster dense one:
        after the first step the parameters differ from the dense trainer's.  The table's share of the step then costs in
        proportion to the batch, not the catalog.  Implies ``deterministic``; single rank, ``loss="bce"``, no ``l2_emb`` /
        ``weight_decay`` / ``max_grad_norm`` / ``shadow_gather`` (``lr_schedule`` / ``warmup_steps`` are fine).  The state
        format is the dense trainer's: checkpoints move between the two.
        ``key_sort``: who sorts a sorted step's key list - "torch" (rocprim through torch: a list over 2^20
        keys is sorted eagerly between two graphs, and the token step's always) or "device" (``srfrd_sort_keys``: 2 or 3 radix
        passes over the bits an item id has, kernel launches only, so the whole step - the token step too - is one graph at
        every length).  A stable sort has one correct output: parameters, moments and loss are the same bits under both, and
        the option is no part of ``state_dict()``.  A trainer that sorts nothing ignores it."""
        if key_sort not in KEY_SORTS:
            raise ValueError(f"key_sort must be one of {KEY_SORTS} (got {key_sort!r})")
        self.lazy_table = _lazy_config(lazy_table, loss, process_group, shadow_gather, l2_emb, weight_decay, max_grad_norm)
        self.opts, self.max_norm = _optim_config(lr, betas, weight_decay, max_grad_norm, lr_schedule, warmup_steps, total_steps,
                                                 final_lr_ratio, process_group)
        q = _loss_config(model, loss, num_negatives, neg_counts, neg_alpha, process_group, gbce_beta,
                         int(batch_size) * int(seq_len or model.layout.max_len))
        self.model = model
        model._ensure_flat()
        self.lay = model.layout
        self._key_mask = model.key_padding_mask      # (in the captured launches' arguments: fixed for this trainer's life)
        self.flat = model._flat
        dev = self.flat.device
        self.B, self.L = int(batch_size), int(seq_len or self.lay.max_len)
        n_f, n_b = _lib.scratch_floats(self.lay, self.B, self.L)      # 0 when the working set fits LDS
        # (where the plan has the one-launch train kernel, its forward hands the head's hidden-state gradient to its backward
        # through the scratch: srfrd_train_scratch_floats)
        fused = _lib.PLAN_POS | _lib.PLAN_NEG | _lib.PLAN_CKPT | _lib.PLAN_LOSS | _lib.PLAN_FUSED_BCE
        has_train = bool(_lib.encoder_plan_train(self.lay, self.B, self.L, fused)[0])
        n_t = int(query("srfrd_train_scratch_floats", lay=self.lay, B=self.B, L=self.L)) if has_train else 0
        self.n_scratch = max(n_f, n_b, n_t)
        self.scratch = torch.empty(self.n_scratch, device=dev, dtype=torch.float32) if self.n_scratch else None
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.group = process_group
        self.n_tab, self.n_flat = model.n_table_pad, model.n_flat
        self.ex = GradExchange(self.n_flat, process_group)
        self.world, self.rank = self.ex.world, self.ex.rank
        if exchange not in ("sharded", "allreduce"):
            raise ValueError("exchange must be 'sharded' or 'allreduce'")
        self.mode = exchange if self.ex.on else "single"      # (ex.on: world > 1, or a forced exchange in a group of one)
        self.shadow_gather = bool(shadow_gather) and self.mode == "sharded"
        if shadow_gather and self.mode == "sharded" and not model.bf16_table:
            raise ValueError("shadow_gather exchanges the bf16 item-table shadow: call model.use_bf16_table() first")
        lay, B, L = self.lay, self.B, self.L
        f32 = dict(device=dev, dtype=torch.float32)
        if self.mode == "sharded":
            # gradient padded to world equal shards; Adam moments and the reduce-scatter landing buffer for the own shard only
            if self.ex.n_pad > model._flat_store.numel():
                raise RuntimeError("flat parameter storage has too little slack for this world size")
            self.flat_pad = model._flat_store[:self.ex.n_pad]
            self.grad = torch.zeros(self.ex.n_pad, **f32)
            self.stats = torch.zeros(4, **f32)
            self.recv = torch.zeros(self.ex.per, **f32)
            self.m = torch.zeros(self.ex.per, **f32)
            self.v = torch.zeros(self.ex.per, **f32)
            if self.shadow_gather:
                # the shadow padded to the shard grid (the all-gather walks the flat index space in 2-byte elements); the
                # model's kernels keep reading its first n_table elements
                self.shadow_pad = torch.zeros(self.ex.n_pad, device=dev, dtype=torch.int16)
                self.shadow_pad[:self.lay.n_table].copy_(model._table16)
                model._table16 = self.shadow_pad[:self.lay.n_table]
                model._bf16_auto = False                     # (the trainer keeps the shadow current; the fp32 table is partly stale)
                self.n_dense_x = self.n_flat - self.n_tab    # dense parameters (+ tail padding): exchanged in fp32
                self.dense_x = torch.zeros(self.n_dense_x, **f32)
        else:
            self.grad = torch.zeros(self.n_flat + 4, **f32)      # [table | dense | stats(4)]: one vector, one all-reduce
            self.stats = self.grad[self.n_flat:]
            self.m = torch.zeros(self.n_flat, **f32)
            self.v = torch.zeros(self.n_flat, **f32)
        # l2_emb * sum_p ||p|| (trainer.py:39): one segment per parameter tensor of the flat vector (the item table first)
        self.l2 = float(l2_emb)
        if self.l2 != 0.0:
            segs = [(off, p.numel()) for p, off in model._slots]
            assert segs[0][0] == 0 and all(off >= self.n_tab for off, _ in segs[1:])
            self.seg_off = torch.tensor([o for o, _ in segs], device=dev, dtype=torch.int64)
            self.seg_len = torch.tensor([n for _, n in segs], device=dev, dtype=torch.int64)
            self.l2_partial = torch.zeros(240 + len(segs), **f32)
            self.l2buf = torch.zeros(4, **f32)
            self.l2_dense = torch.zeros(self.n_flat - self.n_tab, **f32)
        self.state = torch.zeros(32, device=dev, dtype=torch.int32)
        self.state[1] = int(seed) & 0x7FFFFFFF
        if self.max_norm is not None:        # srfrd_grad_norm's workspace and its {norm, coefficient}
            self.norm_partial = torch.zeros(_lib.GRAD_NORM_PARTIALS, device=dev, dtype=torch.float64)
            self.clip = torch.zeros(2, **f32)
        self.deterministic = bool(deterministic) or self.lazy_table      # (lazy Adam starts from the sorted row keys)
        if self.lazy_table and (self.n_tab & 3 or self.flat.data_ptr() & 15):
            raise RuntimeError("lazy_table: the dense parameters do not start on a float4 boundary of the flat vector")
        self.loss_kind = loss
        self.sampled = loss == "sampled_softmax"
        self.token = loss in TOKEN_LOSSES
        # (the sampled and the token-negatives steps keep the encoder's contribution rows in buffers of their own, below)
        self.contrib = torch.zeros(3, B, L, lay.d_item, **f32) if self.deterministic and not (self.sampled or self.token) else None
        # A sorted step's key list (a row of the table per entry), where its stable sort lands, and the contribution rows the
        # list keys, in list order (BCE: the pos, neg and input planes of `contrib`; the other losses: _init_ce).  An unsorted
        # trainer has none of this.
        self.n_keys = sort_key_count(loss, self.deterministic, self.lazy_table, B, L,
                                     num_negatives if self.sampled or self.token else 0)
        self.keys = torch.zeros(self.n_keys, device=dev, dtype=torch.int64) if self.n_keys else None
        self.skeys, self.order = (torch.zeros_like(self.keys), torch.zeros_like(self.keys)) if self.n_keys else (None, None)
        self.key_rows = self.contrib
        # key_sort="device": the workspace of srfrd_sort_keys for this list and this table (None: torch sorts, or nothing is sorted)
        self.key_sort = key_sort
        self.sort_ws = None
        if key_sort == "device" and self.n_keys:
            n_ws = int(query("srfrd_sort_keys_workspace_bytes", n=self.n_keys, key_max=lay.n_items))
            if n_ws <= 0:
                raise ValueError(f"key_sort='device': srfrd_sort_keys refuses {self.n_keys} keys of a table of {lay.n_items} items")
            self.sort_ws = torch.empty(n_ws, device=dev, dtype=torch.uint8)
        self.n_slabs = query("srfrd_bwd_grid", lay=lay, B=B, L=L)
        self.slabs = torch.empty(self.n_slabs, lay.n_dense, **f32)
        # Input ring: `slots` resident (6, B, L) id buffers.  A producer (DeviceSampler, a loader thread's H2D copy)
        # fills slot k + 1 while step k runs and calls step_slot(k + 1): no staging copy on the step's stream.  Slot 0
        # is also the landing buffer of step() / step_packed(), which copy their arguments in.
        self.slots = max(1, int(slots))
        self.ids_ring = torch.zeros(self.slots, 6, B, L, device=dev, dtype=torch.int64)
        self.ids = self.ids_ring[0]
        self.hidden = torch.empty(B, L, lay.d_out, **f32)
        self.pl = torch.empty(B, L, **f32)
        self.nl = torch.empty(B, L, **f32)
        # (zeros, not empty: the ragged kernels write and read only the rows of a sequence's computed tiles; rows nobody
        # wrote must never hold a NaN pattern if a full-row kernel is switched in between two steps)
        self.save_x = torch.zeros(B, lay.n_blocks + 1, L, lay.D, **f32)
        self.save_h1 = torch.zeros(B, lay.n_blocks, L, lay.D, **f32)
        self.save_aux = torch.zeros(query("srfrd_aux_floats", lay=lay, B=B, L=L), **f32)
        self.loss_part = torch.empty(B, 3, **f32)
        self.loss = torch.zeros(1, **f32)
        # Sequence -> workgroup schedule of the seq_len-50 ragged kernels (include/srfrd_hip.h, srfrd_seq_order): one small
        # launch per step ranks the batch by length, forward and backward pair a long with a short sequence on every CU.
        # Built where the kernel plan runs the ragged pair for this shape without switches (a test may set one later; the
        # other kernels ignore the schedule).  SRFRD_SCHED = 0 (off: workgroup x takes sequence x) | 1 (length order; default)
        # (a cross-entropy step runs the encoder without targets: checkpoints only, and its own head after the forward)
        plan_mode = fused if loss == "bce" else _lib.PLAN_CKPT
        ragged = _lib.encoder_plan(lay, B, L, plan_mode)[0][0].startswith("srfrd::encoder_fwd_ragged_kernel<")
        self.sched_mode = min(1, int(os.environ.get("SRFRD_SCHED", "1"))) if ragged else 0
        self.sched = torch.zeros(int(query("srfrd_sched_ints", B=B)), device=dev, dtype=torch.int32) if self.sched_mode else None
        self.pair_stride = max(1, query("srfrd_bwd_grid", lay=lay, B=1 << 30, L=L) // 2)      # CUs: workgroups of the first round
        # single rank: forward + backward as one launch where the plan has a train kernel (srfrd_encoder_train_ranked), asked
        # at every enqueue under the environment's switches then; False: always the two launches (A/B comparisons)
        self._train_mode = fused
        self.train_launch = True
        if loss != "bce":
            self._init_ce(q, num_negatives, logq_correction, remove_accidental_hits, gbce_beta)
        self.packed = model.pack_weights()
        self._step_begin()
        # (a key list too long to sort inside a graph: two graphs around the sort; data parallel: no graphs, and why)
        device_sort = self.sort_ws is not None
        eager_sort, self.use_graph, self.graph_capture_error = sort_plan(self.mode, self.n_keys, bool(use_graph), device_sort)
        self._program = step_program(self.mode, self.token, self.lazy_table, eager_sort, device_sort)
        self._graphs = None              # (stages, their graphs) once captured: `captured`
        self._stats_handle = None        # sharded form: the statistics all-reduce in flight between two eager stages
        self.graph_form = None           # "one" | "split" once captured (one graph per step, or graphs around the eager stages)
        self.steps_done = 0
        self.err = torch.zeros(1, device=dev, dtype=torch.int32)   # srfrd_check_ids word of step() / step_packed() inputs
        self._fresh = False      # packed weights known to match the parameters (see refresh())

    def _init_ce(self, q, num_negatives, logq_correction, remove_hits, gbce_beta=1.0):
        """buffers of the cross-entropy step (DESIGN sections 14 and 18)"""
        lay, B, L, dev = self.lay, self.B, self.L, self.flat.device
        f32 = dict(device=dev, dtype=torch.float32)
        T = B * L
        self.remove_hits = bool(remove_hits)
        self.token_loss = torch.zeros(B, L, **f32)
        self.lse = torch.zeros(B, L, **f32)
        self.d_token = torch.ones(B, L, **f32)               # d loss / d token loss = 1: SUM, the Adam tail divides by the count
        self.d_hidden = torch.zeros(B, L, lay.d_out, **f32)
        if self.sampled:
            K = self.K = int(num_negatives)
            self.logq_correction = bool(logq_correction)
            self._negatives = torch.zeros(K, device=dev, dtype=torch.int64)
            self._log_q = torch.zeros(K, **f32)
            if q is None:
                self.alias_prob = self.alias_idx = self.item_log_q = None
            else:
                prob, idx = alias_table(q)
                with np.errstate(divide="ignore"):                    # (an item of weight 0 is never drawn: its -inf is not read)
                    lq = np.concatenate([[0.0], np.log(K * q)]).astype(np.float32)
                self.alias_prob = torch.from_numpy(prob).to(dev)
                self.alias_idx = torch.from_numpy(idx).to(dev)
                self.item_log_q = torch.from_numpy(lq).to(dev)
            # one contribution buffer for the whole table gradient: rows [0, 3T) the encoder's (pos, neg, input planes; only
            # the input plane carries anything here), rows [3T, 3T + K + T) the loss head's; keys of rows [2T, 4T + K)
            self.contrib_ce = torch.zeros(4 * T + K, lay.d_item, **f32)
        elif self.token:
            K = self.K = int(num_negatives)
            self.objective = _lib.TNEG_OBJECTIVES[TOKEN_LOSSES[self.loss_kind]]
            self.gbce_beta = float(gbce_beta)
            self.logq_correction = bool(logq_correction)
            # negatives and their log-Q are batch data: one plane per input slot, beside ids_ring
            self.neg_ring = torch.zeros(self.slots, B, L, K, device=dev, dtype=torch.int64)
            self.log_q_ring = torch.zeros(self.slots, B, L, K, **f32)
            self._last_slot = 0
            # the encoder's contribution planes (pos, neg, input; only the input plane carries anything here), the head's
            # rank-1 coefficients; the step's ONE key list is [clamped input ids (T) | the head's keys (T (1 + K))]
            self.contrib_tok = torch.zeros(3, B, L, lay.d_item, **f32)
            self.coef_tok = torch.zeros(T * (1 + K), **f32)
        elif self.deterministic:
            self.de_ce = torch.zeros(lay.n_items + 1, lay.d_item, **f32)
        # What the step's compute asks of the loss: its head, where the head's backward leaves the table gradient, the encoder
        # backward's contribution buffer, and the full rows that `keys` - its first T entries the clamped input ids - keys
        if self.token:       #  T (1 + K) coefficients and, behind the T input keys, their keys, unreduced
            head, self.ce_grad_to = loss_heads.TNEG, dict(rows=self.coef_tok, keys=self.keys[T:], finish=False)
            self.ce_contrib, self.key_rows = self.contrib_tok, self.contrib_tok[2].view(T, lay.d_item)
        elif self.sampled:   # its rows and keys land behind the encoder's in the merged buffers, unreduced: one sort for both
            head, self.ce_grad_to = loss_heads.SXENT, dict(rows=self.contrib_ce[3 * T:], keys=self.keys[T:], finish=False)
            self.ce_contrib, self.key_rows = self.contrib_ce, self.contrib_ce[2 * T:]
        else:
            # xent_bwd writes a dense table gradient; the deterministic encoder table reduction STORES its rows (the input
            # plane of `contrib`), so there the head's part waits in de_ce and is added afterwards
            det = self.contrib is not None
            head, self.ce_grad_to = loss_heads.XENT, dict(d_table=self.de_ce if det else self.grad, accumulate=not det)
            self.ce_contrib, self.key_rows = self.contrib, self.contrib[2] if det else None
        self.ce_head = head
        n_ws = head.workspace(lay, B, L, self.K if self.sampled or self.token else 0)
        if self.token:
            # the mixed reduction's list is T (2 + K) long: more than srfrd_tneg_workspace_floats covers
            n_mix = loss_heads.mixed_workspace(T * (2 + self.K), lay.d_item)
            n_ws = max(n_ws, n_mix) if n_ws > 1 and n_mix > 0 else 0      # (TNEG.workspace answers 1 for a refusal)
        if n_ws <= 0:
            raise ValueError(f"loss={self.loss_kind!r}: the cross-entropy kernels refuse this model / shape")
        self.ce_ws = torch.zeros(n_ws, **f32)

    @property
    def negatives(self):
        """(K,) int64: the shared negatives the last sampled-softmax step drew; "token_softmax" / "gbce": (B, L, K), the
        negative plane the last step read (None under another loss); a copy"""
        if self.token:
            return self.neg_ring[self._last_slot].detach().clone()
        return self._negatives.detach().clone() if self.sampled else None

    @property
    def log_q(self):
        """(K,) float32: log(K q) of those negatives, whether or not the loss subtracts it; "token_softmax" / "gbce": (B, L,
        K), the log-Q plane of the last step's slot (None under another loss); a copy"""
        if self.token:
            return self.log_q_ring[self._last_slot].detach().clone()
        return self._log_q.detach().clone() if self.sampled else None

    @property
    def grad_norm(self):
        """device scalar (a view): the last step's global L2 norm of the mean-loss gradient, the ``l2_emb`` term included,
        before clipping (None without ``max_grad_norm``; ``float("inf")`` measures without clipping)"""
        return self.clip[0] if self.max_norm is not None else None

    @property
    def next_lr(self):
        """device scalar (a view): the learning rate the next step will use (None where no option is set: ``lr`` then)"""
        return self.state[3:4].view(torch.float32)[0] if self.opts is not None else None

    # ---- pieces -------------------------------------------------------------------------------
    def _step_begin(self):
        """state words of the step t = state[0] + 1: plain, or (an option set) under the schedule"""
        if self.opts is None:
            call("srfrd_step_begin", state=self.state, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1])
        else:
            call("srfrd_step_begin_sched", state=self.state, opts=self.opts)

    def _enc_args(self, slot, targets: bool):
        """the named arguments every encoder entry point begins with (_lib.encoder_head): layout and tables, the slot's id
        planes (``targets``: the positive / negative planes and their logits too; else NULL - checkpoints and hidden states
        only), shape, dropout rate and seed word, this rank's first global sequence, then the forward's outputs and checkpoints"""
        ids, kind = self.ids_ring[slot], self.lay.kind
        fk = ids[1] if kind != 0 else None
        pos, neg = (ids[2], ids[4]) if targets else (None, None)
        pfk, nfk = (ids[3], ids[5]) if targets and kind == 2 else (None, None)
        p = self.model.dropout_rate if self.model.training else 0.0
        return _lib.encoder_head(self.model._table_args(), self.flat, self.n_tab, self.packed, (ids[0], fk, pos, pfk, neg, nfk),
                                 self.B, self.L, p, self.rank * self.B,
                                 (self.hidden, self.pl, self.nl, self.save_x, self.save_h1, self.save_aux),
                                 seed_dev=self.state.data_ptr() + 8)

    def _bwd_args(self, d_hidden, contrib):
        """what a backward adds to `_enc_args`: the hidden-state gradient it starts from (None: the BCE gradient of the
        target logits, fused), the gradient vector, the item-table contribution rows (None: float atomics into the gradient),
        the dense slabs and the scratch"""
        return dict(d_hidden=d_hidden, d_pos=None, d_neg=None, fused_bce=int(d_hidden is None), grad_table=self.grad,
                    table_contrib=contrib, grad_slabs=self.slabs, scratch=self.scratch, scratch_floats=self.n_scratch)

    def _sched_args(self):
        return dict(sched=self.sched, sched_mode=self.sched_mode)

    def _launch_fwd(self, slot, targets: bool):
        call("srfrd_encoder_fwd_sched", **self._enc_args(slot, targets), loss_part=self.loss_part if targets else None,
             scratch=self.scratch, scratch_floats=self.n_scratch, **self._sched_args())

    def _launch_bwd(self, slot, d_hidden=None, contrib=None):
        call("srfrd_encoder_bwd_sched", **self._enc_args(slot, d_hidden is None), **self._bwd_args(d_hidden, contrib),
             **self._sched_args())

    def _launch_train(self, slot):
        """forward and BCE backward of every sequence as one launch; the kernel ranks the batch by length itself (no
        srfrd_seq_order in front, `sched` untouched): the two launches' sequence -> workgroup order, so their bits"""
        call("srfrd_encoder_train_ranked", **self._enc_args(slot, True), loss_part=self.loss_part, fused_bce=1,
             grad_table=self.grad, table_contrib=self.contrib, grad_slabs=self.slabs,
             pair_stride=self.pair_stride if self.sched_mode else 0)

    def _enqueue_prologue(self, slot, schedule: bool = True):
        """ahead of the forward: the norms of the parameters it uses (l2_emb), the batch's sequence -> workgroup schedule
        (``schedule`` False: the launch that follows ranks the batch itself)"""
        if self.l2 != 0.0:
            call("srfrd_l2_norms", param=self.flat, seg_off=self.seg_off, seg_len=self.seg_len, n_seg=self.seg_off.numel(),
                 n_table_pad=self.n_tab, l2_emb=self.l2, partial=self.l2_partial, l2buf=self.l2buf, dense_scale=self.l2_dense)
        if self.sched_mode and schedule:
            call("srfrd_seq_order", input_ids=self.ids_ring[slot][0], B=self.B, L=self.L, pair_stride=self.pair_stride,
                 sched=self.sched)

    def _enqueue_l2_apply(self, grad, param, i0, i1):
        """grad[i0:i1] += count * l2_emb * p / ||p|| (the Adam step that follows divides by the count)"""
        call("srfrd_l2_apply", grad=grad, param=param, i0=i0, i1=min(i1, self.n_flat), n_table_pad=self.n_tab, l2buf=self.l2buf,
             dense_scale=self.l2_dense, stats=self.stats)

    def _enqueue_fwd(self, slot: int = 0):
        self._enqueue_prologue(slot)
        self._launch_fwd(slot, True)
        if self.mode == "sharded":       # the statistics are forward outputs: reduce them now, exchange them under the backward
            call("srfrd_loss_stats", loss_part=self.loss_part, B=self.B, stats=self.stats, loss_out=None)

    def _enqueue_bwd(self, slot: int = 0):
        self._launch_bwd(slot, None, self.contrib)
        self._enqueue_grad_tail(slot)

    # A step with a key list is cut at the same place into three pieces: up to the key list (the compute, then `_write_keys`),
    # the sort (`_sort_keys`), and what follows it (`_enqueue_reduce`, then the update).  Where the sort is captured they run
    # back to back (`_enqueue_grad_tail`, `_enqueue_step_compute`); step_program(eager_sort=True) makes them three stages.
    def _write_keys(self, slot: int = 0):
        """the slot's ids into the key list: BCE, the pos, neg and input planes (the row order of `contrib`); a cross-entropy
        loss, the clamped input ids into the list's head (the head's backward wrote the rest)"""
        if self.keys is None:        # (the float-atomic scatter)
            return
        ids = self.ids_ring[slot]
        if self.loss_kind == "bce":
            torch.stack((ids[2], ids[4], ids[0]), out=self.keys.view(3, self.B, self.L))
        else:
            torch.clamp(ids[0].reshape(-1), 0, self.lay.n_items, out=self.keys[:self.B * self.L])

    def _sort_keys(self):
        """THE stable sort of the step's key list, into its persistent buffers.  Captured with the step up to
        SORT_CAPTURE_LIMIT keys; a longer list (and the token step's, always) is sorted eagerly, between the step's two graphs -
        checked here on the host, ahead of the sort: a mistake in a program costs an error, not a machine.
        ``key_sort="device"`` (a trainer with `sort_ws`): srfrd_sort_keys instead - the same bits from kernel launches alone,
        captured wherever the program puts it"""
        sort_ws = getattr(self, "sort_ws", None)
        if sort_ws is not None:
            call("srfrd_sort_keys", keys=self.keys, n=self.keys.numel(), key_max=self.lay.n_items, sorted_keys=self.skeys,
                 order=self.order, workspace=sort_ws, ws_bytes=sort_ws.numel())
            return
        if self.keys.numel() > SORT_CAPTURE_LIMIT and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"a sort of {self.keys.numel()} keys (more than {SORT_CAPTURE_LIMIT}) must not be captured: "
                               "its memset nodes do not replay reliably (DESIGN section 18)")
        torch.sort(self.keys, stable=True, out=(self.skeys, self.order))

    def _enqueue_table_reduce(self):
        """the table gradient from the sorted key list, one ordered sum per item: of the full rows the list keys; the token
        step's, per item its input positions' full rows, then its rank-1 rows coef * hidden[t] (the backward read `hidden`, it
        did not write it).  Lazy Adam makes no table gradient: `_enqueue_reduce` steps the rows instead."""
        lay = self.lay
        if self.token:
            loss_heads.table_mixed(lay, self.hidden, self.K, self.key_rows, self.coef_tok, self.keys, self.ce_ws, self.grad,
                                   sorted_pair=(self.skeys, self.order))
        elif not self.lazy_table:
            call("srfrd_table_reduce", sorted_keys=self.skeys, order=self.order, table_contrib=self.key_rows, n=self.n_keys,
                 d_item=lay.d_item, grad_table=self.grad)
            if self.loss_kind == "softmax":      # (the reduction stored the rows: the head's dense part waited in de_ce)
                self.grad[:lay.n_table].add_(self.de_ce.view(-1))

    def _enqueue_reduce(self):
        """after the sort (an unsorted step: after the backward): the table gradient from the sorted keys, the dense-gradient
        slab reduction (+ loss), lazy Adam's rows"""
        if self.keys is not None:
            self._enqueue_table_reduce()
        if self.loss_kind != "bce":
            self._enqueue_ce_dense()
            return
        # single rank: the slab reduction also finalises the loss; all-reduce form: it leaves the local statistics behind the
        # gradient (one vector, one collective); sharded form: the statistics were reduced right after the forward
        fuse_stats = self.mode != "sharded"
        self._enqueue_ce_dense(self.loss_part if fuse_stats else None, self.stats if fuse_stats else None,
                               self.loss if self.mode == "single" else None)
        if self.lazy_table:
            # lazy Adam: from the sorted keys straight to the stepped rows - behind the slab reduction,
            # which finalised the count in `stats`, and ahead of the dense update, which advances `state`.  No table gradient:
            # its slice of `grad` is never written and stays zero.
            call("srfrd_table_reduce_adam", sorted_keys=self.skeys, order=self.order, table_contrib=self.key_rows, n=self.n_keys,
                 d_item=self.lay.d_item, n_rows=self.lay.n_items + 1, table=self.flat, m=self.m, v=self.v, beta1=self.betas[0],
                 beta2=self.betas[1], eps=self.eps, state=self.state, stats=self.stats, table_bf16=self.model._table16)

    def _enqueue_grad_tail(self, slot: int = 0):
        """after the BCE backward: the key list, its sort and what follows it (an unsorted step: the slab reduction alone)"""
        self._write_keys(slot)
        if self.keys is not None:
            self._sort_keys()
        self._enqueue_reduce()

    def _enqueue_ce_dense(self, loss_part=None, stats=None, loss_out=None):
        """the dense-gradient slab reduction (the cross-entropy step's: alone, its head has made the loss statistics)"""
        call("srfrd_reduce_dense", grad_slabs=self.slabs, n_slabs=self.n_slabs, n_dense=self.lay.n_dense,
             grad_dense=_lib.dense_ptr(self.grad, self.n_tab), loss_part=loss_part, B=self.B, stats=stats, loss_out=loss_out)

    def _launch_ce(self, slot: int = 0):
        """the cross-entropy step's launches (single rank): [shared negatives] -> encoder forward (checkpoints,
        hidden) -> loss head forward, {sum, count} into stats[1..2] -> loss head backward with d token loss = 1 -> encoder
        backward from d_hidden.  stats[0] stays 0, so the Adam tail's 1 / stats[2] and srfrd_loss_finalize give the gradient of
        the mean and the mean."""
        lay = self.lay
        self._enqueue_prologue(slot)
        if self.sampled:
            call("srfrd_shared_negatives", state=self.state, n_items=lay.n_items, K=self.K, alias_prob=self.alias_prob,
                 alias_idx=self.alias_idx, item_log_q=self.item_log_q, out_ids=self._negatives, out_log_q=self._log_q)
        self._launch_fwd(slot, False)
        # the loss head (loss_heads.py) on the step's own buffers; the fp32 item table is the flat vector's head
        if self.token:
            log_q = self.log_q_ring[slot] if self.logq_correction and self.loss_kind == "token_softmax" else None
            args = (self.neg_ring[slot], log_q, self.objective, self.gbce_beta, self.remove_hits)
        else:
            args = (self._negatives, self._log_q if self.logq_correction else None, self.remove_hits) if self.sampled else ()
        table, tgt = ptr(self.flat), self.ids_ring[slot][2]
        loss_heads.launch_fwd(self.ce_head, lay, table, self.hidden, tgt, args, ws=self.ce_ws,
                              out=(self.token_loss, self.lse, self.stats[1:]))       # {sum, count} -> stats[1], stats[2]
        loss_heads.launch_bwd(self.ce_head, lay, table, self.hidden, tgt, args, self.lse, self.d_token, ws=self.ce_ws,
                              d_hidden=self.d_hidden, **self.ce_grad_to)
        self._launch_bwd(slot, self.d_hidden, self.ce_contrib)

    def _enqueue_ce_compute(self, slot: int = 0):
        """the cross-entropy step's compute, through the table gradient and the dense slab reduction.  The token-negatives
        step's ends with its key list: the sort, the table gradient and the slab reduction are the step program's next stages."""
        if self.token:
            self._enqueue_to_keys(slot)
        else:
            self._enqueue_step_compute(slot)

    def _enqueue_compute(self, slot: int = 0):
        """forward and backward as their two launches (the data-parallel step, per-launch timing)"""
        self._enqueue_fwd(slot)
        self._enqueue_bwd(slot)

    def _enqueue_to_keys(self, slot: int = 0):
        """the single-rank step up to its key list: the loss's launches - BCE: forward and backward as ONE launch where the
        kernel plan offers a train kernel (each workgroup runs its sequence's backward right after its forward; the same bits as
        the two launches), else the two - then the slot's ids into the list"""
        if self.loss_kind != "bce":
            self._launch_ce(slot)
        elif self.mode == "single" and self.train_launch and _lib.encoder_plan_train(
                self.lay, self.B, self.L, self._train_mode, _lib.env_switches())[0]:
            self._enqueue_prologue(slot, schedule=False)
            self._launch_train(slot)
        else:
            self._enqueue_fwd(slot)
            self._launch_bwd(slot, None, self.contrib)
        self._write_keys(slot)

    def _enqueue_step_compute(self, slot: int = 0):
        """the single-rank step's compute: its three pieces back to back"""
        self._enqueue_to_keys(slot)
        if self.keys is not None:
            self._sort_keys()
        self._enqueue_reduce()

    def _enqueue_compute_update(self, slot: int = 0):
        """the single-rank step, whole: one graph per slot"""
        self._enqueue_step_compute(slot)
        self._enqueue_update()

    def _enqueue_lazy_step(self, slot: int = 0):
        """the ``lazy_table`` step, whole: one graph per slot.  The compute of the single-rank step with the sorted scatter;
        `_enqueue_reduce` ends in srfrd_table_reduce_adam in place of srfrd_table_reduce; then the dense parameters"""
        self._enqueue_step_compute(slot)
        self._enqueue_lazy_update()

    def _enqueue_lazy_update(self):
        """``lazy_table``: the fused Adam tail over the dense parameters alone - every vector biased by the padded table, so
        the launch sees a flat vector without a table (n_table_pad 0: its pack indices are the dense ones).  It re-packs the
        stepped weights and advances `state`, as always; the bf16 shadow belongs to the row kernel."""
        nt = self.n_tab
        vec = dict(lay=self.lay, param=_lib.dense_ptr(self.flat, nt), grad=_lib.dense_ptr(self.grad, nt),
                   m=_lib.dense_ptr(self.m, nt), v=_lib.dense_ptr(self.v, nt), n=self.n_flat - nt, n_table_pad=0, n_zero=0,
                   eps=self.eps, state=self.state, stats=self.stats, packed=self.packed, table_bf16=None)
        if self.opts is None:
            call("srfrd_adam_pack_step", **vec, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1])
        else:       # (a schedule: the W form at decay 1 runs the plain form's arithmetic - srfrd_optim.hip, mul_rounded)
            call("srfrd_adamw_pack_step", **vec, opts=self.opts, clip=None)

    def _enqueue_update(self):
        """single rank / all-reduce form: Adam over the whole flat vector + re-pack + optimizer-state advance, one launch
        (an optimizer option set: [the gradient norm, then] the AdamW form of that launch)"""
        if self.l2 != 0.0:
            self._enqueue_l2_apply(self.grad, self.flat, 0, self.n_flat)
        vec = dict(lay=self.lay, param=self.flat, grad=self.grad, m=self.m, v=self.v, n=self.n_flat, n_table_pad=self.n_tab,
                   n_zero=self.n_tab, eps=self.eps, state=self.state, stats=self.stats, packed=self.packed,
                   table_bf16=self.model._table16)
        if self.opts is None:
            call("srfrd_adam_pack_step", **vec, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1])
        else:
            # the options: the gradient's global norm and clip coefficient, measured behind the l2_emb term,
            # then Adam with the coefficient in its gradient scale, the decay factor of state[7], and the scheduled advance
            if self.max_norm is not None:
                call("srfrd_grad_norm", grad=self.grad, n=self.n_flat, stats=self.stats, max_norm=self.max_norm,
                     partial=self.norm_partial, out=self.clip)
            call("srfrd_adamw_pack_step", **vec, opts=self.opts, clip=self.clip if self.max_norm is not None else None)
        if self.mode != "single" or self.loss_kind != "bce":      # (single-rank BCE: the slab reduction wrote the loss)
            call("srfrd_loss_finalize", stats=self.stats, loss_out=self.loss)
        if self.l2 != 0.0:
            self.loss.add_(self.l2buf[1:2])

    def _enqueue_shard_update(self):
        """sharded form, between the reduce-scatter and the all-gather: re-zero the local item-table gradient (the atomics
        of the next backward accumulate into it) and step this rank's slice; `recv`, `m`, `v` hold that slice only, so
        their pointers are biased by -i0 to be indexed with the global element index."""
        ex = self.ex
        self.grad[:self.n_tab].zero_()
        bias = 4 * ex.i0
        if self.l2 != 0.0:
            self._enqueue_l2_apply(self.recv.data_ptr() - bias, self.flat_pad, ex.i0, ex.i1)
        sg = self.shadow_gather      # (the owner writes the bf16 shadow of the table elements it steps)
        call("srfrd_adam_step", param=self.flat_pad, grad=self.recv.data_ptr() - bias, m=self.m.data_ptr() - bias,
             v=self.v.data_ptr() - bias, n=ex.n_pad, i0=ex.i0, i1=ex.i1, n_zero=0, beta1=self.betas[0], beta2=self.betas[1],
             eps=self.eps, state=self.state, stats=self.stats, table_bf16=self.shadow_pad if sg else None,
             n_table=self.lay.n_table if sg else 0)
        if sg:
            # this rank's part of the dense parameters into the exchange buffer (zeros elsewhere: the SUM all-reduce is a gather)
            self.dense_x.zero_()
            lo, hi = max(ex.i0, self.n_tab), min(ex.i1, self.n_flat)
            if hi > lo:
                self.dense_x[lo - self.n_tab:hi - self.n_tab].copy_(self.flat_pad[lo:hi])

    def _gather_params(self):
        """sharded form: every rank's stepped slice to all ranks - the fp32 vector, or (shadow_gather) the bf16 shadow of the
        table + the dense parameters"""
        if not self.shadow_gather:
            self.ex.all_gather(self.flat_pad)
            return
        self.ex.all_gather(self.shadow_pad.view(torch.float16))      # (2-byte elements; RCCL has no int16: the bits travel as fp16)
        self.ex.all_reduce(self.dense_x)
        self.flat[self.n_tab:self.n_flat].copy_(self.dense_x)

    def sync_master(self):
        """shadow_gather: bring every rank's fp32 parameters up to date (one fp32 all-gather; a collective - every rank calls
        it).  No-op otherwise."""
        if self.shadow_gather:
            self.ex.all_gather(self.flat_pad)

    def _enqueue_shard_finish(self):
        """sharded form, after the all-gather: fragment-ordered copy of the stepped weights + optimizer-state advance + loss"""
        call("srfrd_pack_weights", lay=self.lay, dense=_lib.dense_ptr(self.flat, self.n_tab), packed=self.packed, state=self.state,
             lr=self.lr, beta1=self.betas[0], beta2=self.betas[1])
        if self.model._table16 is not None and not self.shadow_gather:      # bf16 shadow of the all-gathered item table (every rank needs all rows)
            call("srfrd_table_to_bf16", src=self.flat, n=self.lay.n_table, out=self.model._table16)
        call("srfrd_loss_finalize", stats=self.stats, loss_out=self.loss)
        if self.l2 != 0.0:
            self.loss.add_(self.l2buf[1:2])

    # ---- the eager stages of the data-parallel programs ---------------------------------------
    def _all_reduce_grad(self):
        self.ex.all_reduce(self.grad)

    def _start_stats_reduce(self):
        self._stats_handle = self.ex.all_reduce_stats(self.stats)      # 16 bytes, in flight under the backward

    def _scatter_grad(self):
        self.ex.reduce_scatter(self.grad, self.recv)
        h, self._stats_handle = self._stats_handle, None
        if h is not None:
            h.wait()

    # ---- the walks over the step program ------------------------------------------------------
    def _walk(self, stages, graphs, slot, local=False):
        """``stages`` in order: a stage with graphs is replayed, any other has its methods called; ``local``: without the
        collectives"""
        for (kind, per_slot, calls), gs in zip(stages, graphs):
            if gs is not None:
                gs[slot if per_slot else 0].replay()
            elif not (local and kind == "collective"):
                for name in calls:
                    getattr(self, name)(*((slot,) if per_slot and name not in SLOT_FREE else ()))

    def _enqueue_step(self, slot: int = 0, local: bool = False):
        """the whole step on the current stream: the eager step, and (data parallel over RCCL, whose collectives are stream
        work) the body of the one-graph form"""
        self._walk(self._program, [None] * len(self._program), slot, local)

    def _replay(self, slot: int = 0, local: bool = False):
        """the captured step: its graphs replayed, the eager stages between them called"""
        self._walk(*self._graphs, slot, local)

    @property
    def captured(self) -> bool:
        return self._graphs is not None

    @contextlib.contextmanager
    def _snapshot(self):
        """everything a step changes - parameters, moments, optimizer state words, gradient, statistics - put back on exit
        (and by the ``restore`` it yields), with what the model derives from the parameters"""
        torch.cuda.synchronize()
        keep = [self.flat, self.m, self.v, self.state, self.grad, self.stats] + ([self.shadow_pad] if self.shadow_gather else [])
        if self.max_norm is not None:
            keep.append(self.clip)           # (`grad_norm` keeps showing the last real step)
        snap = [t.clone() for t in keep]

        def restore():
            torch.cuda.synchronize()
            for dst, src in zip(keep, snap):
                dst.copy_(src)
            self.model.pack_weights()         # the steps re-packed the stepped weights: restore that too
            if not self.shadow_gather:        # ... and re-derived the bf16 shadow of the stepped table (if one is in use;
                self.model.refresh_bf16_table()   # shadow_gather: the shadow itself is part of the snapshot)
            torch.cuda.synchronize()

        try:
            yield restore
        finally:
            restore()

    def _graphs_of(self, stages):
        """one graph per graph stage and slot (the kernels' id pointers are baked in; a slot-independent stage: one graph),
        None per eager stage"""
        def graph_of(stage, slot):
            g = torch.cuda.CUDAGraph()
            # thread_local capture mode: a collective backend's watchdog thread may touch the HIP runtime while we capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._walk([stage], [None], slot)
            return g

        return [[graph_of(st, k) for k in range(self.slots if st[1] else 1)] if st[0] == "graph" else None for st in stages]

    def _capture(self):
        # warm-up on a side stream (sets the LDS attributes, loads code objects), then capture
        rccl = self.mode != "single" and self.ex.native
        with self._snapshot():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                # RCCL: one whole step EAGERLY, collectives included, before anything is captured - every collective type the
                # graph will hold has then run once on this communicator (lazy channel / buffer set-up cannot be captured)
                self._enqueue_step(0, local=not rccl)
            torch.cuda.current_stream().wait_stream(s)
        with self._snapshot() as restore:
            stages = graphs = None
            if rccl and os.environ.get("SRFRD_DP_SPLIT_GRAPHS", "") != "1":
                # RCCL collectives are stream work: the WHOLE data-parallel step - compute, collectives, sharded Adam, re-pack -
                # goes into ONE graph per slot, so a step is one host launch and nothing on the host sits between the kernels and
                # the collectives.  (ProcessGroupNCCL forks its internal stream off the capturing one and joins it back: the
                # statistics all-reduce stays concurrent with the backward inside the graph.)  If this torch / RCCL pair refuses
                # the capture, the step falls back to the split form below; `graph_form` says which one runs.
                try:
                    stages, graphs = ONE_GRAPH, self._graphs_of(ONE_GRAPH)
                except Exception as e:                      # noqa: BLE001 - any capture failure selects the split form
                    stages = None
                    self.graph_capture_error = repr(e)
                    restore()
            if stages is None:
                stages, graphs = self._program, self._graphs_of(self._program)
            self._graphs = (stages, graphs)
            self.graph_form = "one" if len(stages) == 1 else "split"      # (one graph per step, or graphs around eager stages)
            # The first replay of a graph also uploads it to the device (tens of microseconds, once per graph - and there is one
            # graph per input slot): replay each once here, inside the snapshot, so that no step pays for it.  (Split form: the
            # graphs only, no collective is involved; one-graph form: every rank replays the same graphs in the same order.)
            for gs in graphs:
                for g in gs or ():
                    g.replay()

    # ---- public -------------------------------------------------------------------------------
    def spin_up(self, replays: int = 200):
        """Bring the device to its steady state (clocks, caches, TLBs of the step's buffers) without training: replays the
        captured single-rank step `replays` times on whatever slot 0 holds, inside a snapshot - parameters, optimizer
        moments, step counter and dropout seed are restored afterwards, so the next step is the one it would have been.
        (The first hundred steps after start-up run ~4 % slower than the rest; a short measurement that wants the
        steady-state rate calls this first.  No-op without graphs.  In data parallel every rank replays the same graphs the same
        number of times: the one-graph form with its collectives inside, the split form's local graphs without the collectives
        between them; everything is restored.)"""
        if not self.use_graph:
            return
        if not self._fresh:
            self.refresh()
        if not self.captured:
            self._capture()
        with self._snapshot():
            for _ in range(int(replays)):
                self._replay(0, local=True)

    def refresh(self):
        """Re-derive everything the step keeps derived from the parameters (the MFMA-fragment-ordered weight copy).  Call
        after modifying parameters from outside the trainer - ``load_state_dict``, a re-initialisation, a manual edit;
        the trainer's own Adam tail keeps the copy current by itself.  Done automatically before the first step."""
        self.packed = self.model.pack_weights()
        self._fresh = True

    # ---- optimizer state in torch.optim.Adam's own format ------------------------------------------------------------
    def _moments_full(self):
        """(exp_avg, exp_avg_sq) over the whole flat vector; in the sharded form every rank holds a slice: all-gathered here
        (a collective - every rank must make the call)."""
        if self.mode != "sharded":
            return self.m, self.v
        out = []
        for part in (self.m, self.v):
            full = torch.zeros(self.ex.n_pad, device=part.device, dtype=torch.float32)
            full[self.ex.i0:self.ex.i1] = part
            out.append(self.ex.all_gather(full))
        return out[0], out[1]

    def state_dict(self):
        """The optimizer state as ``torch.optim.Adam(model.parameters(), lr, betas, eps).state_dict()`` would hold it after
        the same steps (per parameter ``step``, ``exp_avg``, ``exp_avg_sq``; one param group) - loadable by either side -
        plus ``"srfrd"``: the dropout base seed, so that a resumed run draws the masks the uninterrupted one would have.
        The reference saves the model only (trainer.py:409-411); this is what resuming TRAINING needs on top."""
        m, v = self._moments_full()
        params = list(self.model.parameters())
        off = {id(p): o for p, o in self.model._slots}
        state = {}
        for i, p in enumerate(params):
            o, n = off[id(p)], p.numel()
            state[i] = {"step": torch.tensor(float(self.steps_done)),
                        "exp_avg": m[o:o + n].view(p.shape).clone(), "exp_avg_sq": v[o:o + n].view(p.shape).clone()}
        wd = self.opts.weight_decay if self.opts is not None else 0.0
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": wd if wd else 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": bool(wd), "params": list(range(len(params)))}
        extra = {"seed": int(self.state[1].item()), "steps_done": int(self.steps_done)}
        if self.opts is not None:        # (`lr` above stays the BASE rate: the schedule maps it to the step's)
            o = self.opts
            extra["schedule"] = {"kind": LR_SCHEDULES[o.schedule], "warmup_steps": int(o.warmup_steps),
                                 "total_steps": int(o.total_steps) if o.schedule else None, "final_lr_ratio": float(o.final_ratio)}
            extra["max_grad_norm"] = self.max_norm
        if self.loss_kind != "bce":
            extra["loss"] = self._loss_signature()
        return {"state": state, "param_groups": [group], "srfrd": extra}

    def _loss_signature(self):
        """the loss configuration a resumed run must share (state_dict()["srfrd"]["loss"]; absent: "bce")"""
        if self.token:
            return {"kind": self.loss_kind, "num_negatives": self.K, "gbce_beta": self.gbce_beta,
                    "logq_correction": self.logq_correction, "remove_accidental_hits": self.remove_hits}
        if not self.sampled:
            return {"kind": self.loss_kind}
        return {"kind": self.loss_kind, "num_negatives": self.K, "popularity": self.alias_prob is not None,
                "logq_correction": self.logq_correction, "remove_accidental_hits": self.remove_hits}

    def load_state_dict(self, sd):
        """Inverse of state_dict(); also takes the state_dict of a torch.optim.Adam / AdamW (or srfrd_amd.Adam / AdamW) that
        stepped the same model's parameters (the module-level path), so a run can move between the two.  Hyper-parameters come
        from the dict: ``lr`` is the BASE rate, ``weight_decay`` is taken with ``decoupled_weight_decay`` only (the coupled,
        L2-style decay of torch.optim.Adam is refused), and ``"srfrd"`` carries the schedule and ``max_grad_norm``; where it
        carries neither (a torch optimizer's state) this trainer keeps its own.  The state of a torch LR scheduler is NOT
        translated: give the trainer the schedule's closed form instead.  The state words are recomputed for t = steps_done + 1
        under the schedule, so a resumed run is bitwise the uninterrupted one."""
        params = list(self.model.parameters())
        off = {id(p): o for p, o in self.model._slots}
        group = sd["param_groups"][0]
        if any(group.get(k) for k in ("amsgrad", "maximize")):
            raise ValueError("FusedTrainer implements Adam / AdamW (no amsgrad / maximize)")
        if group.get("weight_decay") and not group.get("decoupled_weight_decay"):
            raise ValueError("FusedTrainer implements decoupled weight decay (AdamW) only: the coupled, L2-style weight_decay of "
                             "torch.optim.Adam is refused")
        if list(group["params"]) != list(range(len(params))):
            raise ValueError("optimizer state does not cover this model's parameters in order")
        steps = {int(float(st["step"])) for st in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError("parameters with different step counts")
        if "srfrd" in sd:          # (a torch.optim.Adam state carries no loss: it may continue under any)
            saved = (sd["srfrd"] or {}).get("loss", {"kind": "bce"})
            mine = self._loss_signature() if self.loss_kind != "bce" else {"kind": "bce"}
            if saved != mine:
                raise ValueError(f"optimizer state was saved under loss {saved}; this trainer trains {mine}")
        lr, betas, eps = float(group["lr"]), (float(group["betas"][0]), float(group["betas"][1])), float(group["eps"])
        # the options: the saved ones, else (a torch optimizer's state) this trainer's own; validated before anything changes
        extra = sd.get("srfrd") or {}
        mine = self.opts
        sch = extra.get("schedule") or ({"kind": LR_SCHEDULES[mine.schedule], "warmup_steps": int(mine.warmup_steps),
                                         "total_steps": int(mine.total_steps), "final_lr_ratio": float(mine.final_ratio)}
                                        if mine is not None else {"kind": "constant"})
        max_norm = extra["max_grad_norm"] if "schedule" in extra or "max_grad_norm" in extra else self.max_norm
        opts, max_norm = _optim_config(lr, betas, float(group.get("weight_decay") or 0.0), max_norm, sch["kind"],
                                       sch.get("warmup_steps", 0), sch.get("total_steps"), sch.get("final_lr_ratio", 0.0), self.group)
        # (a lazy trainer takes a dense trainer's checkpoint and the other way round - unless it carries an option lazy Adam refuses)
        _lazy_config(self.lazy_table, self.loss_kind, self.group, False, self.l2, float(group.get("weight_decay") or 0.0), max_norm)
        dev = self.flat.device
        if max_norm is not None and self.max_norm is None:
            self.norm_partial = torch.zeros(_lib.GRAD_NORM_PARTIALS, device=dev, dtype=torch.float64)
            self.clip = torch.zeros(2, device=dev, dtype=torch.float32)
        self.lr, self.betas, self.eps, self.opts, self.max_norm = lr, betas, eps, opts, max_norm
        m = torch.zeros(self.ex.n_pad if self.mode == "sharded" else self.n_flat, device=dev, dtype=torch.float32)
        v = torch.zeros_like(m)
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            if st is None:
                continue                                   # (a parameter that never received a gradient: zero moments)
            o, n = off[id(p)], p.numel()
            m[o:o + n] = st["exp_avg"].to(device=dev, dtype=torch.float32).reshape(-1)
            v[o:o + n] = st["exp_avg_sq"].to(device=dev, dtype=torch.float32).reshape(-1)
        if self.mode == "sharded":
            self.m.copy_(m[self.ex.i0:self.ex.i1]); self.v.copy_(v[self.ex.i0:self.ex.i1])
        else:
            self.m.copy_(m); self.v.copy_(v)
        self.steps_done = steps.pop() if steps else 0
        seed = int(extra.get("seed", int(self.state[1].item()))) & 0x7FFFFFFF
        self.state.zero_()                                 # (ticket words of the fused tail included)
        self.state[0] = self.steps_done
        self.state[1] = seed
        # step size, bias correction and dropout seed of the NEXT step (t = steps_done + 1), as after an uninterrupted run.
        # (The captured graphs bake lr / betas in as launch arguments: they are re-captured.)
        self._step_begin()
        self._graphs = None
        self._fresh = False

    def _check_slot(self, slot: int = 0):
        ids, kind = self.ids_ring[slot], self.lay.kind
        n = self.B * self.L
        embeds_fake = kind in (1, 2)
        call("srfrd_check_ids", item_a=ids[0], item_b=ids[2], item_c=ids[4], fake_a=ids[1] if embeds_fake else None,
             fake_b=ids[3] if kind == 2 else None, fake_c=ids[5] if kind == 2 else None, n=n, n_items=self.lay.n_items, fake_hi=2,
             err_word=self.err)

    def check(self):
        """Raise IndexError if a batch given to step() / step_packed() held an id outside the embedding tables (the
        kernels clamp such ids: memory stays safe, the step's result does not count).  Synchronises the device."""
        bits = int(self.err.item())
        if bits:
            self.err.zero_()
            raise IndexError("index out of range in self: a training batch held " + " and ".join(
                n for b, n in ((1, f"an item id outside [0, {self.lay.n_items}]"), (2, "a fake / review id outside [0, 2]"))
                if bits & b))

    def step_packed(self, batch6: torch.Tensor) -> torch.Tensor:
        """One train step on a packed int64 (6, B, L) tensor [seq, rsq, pos, prs, neg, nrs]; returns the device loss.
        ("token_softmax" / "gbce": the negatives are ``neg_ring[0]`` / ``log_q_ring[0]`` as the caller left them.)"""
        self.ids.copy_(batch6, non_blocking=True)
        self._check_slot(0)
        return self._run()

    def step(self, user_ids, input_ids, fake_ids, positive_ids, positive_fake_ids, negative_ids, negative_fake_ids, log_q=None):
        """Same argument order as the reference model call at trainer.py:30 (``user_ids`` is unused there too).  Under a
        cross-entropy loss ``negative_ids`` / ``negative_fake_ids`` are not read and may be None.  Under "token_softmax" /
        "gbce" ``negative_ids`` is the (B, L, K) negative plane and ``log_q`` its (B, L, K) float32 log-Q (None: zeros); they
        are copied into slot 0 of ``neg_ring`` / ``log_q_ring``, and an id outside [0, n_items] is recorded for ``check()``."""
        if self.token:
            shape = (self.B, self.L, self.K)
            if negative_ids is None or tuple(negative_ids.shape) != shape:
                raise ValueError(f"loss={self.loss_kind!r}: negative_ids must be a {shape} integer tensor")
            if log_q is not None and (tuple(log_q.shape) != shape or log_q.dtype != torch.float32):
                raise ValueError(f"log_q must be a float32 tensor of shape {shape} or None")
            self.neg_ring[0].copy_(negative_ids, non_blocking=True)
            if log_q is None:
                self.log_q_ring[0].zero_()
            else:
                self.log_q_ring[0].copy_(log_q, non_blocking=True)
            neg = self.neg_ring[0]
            self.err.bitwise_or_(((neg < 0) | (neg > self.lay.n_items)).any().to(torch.int32))      # (no synchronisation)
            negative_ids = negative_fake_ids = None
        elif log_q is not None:
            raise ValueError("log_q belongs to loss='token_softmax'")
        for k, t in enumerate((input_ids, fake_ids, positive_ids, positive_fake_ids, negative_ids, negative_fake_ids)):
            if t is None and k >= 4 and self.loss_kind != "bce":
                self.ids[k].zero_()
                continue
            self.ids[k].copy_(t, non_blocking=True)
        self._check_slot(0)
        return self._run()

    def step_slot(self, slot: int) -> torch.Tensor:
        """One train step on input slot `slot` of `ids_ring` (already filled by the caller, stream-ordered before this
        call): the zero-copy form of step_packed().  The slot's ids are the producer's responsibility (DeviceSampler
        checks its dataset against the model once, at construction); call ``_check_slot(slot)`` + ``check()`` to
        validate a hand-filled slot."""
        if not 0 <= slot < self.slots:
            raise IndexError(f"slot {slot} outside the ring of {self.slots}")
        return self._run(slot)

    def _run(self, slot: int = 0):
        if self.model.key_padding_mask != self._key_mask:
            raise RuntimeError("model.use_key_padding_mask() changed after this FusedTrainer was built (its launches carry the "
                               "layout's flags as they were): build a new trainer")
        if self.token:
            self._last_slot = slot
        if not self._fresh:
            self.refresh()
        if not self.use_graph:
            self._enqueue_step(slot)
        else:
            if not self.captured:
                self._capture()
            self._replay(slot)
        self.steps_done += 1
        return self.loss
