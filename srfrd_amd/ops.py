"""PyTorch-ROCm custom ops (namespace ``srfrd::``) over the C ABI of include/srfrd_hip.h  (SURVEY.md 8b).

Every launcher the drop-in modules use is registered with ``torch.library`` - visible to the dispatcher as
``torch.ops.srfrd.<name>``, with a fake (meta) implementation for shape propagation and, for the encoder and the loss
heads, a registered backward - instead of being an opaque ctypes call from Python.  The six loss-head ops are thin: their
launches live in loss_heads.py (one ``launch_fwd`` / ``launch_bwd`` over a description per head, shared with the modules'
autograd function and FusedTrainer), and their fakes and autograd are registered once, by ``_register_head``:

    srfrd::encoder_fwd     embedding gather -> n_blocks x {LN, causal self-attention, FFN} -> last LN -> pos / neg logits
                           (reference SRFR_model.py:92-142 and twins); backward = srfrd::encoder_bwd + srfrd_reduce_dense
    srfrd::encoder_bwd     the fused backward (reference trainer.py:40)
    srfrd::predict_logits  candidate logits of predict() (SRFR_model.py:144-152 and twins)
    srfrd::logits_topk     full-catalog top-k over an item range, logits never in HBM
    srfrd::logits_topk_excl  the same with a per-user exclusion set (CSR over the batch) masked inside the ranking passes
    srfrd::logits_topk_wide  exact top-k for k up to 1024 (TOPK_WIDE_MAX), exclusion set optional
    srfrd::logits_topk_allow the same over the items an ItemFilter allows (srfrd::target_rank_allow: the target rank)
    srfrd::target_rank     full-catalog rank of a target item per user (strictly-greater count), exclusion set optional
    srfrd::topk_merge      merge of per-shard top-k lists
    srfrd::topk_merge_runs merge of per-shard lists of up to 1024 entries as sorted runs, read where they lie (strides)
    srfrd::user_labels     get_Labels (SRFR_model.py:546-570)
    srfrd::eval_rank       rank of candidate 0 (utils.py:589-597)
    srfrd::xent_fwd        full-catalog softmax cross-entropy per token (logits never in HBM); backward = srfrd::xent_bwd
    srfrd::xent_bwd        its gradients into the hidden state and the item table
    srfrd::sxent_fwd       sampled softmax cross-entropy with shared negatives per token; backward = srfrd::sxent_bwd
    srfrd::sxent_bwd       its gradients into the hidden state and the item table (deterministic table reduction)
    srfrd::tneg_fwd        sampled softmax / gBCE with K negatives per position, per token; backward = srfrd::tneg_bwd
    srfrd::tneg_bwd        its gradients into the hidden state and the item table (rank-1 contribution list, deterministic)

A model's geometry (the srfrd_layout descriptor, its flat parameter vector and packed weights) is not expressible as op
arguments one by one; the ops take ``model_key``, the registry key of a live model (``register_model``), and read
those from it.  The parameters themselves ARE op inputs (``params``), so autograd sees the dependence and
``encoder_fwd``'s registered backward returns one gradient per parameter.  There is no CPU implementation: the ops are
registered for device type "cuda" only and raise elsewhere.
"""
from __future__ import annotations

import weakref
from typing import List, Optional

import torch

from . import _lib, loss_heads
from ._lib import call, ptr, query

_MODELS: "weakref.WeakValueDictionary[int, torch.nn.Module]" = weakref.WeakValueDictionary()


def register_model(model) -> int:
    key = id(model)
    _MODELS[key] = model
    return key


def _model(key: int):
    m = _MODELS.get(key)
    if m is None:
        raise RuntimeError("srfrd op called with the key of a model that no longer exists")
    return m


# ------------------------------------------------------------------------------------------------ encoder forward
@torch.library.custom_op("srfrd::encoder_fwd", mutates_args=(), device_types="cuda")
def encoder_fwd(params: List[torch.Tensor], input_ids: torch.Tensor, fake_ids: Optional[torch.Tensor],
                pos_ids: Optional[torch.Tensor], pos_fake: Optional[torch.Tensor], neg_ids: Optional[torch.Tensor],
                neg_fake: Optional[torch.Tensor], model_key: int, dropout_p: float, seed: int, seq0: int,
                save: bool) -> List[torch.Tensor]:
    """-> [hidden, pos_logits, neg_logits, save_x, save_h1, save_aux] (absent outputs are empty tensors)."""
    m = _model(model_key)
    out = m._launch_fwd(input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, dropout_p, seed, save, seq0=seq0)
    # (a fresh empty tensor per absent output: custom-op returns may not alias one another)
    return [out["hidden"]] + [out[k] if out[k] is not None else out["hidden"].new_empty(0)
                              for k in ("pos_logits", "neg_logits", "save_x", "save_h1", "save_aux")]


@encoder_fwd.register_fake
def _(params, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, model_key, dropout_p, seed, seq0, save):
    m = _model(model_key)
    lay = m.layout
    B, L = input_ids.shape
    f = dict(device=input_ids.device, dtype=torch.float32)
    return [torch.empty(B, L, lay.d_out, **f), torch.empty(B, L, **f) if pos_ids is not None else torch.empty(0, **f),
            torch.empty(B, L, **f) if neg_ids is not None else torch.empty(0, **f),
            torch.empty(B, lay.n_blocks + 1, L, lay.D, **f) if save else torch.empty(0, **f),
            torch.empty(B, lay.n_blocks, L, lay.D, **f) if save else torch.empty(0, **f),
            torch.empty(query("srfrd_aux_floats", lay=lay, B=B, L=L), **f) if save else torch.empty(0, **f)]


# ------------------------------------------------------------------------------------------------ encoder backward
@torch.library.custom_op("srfrd::encoder_bwd", mutates_args=(), device_types="cuda")
def encoder_bwd(input_ids: torch.Tensor, fake_ids: Optional[torch.Tensor], pos_ids: Optional[torch.Tensor],
                pos_fake: Optional[torch.Tensor], neg_ids: Optional[torch.Tensor], neg_fake: Optional[torch.Tensor],
                model_key: int, dropout_p: float, seed: int, seq0: int, hidden: torch.Tensor, pos_logits: torch.Tensor,
                neg_logits: torch.Tensor, save_x: torch.Tensor, save_h1: torch.Tensor, save_aux: torch.Tensor,
                d_hidden: Optional[torch.Tensor], d_pos: Optional[torch.Tensor], d_neg: Optional[torch.Tensor]) -> torch.Tensor:
    """-> the flat gradient vector [item table | pad | dense] of the model's flat parameter layout."""
    m = _model(model_key)
    out = dict(hidden=hidden, pos_logits=pos_logits, neg_logits=neg_logits, save_x=save_x, save_h1=save_h1, save_aux=save_aux)
    return m._launch_bwd(input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, dropout_p, seed, out, d_hidden, d_pos, d_neg,
                         seq0=seq0)


@encoder_bwd.register_fake
def _(input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, model_key, dropout_p, seed, seq0, hidden, pos_logits, neg_logits,
      save_x, save_h1, save_aux, d_hidden, d_pos, d_neg):
    return torch.empty(_model(model_key).n_flat, device=hidden.device, dtype=torch.float32)


def pack_saved(out, ids):
    """the encoder autograd's saved tuple: the forward's six outputs, then the id planes that are present -> (it, which are)"""
    return (*out, *[t for t in ids if t is not None]), tuple(t is not None for t in ids)


def unpack_saved(saved, id_present, grads):
    """-> (the six outputs, the six id planes with None where absent, the upstream gradients that count, contiguous)"""
    rest = iter(saved[6:])
    ids = tuple(next(rest) if present else None for present in id_present)
    return saved[:6], ids, [None if g is None or t is None else g.contiguous() for g, t in zip(grads, (saved[0], ids[2], ids[4]))]


def _fwd_setup(ctx, inputs, output):
    (params, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, model_key, dropout_p, seed, seq0, save) = inputs
    if not save:
        raise RuntimeError("srfrd::encoder_fwd needs save=True to be differentiated (checkpoints for the backward)")
    # outputs and id tensors through save_for_backward (no output -> grad_fn -> ctx -> output cycle: the checkpoints - B x
    # (n_blocks + 1) x L x D floats - are released by refcount after the backward, and torch's version counters guard them);
    # only ints / flags stay on ctx
    saved, ctx.id_present = pack_saved(output, (input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake))
    ctx.meta = (model_key, dropout_p, seed, seq0, len(params))
    ctx.save_for_backward(*saved)


def _fwd_backward(ctx, grads):
    model_key, p, seed, seq0, n_params = ctx.meta
    m = _model(model_key)
    out, ids, upstream = unpack_saved(ctx.saved_tensors, ctx.id_present, grads)
    gflat = torch.ops.srfrd.encoder_bwd(*ids, model_key, p, seed, seq0, *out, *upstream)
    per_param = list(m._grad_views(gflat))
    assert len(per_param) == n_params
    return (per_param,) + (None,) * 11


encoder_fwd.register_autograd(_fwd_backward, setup_context=_fwd_setup)


# ------------------------------------------------------------------------------------------------ ranking side
@torch.library.custom_op("srfrd::user_labels", mutates_args=(), device_types="cuda")
def user_labels(fake_ids: torch.Tensor, kind: int) -> torch.Tensor:
    fk = fake_ids.contiguous()
    lab = torch.empty(fk.shape[0], device=fk.device, dtype=torch.int64)
    call("srfrd_user_labels", kind=kind, fake_ids=fk, B=fk.shape[0], L=fk.shape[1], labels=lab)
    return lab


@user_labels.register_fake
def _(fake_ids, kind):
    return torch.empty(fake_ids.shape[0], device=fake_ids.device, dtype=torch.int64)


def rank_head(m, hidden, user_label, item_range=None, exclude_pad=False, excl=None):
    """The named values srfrd_predict_logits, srfrd_logits_topk(_excl) and srfrd_target_rank share, of a model ``m`` (its
    ``_table_args()``, ``_flat``, ``n_table_pad``); ``item_range`` (lo, hi) and ``exclude_pad``: the three ranking calls';
    ``excl``: the exclusion triple of ``excl_csr``."""
    lay, tab = m._table_args()
    head = dict(lay=lay, item_table=tab, dense=_lib.dense_ptr(m._flat, m.n_table_pad), hidden=hidden, B=hidden.shape[0],
                L=hidden.shape[1], user_label=user_label)
    if item_range is not None:
        head.update(item_lo=item_range[0], item_hi=item_range[1], exclude_pad=1 if exclude_pad else 0)
    if excl is not None:
        head.update(excl_ptr=excl[0], excl_items=excl[1], max_row=excl[2])
    return head


def _rank_workspaces(hidden, k, n_rows, max_row):
    """(top-k workspace, exclusion workspace) of a ranking call for ``hidden``'s batch over ``n_rows`` items; None for None"""
    B = hidden.shape[0]
    sizes = (None if k is None else query("srfrd_topk_workspace_bytes", B=B, k=k, n_rows=n_rows),
             None if max_row is None else query("srfrd_excl_workspace_bytes", B=B, max_row=min(max_row, _lib.EXCL_CAP), n_rows=n_rows))
    return [None if n is None else torch.empty(max(n, 8), device=hidden.device, dtype=torch.uint8) for n in sizes]


def _topk_out(rows, k):
    return [torch.empty(rows.shape[0], k, device=rows.device, dtype=dt) for dt in (torch.int64, torch.float32)]


@torch.library.custom_op("srfrd::predict_logits", mutates_args=(), device_types="cuda")
def predict_logits(hidden: torch.Tensor, cand: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int) -> torch.Tensor:
    n_cand = cand.shape[-1]
    logits = torch.empty(hidden.shape[0], n_cand, device=hidden.device, dtype=torch.float32)
    call("srfrd_predict_logits", **rank_head(_model(model_key), hidden, user_label), cand=cand, n_cand=n_cand,
         cand_stride=0 if cand.dim() == 1 else cand.shape[1], logits=logits)
    return logits


@predict_logits.register_fake
def _(hidden, cand, user_label, model_key):
    return torch.empty(hidden.shape[0], cand.shape[-1], device=hidden.device, dtype=torch.float32)


@torch.library.custom_op("srfrd::logits_topk", mutates_args=(), device_types="cuda")
def logits_topk(hidden: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int, item_lo: int, item_hi: int, k: int,
                exclude_pad: bool) -> List[torch.Tensor]:
    ws, _ = _rank_workspaces(hidden, k, item_hi - item_lo, None)
    idx, val = _topk_out(hidden, k)
    call("srfrd_logits_topk", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi), exclude_pad=exclude_pad),
         k=k, topk_idx=idx, topk_val=val, workspace=ws)
    return [idx, val]


def excl_csr(exclude, input_ids: Optional[torch.Tensor], B: int, device):
    """an exclusion argument -> (excl_ptr int64 (B + 1), excl_items int32, max_row) on ``device``, or (None, None, 0).
    ``exclude``: None; "input" (the nonzero ids of each row of ``input_ids``); a (ptr, items) CSR pair as a tuple; a list of
    B 1-D integer tensors (one per row)."""
    if exclude is None:
        return None, None, 0
    if isinstance(exclude, str):
        if exclude != "input" or input_ids is None:
            raise ValueError('exclude must be None, "input", a (ptr, items) pair or a list of 1-D tensors')
        keep = input_ids != 0
        ptr_ = torch.zeros(B + 1, device=device, dtype=torch.int64)
        torch.cumsum(keep.sum(1), 0, out=ptr_[1:])
        return ptr_, input_ids[keep].to(torch.int32).contiguous(), int(input_ids.shape[1])
    if isinstance(exclude, tuple) and len(exclude) == 2:
        ptr_, items = (torch.as_tensor(x) for x in exclude)
    elif isinstance(exclude, list):
        if len(exclude) != B:
            raise ValueError(f"exclude: {len(exclude)} rows for a batch of {B}")
        rows = [torch.as_tensor(r).reshape(-1).to(torch.int64).cpu() for r in exclude]
        ptr_ = torch.zeros(B + 1, dtype=torch.int64)
        torch.cumsum(torch.tensor([r.numel() for r in rows], dtype=torch.int64), 0, out=ptr_[1:])
        items = torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64)
    else:
        raise ValueError('exclude must be None, "input", a (ptr, items) pair or a list of 1-D tensors')
    if ptr_.numel() != B + 1:
        raise ValueError(f"exclude: excl_ptr has {ptr_.numel()} entries, the batch needs {B + 1}")
    lens = torch.diff(ptr_.to(torch.int64).cpu())
    if bool((lens < 0).any()) or int(ptr_[0]) != 0 or int(ptr_[-1]) > items.numel():
        raise ValueError("exclude: malformed CSR (excl_ptr must start at 0, not decrease and end within excl_items)")
    max_row = int(lens.max()) if B > 0 else 0
    items = items.to(device=device, dtype=torch.int32)
    if items.numel() == 0:
        items = torch.zeros(1, device=device, dtype=torch.int32)
    return ptr_.to(device=device, dtype=torch.int64).contiguous(), items.contiguous(), max_row


@torch.library.custom_op("srfrd::logits_topk_excl", mutates_args=(), device_types="cuda")
def logits_topk_excl(hidden: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int, item_lo: int, item_hi: int, k: int,
                     exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor],
                     max_row: int) -> List[torch.Tensor]:
    ws, xws = _rank_workspaces(hidden, k, item_hi - item_lo, max_row if excl_ptr is not None else None)
    idx, val = _topk_out(hidden, k)
    call("srfrd_logits_topk_excl", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi),
                                                exclude_pad=exclude_pad, excl=(excl_ptr, excl_items, max_row)),
         k=k, topk_idx=idx, topk_val=val, workspace=ws, excl_workspace=xws)
    return [idx, val]


@torch.library.custom_op("srfrd::logits_topk_wide", mutates_args=(), device_types="cuda")
def logits_topk_wide(hidden: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int, item_lo: int, item_hi: int, k: int,
                     exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor],
                     max_row: int) -> List[torch.Tensor]:
    """srfrd_logits_topk_wide: 1 <= k <= _lib.TOPK_WIDE_MAX; ``excl_ptr`` None: no exclusion sets"""
    n_rows = item_hi - item_lo
    _, xws = _rank_workspaces(hidden, None, n_rows, max_row if excl_ptr is not None else None)
    n = query("srfrd_topk_wide_workspace_bytes", B=hidden.shape[0], k=k, n_rows=n_rows)
    ws = torch.empty(max(n, 8), device=hidden.device, dtype=torch.uint8)
    idx, val = _topk_out(hidden, k)
    call("srfrd_logits_topk_wide", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi),
                                                exclude_pad=exclude_pad, excl=(excl_ptr, excl_items, max_row)),
         k=k, topk_idx=idx, topk_val=val, workspace=ws, ws_bytes=n, excl_workspace=xws)
    return [idx, val]


def _allow_args(allow_words, allow_group):
    """the four filter arguments of srfrd_logits_topk_allow / srfrd_target_rank_allow from an ItemFilter's words (G, W) int32"""
    return dict(allow_words=allow_words, n_groups=allow_words.shape[0], words_per_group=allow_words.shape[1], allow_group=allow_group)


@torch.library.custom_op("srfrd::logits_topk_allow", mutates_args=(), device_types="cuda")
def logits_topk_allow(hidden: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int, item_lo: int, item_hi: int, k: int,
                      exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor], max_row: int,
                      allow_words: torch.Tensor, allow_group: Optional[torch.Tensor]) -> List[torch.Tensor]:
    """srfrd_logits_topk_allow: 1 <= k <= _lib.TOPK_WIDE_MAX over the items ``allow_words`` (an ItemFilter's packed rows) allows;
    ``allow_group`` int64 (B,) or None (row 0); ``excl_ptr`` None: no exclusion sets"""
    n_rows = item_hi - item_lo
    _, xws = _rank_workspaces(hidden, None, n_rows, max_row if excl_ptr is not None else None)
    n = query("srfrd_topk_allow_workspace_bytes", B=hidden.shape[0], k=k, n_rows=n_rows)
    ws = torch.empty(max(n, 8), device=hidden.device, dtype=torch.uint8)
    idx, val = _topk_out(hidden, k)
    call("srfrd_logits_topk_allow", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi),
                                                 exclude_pad=exclude_pad, excl=(excl_ptr, excl_items, max_row)),
         k=k, topk_idx=idx, topk_val=val, workspace=ws, ws_bytes=n, excl_workspace=xws, **_allow_args(allow_words, allow_group))
    return [idx, val]


for _op in (logits_topk, logits_topk_excl, logits_topk_wide, logits_topk_allow):
    _op.register_fake(lambda hidden, user_label, model_key, item_lo, item_hi, k, *rest: _topk_out(hidden, k))


@torch.library.custom_op("srfrd::target_rank", mutates_args=(), device_types="cuda")
def target_rank(hidden: torch.Tensor, user_label: Optional[torch.Tensor], targets: torch.Tensor, model_key: int, item_lo: int,
                item_hi: int, exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor],
                max_row: int) -> torch.Tensor:
    _, ws = _rank_workspaces(hidden, None, item_hi - item_lo, max_row if excl_ptr is not None else 0)
    rank = torch.empty(hidden.shape[0], device=hidden.device, dtype=torch.int32)
    targets = targets.to(device=hidden.device, dtype=torch.int64).contiguous()
    call("srfrd_target_rank", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi),
                                           exclude_pad=exclude_pad, excl=(excl_ptr, excl_items, max_row)),
         targets=targets, cut_k=10, rank=rank, metric_acc=None, workspace=ws)
    return rank


@target_rank.register_fake
def _(hidden, user_label, targets, model_key, item_lo, item_hi, exclude_pad, excl_ptr, excl_items, max_row):
    return torch.empty(hidden.shape[0], device=hidden.device, dtype=torch.int32)


@torch.library.custom_op("srfrd::target_rank_allow", mutates_args=(), device_types="cuda")
def target_rank_allow(hidden: torch.Tensor, user_label: Optional[torch.Tensor], targets: torch.Tensor, model_key: int, item_lo: int,
                      item_hi: int, exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor],
                      max_row: int, allow_words: torch.Tensor, allow_group: Optional[torch.Tensor]) -> torch.Tensor:
    """srfrd_target_rank_allow: ``target_rank`` over the items ``allow_words`` allows"""
    _, ws = _rank_workspaces(hidden, None, item_hi - item_lo, max_row if excl_ptr is not None else 0)
    rank = torch.empty(hidden.shape[0], device=hidden.device, dtype=torch.int32)
    targets = targets.to(device=hidden.device, dtype=torch.int64).contiguous()
    call("srfrd_target_rank_allow", **rank_head(_model(model_key), hidden, user_label, item_range=(item_lo, item_hi),
                                                 exclude_pad=exclude_pad, excl=(excl_ptr, excl_items, max_row)),
         targets=targets, cut_k=10, rank=rank, metric_acc=None, workspace=ws, **_allow_args(allow_words, allow_group))
    return rank


@target_rank_allow.register_fake
def _(hidden, user_label, targets, model_key, item_lo, item_hi, exclude_pad, excl_ptr, excl_items, max_row, allow_words, allow_group):
    return torch.empty(hidden.shape[0], device=hidden.device, dtype=torch.int32)


@torch.library.custom_op("srfrd::topk_merge", mutates_args=(), device_types="cuda")
def topk_merge(cand_idx: torch.Tensor, cand_val: torch.Tensor, k: int) -> List[torch.Tensor]:
    cand_idx, cand_val = cand_idx.contiguous(), cand_val.contiguous()
    B, n = cand_idx.shape
    idx, val = _topk_out(cand_idx, k)
    call("srfrd_topk_merge", cand_idx=cand_idx, cand_val=cand_val, B=B, n_cand=n, k=k, topk_idx=idx, topk_val=val)
    return [idx, val]


@topk_merge.register_fake
def _(cand_idx, cand_val, k):
    return _topk_out(cand_idx, k)


@torch.library.custom_op("srfrd::topk_merge_runs", mutates_args=(), device_types="cuda")
def topk_merge_runs(cand_idx: torch.Tensor, cand_val: torch.Tensor, k: int) -> List[torch.Tensor]:
    """srfrd_topk_merge_runs: ``cand_idx`` int64 / ``cand_val`` fp32 (n_lists, B, list_len), each list sorted by the order law
    (an unsorted one is sorted, ``path`` says so) -> [idx (B, k), val (B, k), path int32 (B,)].  The strides are read, so a view
    with innermost stride 1 (a ``permute`` of a (B, n_lists, list_len) tensor, a slice) merges where it lies."""
    if cand_idx.dim() != 3 or cand_idx.shape != cand_val.shape:
        raise ValueError("topk_merge_runs: cand_idx and cand_val must be (n_lists, B, list_len) tensors of one shape")
    if cand_idx.dtype != torch.int64 or cand_val.dtype != torch.float32:
        raise ValueError("topk_merge_runs: cand_idx must be int64 and cand_val float32")
    if cand_idx.stride(2) != 1 or cand_idx.stride() != cand_val.stride():
        cand_idx, cand_val = cand_idx.contiguous(), cand_val.contiguous()
    S, B, n = cand_idx.shape
    idx, val = _topk_out(cand_idx[0], k)
    path = torch.empty(B, device=cand_idx.device, dtype=torch.int32)
    # (a dimension of size 1 may carry any stride: give it the one a contiguous tensor would have)
    call("srfrd_topk_merge_runs", cand_idx=cand_idx, cand_val=cand_val, B=B, n_lists=S, list_len=n,
         user_stride=cand_idx.stride(1) if B > 1 else n, list_stride=cand_idx.stride(0) if S > 1 else n, k=k,
         topk_idx=idx, topk_val=val, path=path)
    return [idx, val, path]


@topk_merge_runs.register_fake
def _(cand_idx, cand_val, k):
    return _topk_out(cand_idx[0], k) + [torch.empty(cand_idx.shape[1], device=cand_idx.device, dtype=torch.int32)]


@torch.library.custom_op("srfrd::eval_rank", mutates_args=(), device_types="cuda")
def eval_rank(logits: torch.Tensor) -> torch.Tensor:
    logits = logits.contiguous()
    B, n = logits.shape
    rank = torch.empty(B, device=logits.device, dtype=torch.int32)
    call("srfrd_eval_rank", logits=logits, B=B, n_cand=n, rank=rank, metric_acc=None)
    return rank


@eval_rank.register_fake
def _(logits):
    return torch.empty(logits.shape[0], device=logits.device, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ the three loss heads
def _xent_table(m, table: torch.Tensor):
    if m.bf16_table:
        raise RuntimeError("full-catalog cross-entropy needs the fp32 item table: call use_bf16_table(False) first")
    lay = m.layout
    if table.dtype != torch.float32 or not table.is_contiguous() or tuple(table.shape) != (lay.n_items + 1, lay.d_item):
        raise ValueError("the item table must be the model's contiguous fp32 (n_items + 1, d_item) parameter")
    return lay, ptr(table)


def _contiguous(args):
    return tuple(a.contiguous() if isinstance(a, torch.Tensor) else a for a in args)


def _head_fwd(head, model_key, table, hidden, targets, *args):
    """-> [token_loss (B, L), lse (B, L), stats (2) = {sum, count}]"""
    lay, tab = _xent_table(_model(model_key), table)
    return list(loss_heads.launch_fwd(head, lay, tab, hidden.contiguous(), targets.contiguous(), _contiguous(args)))


def _head_bwd(head, model_key, table, lse, d_token_loss, hidden, targets, *args):
    """-> [d_hidden (B, L, d_out), d_table (n_items + 1, d_item)]"""
    lay, tab = _xent_table(_model(model_key), table)
    return list(loss_heads.launch_bwd(head, lay, tab, hidden.contiguous(), targets.contiguous(), _contiguous(args),
                                      lse.contiguous(), d_token_loss.contiguous()))


@torch.library.custom_op("srfrd::xent_fwd", mutates_args=(), device_types="cuda")
def xent_fwd(hidden: torch.Tensor, targets: torch.Tensor, table: torch.Tensor, model_key: int) -> List[torch.Tensor]:
    return _head_fwd(loss_heads.XENT, model_key, table, hidden, targets)


@torch.library.custom_op("srfrd::xent_bwd", mutates_args=(), device_types="cuda")
def xent_bwd(hidden: torch.Tensor, targets: torch.Tensor, table: torch.Tensor, lse: torch.Tensor, d_token_loss: torch.Tensor,
             model_key: int) -> List[torch.Tensor]:
    return _head_bwd(loss_heads.XENT, model_key, table, lse, d_token_loss, hidden, targets)


@torch.library.custom_op("srfrd::sxent_fwd", mutates_args=(), device_types="cuda")
def sxent_fwd(hidden: torch.Tensor, targets: torch.Tensor, negatives: torch.Tensor, log_q: Optional[torch.Tensor],
              table: torch.Tensor, remove_hits: bool, model_key: int) -> List[torch.Tensor]:
    return _head_fwd(loss_heads.SXENT, model_key, table, hidden, targets, negatives, log_q, remove_hits)


@torch.library.custom_op("srfrd::sxent_bwd", mutates_args=(), device_types="cuda")
def sxent_bwd(hidden: torch.Tensor, targets: torch.Tensor, negatives: torch.Tensor, log_q: Optional[torch.Tensor],
              table: torch.Tensor, remove_hits: bool, lse: torch.Tensor, d_token_loss: torch.Tensor,
              model_key: int) -> List[torch.Tensor]:
    return _head_bwd(loss_heads.SXENT, model_key, table, lse, d_token_loss, hidden, targets, negatives, log_q, remove_hits)


@torch.library.custom_op("srfrd::tneg_fwd", mutates_args=(), device_types="cuda")
def tneg_fwd(hidden: torch.Tensor, targets: torch.Tensor, negatives: torch.Tensor, log_q: Optional[torch.Tensor],
             table: torch.Tensor, objective: int, beta: float, remove_hits: bool, model_key: int) -> List[torch.Tensor]:
    """objective: _lib.TNEG_OBJECTIVES"""
    return _head_fwd(loss_heads.TNEG, model_key, table, hidden, targets, negatives, log_q, objective, beta, remove_hits)


@torch.library.custom_op("srfrd::tneg_bwd", mutates_args=(), device_types="cuda")
def tneg_bwd(hidden: torch.Tensor, targets: torch.Tensor, negatives: torch.Tensor, log_q: Optional[torch.Tensor],
             table: torch.Tensor, objective: int, beta: float, remove_hits: bool, lse: torch.Tensor, d_token_loss: torch.Tensor,
             model_key: int) -> List[torch.Tensor]:
    return _head_bwd(loss_heads.TNEG, model_key, table, lse, d_token_loss, hidden, targets, negatives, log_q, objective, beta,
                     remove_hits)


def _head_fwd_fake(hidden, targets, *rest):
    B, L = targets.shape
    f = dict(device=hidden.device, dtype=torch.float32)
    return [torch.empty(B, L, **f), torch.empty(B, L, **f), torch.empty(2, **f)]


def _register_head(fwd, bwd, i_table):
    """fakes and autograd of one head's op pair.  Both ops take (hidden, targets, [negatives, log_q,] table, *scalars, ...) with
    the table at ``i_table``; the forward ends in model_key, the backward in (lse, d_token_loss, model_key)."""
    def bwd_fake(*args):
        return [torch.empty_like(args[0]), torch.empty_like(args[i_table])]

    def setup_context(ctx, inputs, output):
        ctx.rest = inputs[i_table + 1:]                                   # (*scalars, model_key)
        ctx.save_for_backward(*inputs[:i_table + 1], output[1])

    def backward(ctx, grads):
        *tensors, lse = ctx.saved_tensors
        out = [None] * (len(tensors) + len(ctx.rest))
        if grads[0] is not None:
            out[0], out[i_table] = bwd(*tensors, *ctx.rest[:-1], lse, grads[0].contiguous(), ctx.rest[-1])
        return tuple(out)

    fwd.register_fake(_head_fwd_fake)
    bwd.register_fake(bwd_fake)
    fwd.register_autograd(backward, setup_context=setup_context)


_register_head(xent_fwd, xent_bwd, 2)
_register_head(sxent_fwd, sxent_bwd, 4)
_register_head(tneg_fwd, tneg_bwd, 4)


OPS = ("encoder_fwd", "encoder_bwd", "user_labels", "predict_logits", "logits_topk", "logits_topk_excl", "logits_topk_wide", "logits_topk_allow", "target_rank",
       "target_rank_allow", "topk_merge", "topk_merge_runs",
       "eval_rank", "xent_fwd", "xent_bwd", "sxent_fwd", "sxent_bwd", "tneg_fwd", "tneg_bwd")
