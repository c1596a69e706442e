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
    srfrd::target_rank     full-catalog rank of a target item per user (strictly-greater count), exclusion set optional
    srfrd::topk_merge      merge of per-shard top-k lists
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

import ctypes as C
import weakref
from typing import List, Optional

import torch

from . import _lib, loss_heads
from ._lib import check, ptr

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


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


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
            torch.empty(_lib.lib().srfrd_aux_floats(C.byref(lay), B, L), **f) if save else torch.empty(0, **f)]


# ------------------------------------------------------------------------------------------------ encoder backward
@torch.library.custom_op("srfrd::encoder_bwd", mutates_args=(), device_types="cuda")
def encoder_bwd(input_ids: torch.Tensor, fake_ids: Optional[torch.Tensor], pos_ids: Optional[torch.Tensor],
                pos_fake: Optional[torch.Tensor], neg_ids: Optional[torch.Tensor], neg_fake: Optional[torch.Tensor],
                model_key: int, dropout_p: float, seed: int, seq0: int, hidden: torch.Tensor, pos_logits: torch.Tensor,
                neg_logits: torch.Tensor, save_x: torch.Tensor, save_h1: torch.Tensor, save_aux: torch.Tensor,
                d_hidden: Optional[torch.Tensor], d_pos: Optional[torch.Tensor], d_neg: Optional[torch.Tensor]) -> torch.Tensor:
    """-> the flat gradient vector [item table | pad | dense] of the model's flat parameter layout."""
    m = _model(model_key)
    out = {"hidden": hidden, "pos_logits": pos_logits if pos_ids is not None else None,
           "neg_logits": neg_logits if neg_ids is not None else None, "save_x": save_x, "save_h1": save_h1, "save_aux": save_aux}
    return m._launch_bwd(input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, dropout_p, seed, out, d_hidden, d_pos, d_neg,
                         seq0=seq0)


@encoder_bwd.register_fake
def _(input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, model_key, dropout_p, seed, seq0, hidden, pos_logits, neg_logits,
      save_x, save_h1, save_aux, d_hidden, d_pos, d_neg):
    return torch.empty(_model(model_key).n_flat, device=hidden.device, dtype=torch.float32)


def _fwd_setup(ctx, inputs, output):
    (params, input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake, model_key, dropout_p, seed, seq0, save) = inputs
    if not save:
        raise RuntimeError("srfrd::encoder_fwd needs save=True to be differentiated (checkpoints for the backward)")
    # outputs and id tensors through save_for_backward (no output -> grad_fn -> ctx -> output cycle: the checkpoints - B x
    # (n_blocks + 1) x L x D floats - are released by refcount after the backward, and torch's version counters guard them);
    # only ints / flags stay on ctx
    ids = (input_ids, fake_ids, pos_ids, pos_fake, neg_ids, neg_fake)
    ctx.id_present = tuple(t is not None for t in ids)
    ctx.meta = (model_key, dropout_p, seed, seq0, len(params))
    ctx.save_for_backward(*output, *[t for t in ids if t is not None])


def _fwd_backward(ctx, grads):
    model_key, p, seed, seq0, n_params = ctx.meta
    m = _model(model_key)
    saved = ctx.saved_tensors
    hidden, pl, nl, sx, sh, sa = saved[:6]
    rest = iter(saved[6:])
    inp, fk, pos, pfk, neg, nfk = (next(rest) if present else None for present in ctx.id_present)
    d_hidden, d_pl, d_nl = grads[0], grads[1], grads[2]
    gflat = torch.ops.srfrd.encoder_bwd(inp, fk, pos, pfk, neg, nfk, model_key, p, seed, seq0, hidden, pl, nl, sx, sh, sa,
                                        None if d_hidden is None else d_hidden.contiguous(),
                                        None if (d_pl is None or pos is None) else d_pl.contiguous(),
                                        None if (d_nl is None or neg is None) else d_nl.contiguous())
    per_param = list(m._grad_views(gflat))
    assert len(per_param) == n_params
    return (per_param,) + (None,) * 11


encoder_fwd.register_autograd(_fwd_backward, setup_context=_fwd_setup)


# ------------------------------------------------------------------------------------------------ ranking side
@torch.library.custom_op("srfrd::user_labels", mutates_args=(), device_types="cuda")
def user_labels(fake_ids: torch.Tensor, kind: int) -> torch.Tensor:
    fk = fake_ids.contiguous()
    lab = torch.empty(fk.shape[0], device=fk.device, dtype=torch.int64)
    check(_lib.lib().srfrd_user_labels(kind, ptr(fk), fk.shape[0], fk.shape[1], ptr(lab), _stream()), "srfrd_user_labels")
    return lab


@user_labels.register_fake
def _(fake_ids, kind):
    return torch.empty(fake_ids.shape[0], device=fake_ids.device, dtype=torch.int64)


@torch.library.custom_op("srfrd::predict_logits", mutates_args=(), device_types="cuda")
def predict_logits(hidden: torch.Tensor, cand: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int) -> torch.Tensor:
    m = _model(model_key)
    lay, tab = m._table_args()
    B, L = hidden.shape[0], hidden.shape[1]
    stride = 0 if cand.dim() == 1 else cand.shape[1]
    n_cand = cand.shape[-1]
    logits = torch.empty(B, n_cand, device=hidden.device, dtype=torch.float32)
    check(_lib.lib().srfrd_predict_logits(C.byref(lay), tab, C.c_void_p(m._flat.data_ptr() + 4 * m.n_table_pad), ptr(hidden),
                                          B, L, ptr(cand), n_cand, stride, ptr(user_label), ptr(logits), _stream()),
          "srfrd_predict_logits")
    return logits


@predict_logits.register_fake
def _(hidden, cand, user_label, model_key):
    return torch.empty(hidden.shape[0], cand.shape[-1], device=hidden.device, dtype=torch.float32)


@torch.library.custom_op("srfrd::logits_topk", mutates_args=(), device_types="cuda")
def logits_topk(hidden: torch.Tensor, user_label: Optional[torch.Tensor], model_key: int, item_lo: int, item_hi: int, k: int,
                exclude_pad: bool) -> List[torch.Tensor]:
    m = _model(model_key)
    lay, tab = m._table_args()
    B, L = hidden.shape[0], hidden.shape[1]
    dev = hidden.device
    ws = torch.empty(max(_lib.lib().srfrd_topk_workspace_bytes(B, k, item_hi - item_lo), 8), device=dev, dtype=torch.uint8)
    idx = torch.empty(B, k, device=dev, dtype=torch.int64)
    val = torch.empty(B, k, device=dev, dtype=torch.float32)
    check(_lib.lib().srfrd_logits_topk(C.byref(lay), tab, C.c_void_p(m._flat.data_ptr() + 4 * m.n_table_pad), ptr(hidden), B, L,
                                       item_lo, item_hi, 1 if exclude_pad else 0, ptr(user_label), k, ptr(idx), ptr(val), ptr(ws),
                                       _stream()), "srfrd_logits_topk")
    return [idx, val]


@logits_topk.register_fake
def _(hidden, user_label, model_key, item_lo, item_hi, k, exclude_pad):
    B = hidden.shape[0]
    return [torch.empty(B, k, device=hidden.device, dtype=torch.int64), torch.empty(B, k, device=hidden.device, dtype=torch.float32)]


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
    m = _model(model_key)
    lay, tab = m._table_args()
    B, L = hidden.shape[0], hidden.shape[1]
    dev = hidden.device
    L_ = _lib.lib()
    ws = torch.empty(max(L_.srfrd_topk_workspace_bytes(B, k, item_hi - item_lo), 8), device=dev, dtype=torch.uint8)
    xws = None
    if excl_ptr is not None:
        xws = torch.empty(max(L_.srfrd_excl_workspace_bytes(B, min(max_row, _lib.EXCL_CAP), item_hi - item_lo), 8), device=dev,
                          dtype=torch.uint8)
    idx = torch.empty(B, k, device=dev, dtype=torch.int64)
    val = torch.empty(B, k, device=dev, dtype=torch.float32)
    check(L_.srfrd_logits_topk_excl(C.byref(lay), tab, C.c_void_p(m._flat.data_ptr() + 4 * m.n_table_pad), ptr(hidden), B, L,
                                    item_lo, item_hi, 1 if exclude_pad else 0, ptr(user_label), k, ptr(excl_ptr), ptr(excl_items),
                                    max_row, ptr(idx), ptr(val), ptr(ws), ptr(xws), _stream()), "srfrd_logits_topk_excl")
    return [idx, val]


@logits_topk_excl.register_fake
def _(hidden, user_label, model_key, item_lo, item_hi, k, exclude_pad, excl_ptr, excl_items, max_row):
    B = hidden.shape[0]
    return [torch.empty(B, k, device=hidden.device, dtype=torch.int64), torch.empty(B, k, device=hidden.device, dtype=torch.float32)]


@torch.library.custom_op("srfrd::target_rank", mutates_args=(), device_types="cuda")
def target_rank(hidden: torch.Tensor, user_label: Optional[torch.Tensor], targets: torch.Tensor, model_key: int, item_lo: int,
                item_hi: int, exclude_pad: bool, excl_ptr: Optional[torch.Tensor], excl_items: Optional[torch.Tensor],
                max_row: int) -> torch.Tensor:
    m = _model(model_key)
    lay, tab = m._table_args()
    B, L = hidden.shape[0], hidden.shape[1]
    dev = hidden.device
    L_ = _lib.lib()
    mr = min(max_row, _lib.EXCL_CAP) if excl_ptr is not None else 0
    ws = torch.empty(max(L_.srfrd_excl_workspace_bytes(B, mr, item_hi - item_lo), 8), device=dev, dtype=torch.uint8)
    rank = torch.empty(B, device=dev, dtype=torch.int32)
    targets = targets.to(device=dev, dtype=torch.int64).contiguous()
    check(L_.srfrd_target_rank(C.byref(lay), tab, C.c_void_p(m._flat.data_ptr() + 4 * m.n_table_pad), ptr(hidden), B, L,
                               item_lo, item_hi, 1 if exclude_pad else 0, ptr(user_label), ptr(targets), ptr(excl_ptr),
                               ptr(excl_items), max_row, 10, ptr(rank), None, ptr(ws), _stream()), "srfrd_target_rank")
    return rank


@target_rank.register_fake
def _(hidden, user_label, targets, model_key, item_lo, item_hi, exclude_pad, excl_ptr, excl_items, max_row):
    return torch.empty(hidden.shape[0], device=hidden.device, dtype=torch.int32)


@torch.library.custom_op("srfrd::topk_merge", mutates_args=(), device_types="cuda")
def topk_merge(cand_idx: torch.Tensor, cand_val: torch.Tensor, k: int) -> List[torch.Tensor]:
    cand_idx, cand_val = cand_idx.contiguous(), cand_val.contiguous()
    B, n = cand_idx.shape
    idx = torch.empty(B, k, device=cand_idx.device, dtype=torch.int64)
    val = torch.empty(B, k, device=cand_idx.device, dtype=torch.float32)
    check(_lib.lib().srfrd_topk_merge(ptr(cand_idx), ptr(cand_val), B, n, k, ptr(idx), ptr(val), _stream()), "srfrd_topk_merge")
    return [idx, val]


@topk_merge.register_fake
def _(cand_idx, cand_val, k):
    B = cand_idx.shape[0]
    return [torch.empty(B, k, device=cand_idx.device, dtype=torch.int64), torch.empty(B, k, device=cand_idx.device, dtype=torch.float32)]


@torch.library.custom_op("srfrd::eval_rank", mutates_args=(), device_types="cuda")
def eval_rank(logits: torch.Tensor) -> torch.Tensor:
    logits = logits.contiguous()
    B, n = logits.shape
    rank = torch.empty(B, device=logits.device, dtype=torch.int32)
    check(_lib.lib().srfrd_eval_rank(ptr(logits), B, n, ptr(rank), None, _stream()), "srfrd_eval_rank")
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


OPS = ("encoder_fwd", "encoder_bwd", "user_labels", "predict_logits", "logits_topk", "logits_topk_excl", "target_rank", "topk_merge",
       "eval_rank", "xent_fwd", "xent_bwd", "sxent_fwd", "sxent_bwd", "tneg_fwd", "tneg_bwd")
