"""The launches of the three fused loss heads over the item table, written once  (DESIGN sections 12-15).

    XENT    full-catalog softmax                     srfrd_xent_fwd / _bwd     head arguments: none
    SXENT   sampled softmax, shared negatives (K,)   srfrd_sxent_fwd / _bwd    (negatives, log_q, remove_hits)
    TNEG    K negatives per position (B, L, K)       srfrd_tneg_fwd / _bwd     (negatives, log_q, objective, beta, remove_hits)

The C entry points of a head differ from one another in two places only, and a ``Head`` names both.  Between the targets and
the lse / shape arguments sit the head's own arguments (none, or negatives, log_q, K and the scalars in the order above).
Between d_hidden and the workspace sits the table gradient in one of three forms: a dense (n_items + 1, d_item) write with
an accumulate flag (XENT); K + T contribution rows and their item keys, summed per item by srfrd_table_reduce (SXENT); or
T (1 + K) coefficients and keys, summed per item as coef * hidden[t] by srfrd_table_reduce_rank1 (TNEG).  Both reduces run
over a stable sort of the keys, so every item's rows are added in list order: bitwise reproducible.  ``table_mixed`` is the
reduce of a list that holds both full rows and rank-1 rows (srfrd_table_reduce_mixed): FusedTrainer's token-negatives step.

``launch_fwd`` / ``launch_bwd`` are what the ``srfrd::{xent,sxent,tneg}_{fwd,bwd}`` library ops (ops.py), the modules'
autograd function (modules.py) and FusedTrainer's cross-entropy step (trainer.py) all call.  Every buffer they would
allocate may be handed in instead (a persistent-buffer step allocates nothing); tensors must be contiguous.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from ._lib import call, query


def table_dense(lay, hidden, K, rows, keys, ws, d_table):
    """the backward kernel wrote (or accumulated into) the dense table gradient itself"""
    return d_table


def _sorted_keys(lay, keys, d_table):
    skeys, order = torch.sort(keys, stable=True)
    if d_table is None:
        d_table = torch.zeros(lay.n_items + 1, lay.d_item, device=keys.device, dtype=torch.float32)
    return skeys, order, d_table


def table_rows(lay, hidden, K, rows, keys, ws, d_table):
    """every item's contribution rows (its negative slots in slot order, then its target tokens in position order) summed in
    that fixed order"""
    skeys, order, d_table = _sorted_keys(lay, keys, d_table)
    call("srfrd_table_reduce", sorted_keys=skeys, order=order, table_contrib=rows, n=skeys.numel(), d_item=lay.d_item,
         grad_table=d_table)
    return d_table


def table_rank1(lay, hidden, K, rows, keys, ws, d_table):
    """every item's rank-1 rows coef * hidden[t] summed in list order (position-major, the target before its negatives)"""
    skeys, order, d_table = _sorted_keys(lay, keys, d_table)
    call("srfrd_table_reduce_rank1", sorted_keys=skeys, order=order, contrib_coef=rows, hidden=hidden, d_out=lay.d_out,
         rows_per_token=1 + K, n=skeys.numel(), d_item=lay.d_item, grad_table=d_table, workspace=ws, ws_floats=ws.numel())
    return d_table


def mixed_workspace(n, d_item):
    """floats of workspace srfrd_table_reduce_mixed needs for a list of n entries (0: it refuses them)"""
    return int(query("srfrd_table_reduce_mixed_workspace_floats", n=int(n), d_item=int(d_item)))


def table_mixed(lay, hidden, K, full_rows, coef, keys, ws, d_table, sorted_pair=None):
    """one table gradient from two kinds of rows (a train step: the encoder backward's full rows, then the TNEG head's
    rank-1 list): ``keys`` is [the keys of ``full_rows`` (n_rows, d_item) | the keys of ``coef``], stable-sorted here
    (``sorted_pair``: the (sorted keys, order) of a stable sort the caller has made already); per item the full rows are
    summed first, in row order, then the rank-1 rows coef * hidden[t] in list order.  The sizes the kernel indexes by are
    checked here: it reads hidden[(e - n_rows) // (1 + K)] for every list entry e >= n_rows."""
    n_rows = 0 if full_rows is None else full_rows.shape[0]
    n_coef = 0 if coef is None else coef.numel()
    n = keys.numel()
    if n != n_rows + n_coef:
        raise ValueError(f"{n} keys for {n_rows} full rows and {n_coef} rank-1 rows")
    if full_rows is not None and (full_rows.dim() != 2 or full_rows.shape[1] != lay.d_item or not full_rows.is_contiguous()):
        raise ValueError(f"full_rows must be a contiguous (n_rows, {lay.d_item}) tensor")
    if n_coef and (hidden.shape[-1] != lay.d_out or not hidden.is_contiguous() or
                   n_coef > (hidden.numel() // lay.d_out) * (1 + K)):
        raise ValueError(f"{n_coef} rank-1 rows need ceil({n_coef} / {1 + K}) hidden rows of {lay.d_out}")
    if ws.numel() < mixed_workspace(n, lay.d_item) or mixed_workspace(n, lay.d_item) <= 0:
        raise ValueError(f"the workspace holds {ws.numel()} floats; a list of {n} entries needs "
                         f"{mixed_workspace(n, lay.d_item)} (0: refused)")
    if sorted_pair is None:
        skeys, order, d_table = _sorted_keys(lay, keys, d_table)
    else:
        skeys, order = sorted_pair
        if skeys.numel() != n or order.numel() != n or skeys.dtype != torch.int64 or order.dtype != torch.int64:
            raise ValueError(f"sorted_pair must be two int64 tensors of {n} elements")
    call("srfrd_table_reduce_mixed", sorted_keys=skeys, order=order, n=n, rows=full_rows, n_rows=n_rows, contrib_coef=coef,
         hidden=hidden if n_coef else None, d_out=lay.d_out, rows_per_token=1 + K, d_item=lay.d_item, grad_table=d_table,
         workspace=ws, ws_floats=ws.numel())
    return d_table


class Head(NamedTuple):
    fwd: str                        # the C entry points
    bwd: str
    n_neg: Optional[Callable]       # negatives tensor -> K (None: the head takes no arguments of its own)
    scalars: tuple                  # the C names of the head's scalar arguments, in the order `args` gives them
    workspace: Callable             # (layout, B, L, K) -> workspace floats
    grad: tuple                     # the C names of the backward's two table-gradient arguments
    rows: Optional[Callable]        # (layout, T, K) -> shape of the backward's contribution list (None: dense table gradient)
    finish: Callable                # table_dense | table_rows | table_rank1


XENT = Head("srfrd_xent_fwd", "srfrd_xent_bwd", None, (),
            lambda lay, B, L, K: query("srfrd_xent_workspace_floats", lay=lay, B=B, L=L),
            ("grad_table", "accumulate"), None, table_dense)
SXENT = Head("srfrd_sxent_fwd", "srfrd_sxent_bwd", lambda neg: neg.numel(), ("remove_hits",),
             lambda lay, B, L, K: query("srfrd_sxent_workspace_floats", lay=lay, B=B, L=L, K=K),
             ("table_contrib", "contrib_keys"), lambda lay, T, K: (K + T, lay.d_item), table_rows)
TNEG = Head("srfrd_tneg_fwd", "srfrd_tneg_bwd", lambda neg: neg.shape[2], ("objective", "beta", "remove_hits"),
            lambda lay, B, L, K: max(query("srfrd_tneg_workspace_floats", lay=lay, B=B, L=L, K=K), 1),
            ("contrib_coef", "contrib_keys"), lambda lay, T, K: (T * (1 + K),), table_rank1)


def _head_args(head, lay, table_ptr, hidden, targets, args, ws):
    """(negatives, log_q, *scalars) -> (K, the workspace, the named C arguments both directions of the head share)"""
    B, L = targets.shape
    named = dict(lay=lay, table=table_ptr, hidden=hidden, targets=targets, B=B, L=L)
    K = 0
    if head.n_neg is not None:
        negatives, log_q, *scalars = args
        K = head.n_neg(negatives)
        named.update(negatives=negatives, log_q=log_q, K=K)
        named.update(zip(head.scalars, (int(s) if isinstance(s, bool) else s for s in scalars)))
    if ws is None:
        ws = torch.empty(head.workspace(lay, B, L, K), device=hidden.device, dtype=torch.float32)
    named.update(workspace=ws, ws_floats=ws.numel())
    return K, ws, named


def launch_fwd(head: Head, lay, table_ptr, hidden, targets, args=(), *, out=None, ws=None):
    """the head's forward -> (token_loss (B, L), lse (B, L), stats {sum, count}); ``args``: the head's own arguments (see the
    module docstring); ``out``: those three tensors, ``ws``: the workspace, where the caller keeps them"""
    B, L = targets.shape
    f32 = dict(device=hidden.device, dtype=torch.float32)
    _, _, named = _head_args(head, lay, table_ptr, hidden, targets, args, ws)
    tl, lse, stats = out if out is not None else (torch.empty(B, L, **f32), torch.empty(B, L, **f32), torch.empty(2, **f32))
    call(head.fwd, **named, token_loss=tl, lse=lse, stats=stats)
    return tl, lse, stats


def launch_bwd(head: Head, lay, table_ptr, hidden, targets, args, lse, d_token_loss, *, d_hidden=None, ws=None, rows=None,
               keys=None, d_table=None, accumulate=False, finish=True):
    """the head's backward, then the head's table-gradient finisher -> (d_hidden (B, L, d_out), d_table (n_items + 1, d_item)).
    ``d_hidden``, ``ws``, ``rows`` / ``keys`` (the contribution list) and ``d_table`` (where the table gradient goes; a
    reducing finisher stores into it as it is) are the caller's buffers where given.  ``accumulate``: the dense form adds to
    ``d_table``.  ``finish=False`` leaves the contribution list unreduced (-> (d_hidden, None)): the caller merges it with
    rows of its own."""
    B, L = targets.shape
    f32 = dict(device=hidden.device, dtype=torch.float32)
    K, ws, named = _head_args(head, lay, table_ptr, hidden, targets, args, ws)
    if d_hidden is None:
        d_hidden = torch.empty(B, L, lay.d_out, **f32)
    if head.rows is None:
        if d_table is None:
            d_table = torch.empty(lay.n_items + 1, lay.d_item, **f32)
        grad = (d_table, int(accumulate))
    else:
        shape = head.rows(lay, B * L, K)
        if rows is None:
            rows = torch.empty(shape, **f32)
        if keys is None:
            keys = torch.empty(shape[0], device=hidden.device, dtype=torch.int64)
        grad = (rows, keys)
    call(head.bwd, **named, lse=lse, d_token_loss=d_token_loss, d_hidden=d_hidden, **dict(zip(head.grad, grad)))
    return d_hidden, (head.finish(lay, hidden, K, rows, keys, ws, d_table) if finish else None)
