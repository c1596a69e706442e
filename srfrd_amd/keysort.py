"""The device key sort (include/srfrd_hip_sort.h) as a plain function over torch tensors."""
from __future__ import annotations

import torch

from ._lib import call, query


def sort_workspace_bytes(n: int, key_max: int) -> int:
    """bytes of workspace ``sort_keys`` needs for ``n`` keys in [0, key_max]; raises where the entry point would refuse"""
    nb = int(query("srfrd_sort_keys_workspace_bytes", n=int(n), key_max=int(key_max)))
    if nb <= 0:
        raise ValueError(f"sort_keys: n = {n} must lie in [0, 2^31 - 1] and key_max = {key_max} in [0, 2^31 - 3]")
    return nb


def sort_keys(keys: torch.Tensor, key_max: int, out=None, workspace: torch.Tensor | None = None):
    """The stable sort of a contiguous int64 device tensor of item ids -> ``(sorted_keys, order)``, both int64 and shaped as
    ``keys``: with every key in [0, key_max], ``torch.sort(keys.reshape(-1), stable=True)`` bit for bit.  A negative key sorts
    ahead of key 0 and a key above ``key_max`` behind ``key_max``, each group in input order; ``sorted_keys`` holds the
    original values.  Kernel launches on the current stream and nothing else: a graph may hold the call at any length, given
    ``out=(sorted_keys, order)`` and a ``workspace`` (uint8, at least ``sort_workspace_bytes(keys.numel(), key_max)`` bytes,
    16-byte aligned) that outlive the graph; what is not handed in is allocated."""
    if keys.dtype != torch.int64 or not keys.is_cuda or not keys.is_contiguous():
        raise ValueError("sort_keys: keys must be a contiguous int64 device tensor")
    n = keys.numel()
    nb = sort_workspace_bytes(n, key_max)
    if out is None:
        out = (torch.empty_like(keys), torch.empty_like(keys))
    skeys, order = out
    for name, t in (("sorted_keys", skeys), ("order", order)):
        if t.dtype != torch.int64 or t.device != keys.device or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"sort_keys: out's {name} must be a contiguous int64 tensor of {n} elements on {keys.device}")
    if n == 0:                       # (an empty tensor has no address to hand over; the entry point would launch nothing)
        return skeys, order
    if workspace is None:
        workspace = torch.empty(nb, device=keys.device, dtype=torch.uint8)
    elif workspace.device != keys.device or not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nb:
        raise ValueError(f"sort_keys: workspace must be a contiguous tensor of at least {nb} bytes on {keys.device}")
    call("srfrd_sort_keys", keys=keys, n=n, key_max=int(key_max), sorted_keys=skeys, order=order, workspace=workspace,
         ws_bytes=workspace.numel() * workspace.element_size())
    return skeys, order
