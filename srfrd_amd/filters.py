"""Item filters for full-catalog ranking (include/srfrd_hip_filter.h): a large arbitrary subset of the catalog, shared by many
users - "in stock", "this category", "this tenant's slice" - as a packed bitmap over the item ids, one row per user group."""
from __future__ import annotations

import torch

from . import _lib


class ItemFilter:
    """``mask``: bool (or integer, nonzero = allowed) ``(n_items + 1,)`` or ``(G, n_items + 1)`` on any device: ``mask[g, i]``
    says whether the users of group g may be shown item i.  Packed once on ``device`` by ``srfrd_item_mask_pack``.

    ``words``    (G, W) int32 on ``device``: bit ``i & 31`` of word ``i >> 5`` is item i; the last word and the tail bits are 0
    ``n_groups`` G
    ``n_items``  the catalog the filter was built for
    ``counts``   (G,) int64 on the CPU: allowed ids per group (diagnostics)

    ``model.topk(..., allow=f, allow_group=g)`` and ``model.target_rank(..., allow=f, allow_group=g)`` rank over the allowed
    items only; ``allow_group`` (B,) int64 names each user's row and may be left out when G = 1."""

    def __init__(self, mask, n_items: int, device):
        mask = torch.as_tensor(mask)
        if mask.dim() == 1:
            mask = mask.unsqueeze(0)
        if mask.dim() != 2 or mask.shape[0] < 1 or mask.shape[1] != n_items + 1:
            raise ValueError(f"ItemFilter: the mask must be (n_items + 1,) or (G, n_items + 1) with n_items + 1 = {n_items + 1} "
                             f"(got shape {tuple(mask.shape)})")
        if mask.is_floating_point() or mask.is_complex():
            raise ValueError(f"ItemFilter: the mask must be bool or integer (got {mask.dtype})")
        if torch.device(device).type != "cuda":
            raise ValueError(f"ItemFilter: the filter is packed and read on a ROCm GPU (device 'cuda'), not on {device!r}")
        on = (mask != 0)
        self.n_items, self.n_groups = int(n_items), int(on.shape[0])
        self.counts = on.sum(1).to(torch.int64).cpu()
        bytes_ = on.to(device=device, dtype=torch.uint8).contiguous()
        n_words = _lib.query("srfrd_item_mask_words", n_rows=n_items + 1)
        self.words = torch.empty(self.n_groups, n_words, device=bytes_.device, dtype=torch.int32)
        _lib.call("srfrd_item_mask_pack", mask=bytes_, n_groups=self.n_groups, n_rows=n_items + 1, words=self.words)

    @classmethod
    def from_ids(cls, ids, n_items: int, device):
        """``ids``: one 1-D integer tensor of allowed ids per group (or a single tensor: one group); ids outside 0..n_items
        are dropped"""
        if isinstance(ids, torch.Tensor):
            ids = [ids]
        mask = torch.zeros(len(ids), n_items + 1, dtype=torch.bool)
        for g, row in enumerate(ids):
            row = torch.as_tensor(row).reshape(-1).to(torch.int64).cpu()
            mask[g, row[(row >= 0) & (row <= n_items)]] = True
        return cls(mask, n_items, device)

    def group_arg(self, allow_group, B: int, device):
        """``allow_group`` of a ranking call over a batch of B -> int64 (B,) on ``device``, or None (every user reads row 0)"""
        if allow_group is None:
            if self.n_groups > 1:
                raise ValueError(f"allow_group is required: the filter has {self.n_groups} groups")
            return None
        g = torch.as_tensor(allow_group)
        if g.dtype != torch.int64 or tuple(g.shape) != (B,):
            raise ValueError(f"allow_group must be an int64 tensor of shape ({B},) (got {g.dtype}, {tuple(g.shape)})")
        return g.to(device).contiguous()
