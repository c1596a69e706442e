"""Drop-in ``nn.Module`` surface of the reference model zoo, backed by the HIP kernels.

Same class names, positional constructor signatures, ``forward`` / ``predict`` signatures, attribute tree and
``state_dict`` keys as the reference (SRFR_model.py:53 SRFR, :154 SRFRN, :429 SRFU, :543/:553/:562 SRFU_B/F/R,
:572 SASRec).  The stock ``nn.Embedding`` / ``nn.LayerNorm`` / ``nn.MultiheadAttention`` /
``nn.Conv1d`` objects are kept ONLY as parameter containers (created in the reference's construction order, so a
given ``torch.manual_seed`` yields the same initial weights); none of their ``forward`` methods is ever called.
All arithmetic runs in ``libsrfrd_hip.so``; on a non-CUDA device or without the library, calls raise.
"""
from __future__ import annotations

import weakref

import torch
import torch.nn as nn

from . import _lib, loss_heads, ops
from ._lib import call, ptr


FLAT_SLACK = 4096        # floats of zero padding kept behind a model's flat parameter vector
# storage address -> the module whose flat parameter vector lives there (srfrd_amd.Adam asks which tensors the vector holds)
_FLAT_OWNERS: "weakref.WeakValueDictionary[int, nn.Module]" = weakref.WeakValueDictionary()


def flat_owner(storage_ptr: int):
    """The srfrd_amd module whose current flat parameter vector starts the storage at `storage_ptr`, or None."""
    m = _FLAT_OWNERS.get(storage_ptr)
    if m is None or m._flat is None or m._flat.untyped_storage().data_ptr() != storage_ptr:
        return None
    return m


def _ids(t, device, shape=None):
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.device != device or t.dtype != torch.int64 or not t.is_contiguous():
        t = t.to(device=device, dtype=torch.int64).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"id tensor has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class PointWiseFeedForward(nn.Module):
    """Parameter container for reference SRFR_model.py:36-51 (conv1 / conv2 with kernel_size=1)."""

    def __init__(self, in_channel, out_channel, pwff_dropout_rate):
        super().__init__()
        self.conv1 = nn.Conv1d(in_channel, out_channel, kernel_size=1)
        self.dropout1 = nn.Dropout(p=pwff_dropout_rate)
        self.relu = nn.ReLU()
        self.conv2 = nn.Conv1d(out_channel, out_channel, kernel_size=1)
        self.dropout2 = nn.Dropout(p=pwff_dropout_rate)


class SRFR_Embedding(nn.Module):
    """Parameter container for reference SRFR_model.py:6-15."""

    def __init__(self, item_number, item_embedding_size, fake_embedding_size, dropout_rate, maxlen, device):
        super().__init__()
        self.item_embed = nn.Embedding(item_number + 1, item_embedding_size, padding_idx=0)
        self.fake_embed = nn.Embedding(3, fake_embedding_size, padding_idx=0)   # 0 padding, 1 fake, 2 real
        self.pos_embed = nn.Embedding(maxlen, item_embedding_size)
        self.total_hiden_size = item_embedding_size + fake_embedding_size
        self.dropout = nn.Dropout(p=dropout_rate)
        self.device = device


class SRFU_Embedding(nn.Module):
    """Parameter container for reference SRFR_model.py:399-409."""

    def __init__(self, item_number, item_embedding_size, number_of_labels, dropout_rate, maxlen, device):
        super().__init__()
        self.item_embed = nn.Embedding(item_number + 1, item_embedding_size, padding_idx=0)
        self.user_label_embed = nn.Embedding(number_of_labels, item_embedding_size)
        self.pos_embed = nn.Embedding(maxlen, item_embedding_size)
        self.dropout = nn.Dropout(p=dropout_rate)
        self.device = device
        self.item_embedding_size = item_embedding_size
        self.number_of_labels = number_of_labels
        self.maxlen = maxlen

    def get_user_label_embed(self):
        return self.user_label_embed


OUT_KEYS = ("hidden", "pos_logits", "neg_logits", "save_x", "save_h1", "save_aux")      # what _launch_fwd returns, in order


class _EncoderFn(torch.autograd.Function):
    """forward() of the drop-in modules under autograd: the same two launches as the registered ``srfrd::encoder_fwd`` /
    ``srfrd::encoder_bwd`` custom ops (srfrd_amd/ops.py - dispatcher-visible, opcheck'ed, and what ``module.library_ops =
    True`` routes through), without the Python glue torch.library generates around a custom op's autograd (measured: ~300 us
    of host time per training step at C2, more than the kernels take).  Unused outputs hand back None instead of a zero
    tensor (``set_materialize_grads(False)``): the backward then knows no hidden-state gradient exists and its head runs
    over the sequence's own rows only."""

    @staticmethod
    def forward(ctx, model, p, seed, inp, fk, pos, pfk, neg, nfk, *params):
        out = model._launch_fwd(inp, fk, pos, pfk, neg, nfk, p, seed, True)
        ctx.model, ctx.meta = model, (p, seed)
        ctx.set_materialize_grads(False)
        hidden = out["hidden"]
        pl = out["pos_logits"] if pos is not None else hidden.new_empty(0)
        nl = out["neg_logits"] if neg is not None else hidden.new_empty(0)
        saved, ctx.id_present = ops.pack_saved((hidden, pl, nl, out["save_x"], out["save_h1"], out["save_aux"]),
                                           (inp, fk, pos, pfk, neg, nfk))
        ctx.save_for_backward(*saved)
        return hidden, pl, nl

    @staticmethod
    def backward(ctx, d_hidden, d_pl, d_nl):
        out, ids, upstream = ops.unpack_saved(ctx.saved_tensors, ctx.id_present, (d_hidden, d_pl, d_nl))
        gflat = ctx.model._launch_bwd(*ids, *ctx.meta, dict(zip(OUT_KEYS, out)), *upstream)
        return (None,) * 9 + ctx.model._grad_views(gflat)


class _LossHeadFn(torch.autograd.Function):
    """full_catalog_loss() / sampled_softmax_loss() / token_negatives_loss() under autograd: the launches of the registered
    ``srfrd::{xent,sxent,tneg}_fwd`` / ``_bwd`` ops (srfrd_amd/loss_heads.py) without torch.library's Python glue, as _EncoderFn
    does for the encoder.  ``head``: loss_heads.XENT / SXENT / TNEG; ``scalars``: its non-tensor arguments; ``ids``: () or
    (negatives, log_q).  The reduction is applied on the device from the forward's {sum, count}: no host synchronisation in
    either direction.  log_q is not differentiable."""

    @staticmethod
    def forward(ctx, model, head, reduction, scalars, hidden, table, targets, *ids):
        tl, lse, stats = loss_heads.launch_fwd(head, model.layout, ptr(table), hidden, targets, (*ids, *scalars))
        ctx.model, ctx.head, ctx.reduction, ctx.scalars = model, head, reduction, scalars
        ctx.save_for_backward(hidden, table, targets, lse, stats, *ids)
        if reduction == "none":
            return tl
        return stats[0].clone() if reduction == "sum" else stats[0] / stats[1]

    @staticmethod
    def backward(ctx, g):
        hidden, table, targets, lse, stats, *ids = ctx.saved_tensors
        if ctx.reduction == "none":
            d_tok = g.contiguous()
        else:
            d_tok = (g if ctx.reduction == "sum" else g / stats[1]).expand(targets.shape).contiguous()
        dh, de = loss_heads.launch_bwd(ctx.head, ctx.model.layout, ptr(table), hidden, targets, (*ids, *ctx.scalars), lse, d_tok)
        return (None,) * 4 + (dh, de, None) + (None,) * len(ids)


class _SRFRDBase(nn.Module):
    """Shared machinery: flat parameter storage, kernel launches, predict."""

    _kind = None

    # ---- construction helpers (same order as the reference constructors)
    def _build_blocks(self, hidden, num_blocks, num_heads, dropout_rate):
        for _ in range(num_blocks):
            self.attention_layernorms.append(nn.LayerNorm(hidden, eps=1e-8))
            self.attention_layers.append(nn.MultiheadAttention(hidden, num_heads, dropout_rate))
            self.forward_layernorms.append(nn.LayerNorm(hidden, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(hidden, hidden, dropout_rate))

    def _init_lists(self):
        self.attention_layernorms = nn.ModuleList()
        self.attention_layers = nn.ModuleList()
        self.forward_layernorms = nn.ModuleList()
        self.forward_layers = nn.ModuleList()

    def _finish(self, item_number, max_len, d_item, d_fake, n_labels, num_blocks, num_heads, dropout_rate):
        if not 1 <= int(num_blocks) <= _lib.MAX_BLOCKS:      # (here, not at the first make_layout: the kernels take no depth 0)
            raise ValueError(f"num_blocks must be 1 .. {_lib.MAX_BLOCKS}, got {num_blocks}")
        self._cfg = dict(kind=self._kind, n_items=item_number, max_len=max_len, d_item=d_item, d_fake=d_fake,
                         n_labels=n_labels, n_blocks=num_blocks, n_heads=num_heads)
        self.dropout_rate = float(dropout_rate)
        self._lay = None
        self._flat = None
        self._slots = None
        self._packed = None
        self._scratch = None
        self._err = None
        self._table16 = None     # bf16 shadow of the item table (use_bf16_table)
        self._lay16 = None
        # "lazy": every call launches srfrd_check_ids on its id tensors and check_ids() (called by evaluation(), or by
        # the user at any synchronisation point) raises; "eager": raise at the call itself like nn.Embedding does (one
        # host sync per call); None: no validation launch (the kernels still clamp ids, so memory stays safe)
        self.validate_ids = "lazy"

    # ---- layout / flat storage
    @property
    def layout(self):
        if self._lay is None:
            self._lay = _lib.make_layout(**self._cfg)
        return self._lay

    def _item_param(self):
        raise NotImplementedError

    def _dense_params(self):
        """[(parameter, dense offset)] in the canonical order of include/srfrd_hip.h."""
        raise NotImplementedError

    def _block_params(self, lay):
        out = []
        for i in range(lay.n_blocks):
            o, mha, ff = lay.blk[i], self.attention_layers[i], self.forward_layers[i]
            out += [(self.attention_layernorms[i].weight, o.ln1_w), (self.attention_layernorms[i].bias, o.ln1_b),
                    (mha.in_proj_weight, o.in_w), (mha.in_proj_bias, o.in_b),
                    (mha.out_proj.weight, o.out_w), (mha.out_proj.bias, o.out_b),
                    (self.forward_layernorms[i].weight, o.ln2_w), (self.forward_layernorms[i].bias, o.ln2_b),
                    (ff.conv1.weight, o.c1_w), (ff.conv1.bias, o.c1_b), (ff.conv2.weight, o.c2_w), (ff.conv2.bias, o.c2_b)]
        return out

    @property
    def n_table_pad(self):
        return (self.layout.n_table + 3) // 4 * 4

    @property
    def n_flat(self):
        return (self.n_table_pad + self.layout.n_dense + 3) // 4 * 4

    def flat_parameters(self):
        """The single fp32 vector [item table | pad | dense parameters] every nn.Parameter is a view of."""
        self._ensure_flat()
        return self._flat

    def _current_slots(self, table):
        """[(parameter, flat offset)] of the parameters the module tree holds NOW.  forward() asks on every call (a parameter or
        a submodule may have been replaced since the last one); walking the tree through nn.Module.__getattr__ costs ~60 us of
        host time per call (62 attribute lookups), so the (module path, name) of every slot is resolved once and each call
        follows the paths through the _modules / _parameters dictionaries - the objects found are always the current ones."""
        paths = getattr(self, "_slot_paths", None)
        if paths is not None:
            try:
                out = []
                for path, pname, off in paths:
                    m = self
                    for n in path:
                        m = m._modules[n]
                    out.append((m._parameters[pname], off))
                if out[0][0] is table:
                    return out
            except (KeyError, AttributeError):
                pass
        slots = [(table, 0)] + [(p, self.n_table_pad + off) for p, off in self._dense_params()]
        where = {}
        for mname, mod in self.named_modules():
            for pname, q in mod._parameters.items():
                if q is not None:
                    where.setdefault(id(q), (tuple(mname.split(".")) if mname else (), pname))
        try:
            self._slot_paths = [where[id(q)] + (off,) for q, off in slots]
        except KeyError:
            self._slot_paths = None
        return slots

    def _ensure_flat(self):
        lay = self.layout
        table = self._item_param()
        dev = table.device
        if dev.type != "cuda":
            raise RuntimeError("srfrd_amd modules compute only on a ROCm GPU (device 'cuda'); move the model with "
                               ".to('cuda'). There is no CPU fallback.")
        if lay.D > _lib.MAX_D:
            raise NotImplementedError(f"the fused MI355X kernels cover hidden width <= 64 (got width {lay.D})")
        slots = self._current_slots(table)
        flat = self._flat
        if flat is not None and flat.device == dev:
            base = flat.data_ptr()
            if all(p.data_ptr() == base + 4 * off and p.dtype == torch.float32 for p, off in slots):
                self._slots = slots
                if _FLAT_OWNERS.get(base) is not self:          # (a deep copy shares no storage with its original)
                    _FLAT_OWNERS[base] = self
                return
        # (a few KiB of zeroed slack behind the vector: the data-parallel all-gather pads it to world equal shards)
        self._flat_store = torch.zeros(self.n_flat + FLAT_SLACK, device=dev, dtype=torch.float32)
        flat = self._flat_store[:self.n_flat]
        covered = 0
        for p, off in slots:
            n = p.numel()
            flat[off:off + n].copy_(p.data.reshape(-1).to(device=dev, dtype=torch.float32))
            p.data = flat[off:off + n].view(p.shape)
            p.grad = None
            covered += n
        assert covered == lay.n_table + lay.n_dense, "parameter list does not match the dense layout"
        self._flat, self._slots = flat, slots
        _FLAT_OWNERS[flat.data_ptr()] = self

    # ---- bf16 item-table shadow (BASELINE configs[1] / [4] "bf16"; no reference counterpart: its table is fp32)
    def use_bf16_table(self, on: bool = True, auto_refresh: bool = True):
        """Gather item rows (embedding, pos / neg targets, predict / top-k candidates) from a bf16 shadow of the item
        table: half the gather bytes.  The parameter stays fp32 (state_dict, gradients, Adam unchanged); the shadow is
        rebuilt from it before every forward of the module path and rewritten by the fused optimizer in FusedTrainer.
        Forward values then carry bf16-rounded embeddings (parity is held against the oracle with ``table_bf16``).
        ``auto_refresh=False`` (frozen weights, e.g. serving / an evaluation loop): the module path stops re-deriving the
        shadow on every call (a pass over the whole table: 50 us at 1 M items); call ``refresh_bf16_table()`` yourself
        after changing the item embeddings."""
        self._ensure_flat()
        self._bf16_auto = bool(auto_refresh)
        if on:
            lay16 = _lib.Layout.from_buffer_copy(bytes(self.layout))      # (flags included: use_key_padding_mask)
            lay16.table_bf16 = 1
            self._lay16 = lay16
            self._table16 = torch.empty(self.layout.n_table, device=self._flat.device, dtype=torch.int16)
            self.refresh_bf16_table()
        else:
            self._lay16 = self._table16 = None
        return self

    @property
    def bf16_table(self) -> bool:
        return self._table16 is not None

    def refresh_bf16_table(self):
        if self._table16 is not None:
            if self._table16.device != self._flat.device:
                self._table16 = torch.empty(self.layout.n_table, device=self._flat.device, dtype=torch.int16)
            call("srfrd_table_to_bf16", src=self._flat, n=self.layout.n_table, out=self._table16)

    # ---- key-padding mask (the original SASRec's; no reference counterpart: it passes none, SRFR_model.py:112)
    def use_key_padding_mask(self, on: bool = True):
        """Mask every sequence's LEADING pads out of its attention keys (``srfrd_layout.flags``, include/srfrd_hip.h): a live
        position then attends to the history alone, so its output no longer depends on how much padding precedes it - the
        same user scores the same at any window that holds the history.  An id 0 behind the first item stays a key.
        Every path that takes the model's layout follows: forward / backward, predict, topk, target_rank, evaluation and
        srfrd_amd.Adam; a ``FusedTrainer`` reads the switch when it is built and refuses to step once it has changed.
        Not part of any ``state_dict``.  Off, or on a batch without pads: the unmasked results, bit for bit."""
        lay = self.layout
        bit = _lib.LAYOUT_MASK_PAD_KEYS
        lay.flags = (lay.flags | bit) if on else (lay.flags & ~bit)
        if self._lay16 is not None:
            self._lay16.flags = lay.flags
        return self

    @property
    def key_padding_mask(self) -> bool:
        return bool(self.layout.flags & _lib.LAYOUT_MASK_PAD_KEYS)

    def _table_args(self):
        """(layout, item-table pointer) as the gathering launchers take them: fp32 parameter, or the bf16 shadow"""
        if self._table16 is not None:
            return self._lay16, ptr(self._table16)
        return self.layout, ptr(self._flat)

    def pack_weights(self):
        """Refresh the MFMA-fragment-ordered copy of the encoder weights (srfrd_pack_weights) from the parameters (and the
        bf16 item-table shadow, when in use)."""
        lay, flat = self.layout, self._flat
        if getattr(self, "_bf16_auto", True):
            self.refresh_bf16_table()
        if self._packed is None or self._packed.device != flat.device:
            self._packed = torch.empty(_lib.query("srfrd_packed_floats", lay=lay), device=flat.device, dtype=torch.float32)
        call("srfrd_pack_weights", lay=lay, dense=_lib.dense_ptr(flat, self.n_table_pad), packed=self._packed, state=None,
             lr=0.0, beta1=0.0, beta2=0.0)
        return self._packed

    def _scratch_for(self, B, L, backward):
        """global workspace for sequences whose working set does not fit LDS (None when it does)."""
        need = _lib.scratch_floats(self.layout, B, L)[1 if backward else 0]
        if need == 0:
            return None, 0
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != self._flat.device:
            self._scratch = torch.empty(need, device=self._flat.device, dtype=torch.float32)
        return self._scratch, need

    # ---- launches
    def _enc_head(self, ids, dropout_p, seed, seq0, out):
        """_lib.encoder_head of this model for the id planes ``ids`` and the forward's outputs ``out`` (a dict by OUT_KEYS)"""
        B, L = ids[0].shape
        return _lib.encoder_head(self._table_args(), self._flat, self.n_table_pad, self._packed, ids, B, L, dropout_p, seq0,
                                 [out[k] for k in OUT_KEYS], seed=seed)

    def _launch_fwd(self, inp, fk, pos, pfk, neg, nfk, dropout_p, seed, save, seq0=0, dbg=None, dbg_seq=0, out=None):
        """``out``: the caller's output buffers by OUT_KEYS (None: allocated here, only those the call writes)"""
        lay = self.layout
        B, L = inp.shape
        if out is None:
            f32 = dict(device=inp.device, dtype=torch.float32)
            out = {"hidden": torch.empty(B, L, lay.d_out, **f32),
                   "pos_logits": torch.empty(B, L, **f32) if pos is not None else None,
                   "neg_logits": torch.empty(B, L, **f32) if neg is not None else None,
                   "save_x": torch.empty(B, lay.n_blocks + 1, L, lay.D, **f32) if save else None,
                   "save_h1": torch.empty(B, lay.n_blocks, L, lay.D, **f32) if save else None,
                   "save_aux": torch.empty(_lib.query("srfrd_aux_floats", lay=lay, B=B, L=L), **f32) if save else None}
        self.pack_weights()          # parameters may have been stepped since the last call
        scratch, n_scr = self._scratch_for(B, L, backward=False)
        call("srfrd_encoder_fwd", **self._enc_head((inp, fk, pos, pfk, neg, nfk), dropout_p, seed, seq0, out), loss_part=None,
             scratch=scratch, scratch_floats=n_scr, dbg=dbg, dbg_seq=int(dbg_seq))
        return out

    def _launch_fwd_last(self, inp, fk):
        """Eval-mode encoder state of the last position only, (B, 1, d_out): what predict() / topk() rank with."""
        B, L = inp.shape
        hidden = torch.empty(B, 1, self.layout.d_out, device=inp.device, dtype=torch.float32)
        self.pack_weights()
        scratch, n_scr = self._scratch_for(B, L, backward=False)
        head = self._enc_head((inp, fk, None, None, None, None), 0.0, 0, 0, dict.fromkeys(OUT_KEYS))
        call("srfrd_encoder_fwd_last", **{k: head[k] for k in _lib.ENCODER_HEAD[:6]}, B=B, L=L, hidden_last=hidden,
             scratch=scratch, scratch_floats=n_scr)
        return hidden

    def _launch_bwd(self, inp, fk, pos, pfk, neg, nfk, dropout_p, seed, out, d_hidden, d_pl, d_nl, seq0=0, dbg=None, dbg_seq=0):
        lay = self.layout
        B, L = inp.shape
        gflat = torch.zeros(self.n_flat, device=inp.device, dtype=torch.float32)
        n_slabs = _lib.query("srfrd_bwd_grid", lay=lay, B=B, L=L)
        slabs = torch.empty(n_slabs, lay.n_dense, device=inp.device, dtype=torch.float32)
        scratch, n_scr = self._scratch_for(B, L, backward=True)
        call("srfrd_encoder_bwd", **self._enc_head((inp, fk, pos, pfk, neg, nfk), dropout_p, seed, seq0, out),
             d_hidden=d_hidden, d_pos=d_pl, d_neg=d_nl, fused_bce=0, grad_table=gflat, table_contrib=None, grad_slabs=slabs,
             scratch=scratch, scratch_floats=n_scr, dbg=dbg, dbg_seq=int(dbg_seq))
        call("srfrd_reduce_dense", grad_slabs=slabs, n_slabs=n_slabs, n_dense=lay.n_dense,
             grad_dense=_lib.dense_ptr(gflat, self.n_table_pad), loss_part=None, B=B, stats=None, loss_out=None)
        return gflat

    def _validate(self, inp, fk, pos, pfk, neg, nfk):
        if not self.validate_ids:
            return
        self._err_word(inp.device)
        embeds_fake = self._kind in ("SRFR", "SRFRN")      # SRFU_* only count ids 1 / 2; SASRec ignores them
        call("srfrd_check_ids", item_a=inp, item_b=pos, item_c=neg, fake_a=fk if embeds_fake else None, fake_b=pfk, fake_c=nfk,
             n=inp.numel(), n_items=self.layout.n_items, fake_hi=2, err_word=self._err)
        if self.validate_ids == "eager":
            self.check_ids()

    def _err_word(self, dev):
        if self._err is None or self._err.device != dev:
            self._err = torch.zeros(1, device=dev, dtype=torch.int32)
        return self._err

    def check_ids(self):
        """Raise IndexError if any call since the last check saw an id outside the embedding tables (what the
        reference's nn.Embedding raises at the lookup).  Synchronises the device."""
        if self._err is None:
            return
        bits = int(self._err.item())
        if bits:
            self._err.zero_()
            what = " and ".join(n for b, n in ((1, f"an item id outside [0, {self.layout.n_items}]"),
                                               (2, "a fake / review id outside [0, 2]")) if bits & b)
            raise IndexError(f"index out of range in self: {what} (ids were clamped; results of that call are invalid)")

    def _prep(self, input_ids, fake_ids, positive_ids, positive_fake_ids, negative_ids, negative_fake_ids):
        self._ensure_flat()
        dev = self._flat.device
        inp = _ids(input_ids, dev)
        if inp.dim() != 2:
            raise ValueError("input_ids must be (batch, seq_len)")
        if inp.shape[1] > self.layout.max_len:
            raise IndexError(f"sequence length {inp.shape[1]} exceeds max_len {self.layout.max_len}")
        shp = inp.shape
        fk = _ids(fake_ids, dev, shp)
        pos, neg = _ids(positive_ids, dev, shp), _ids(negative_ids, dev, shp)
        pfk = _ids(positive_fake_ids, dev, shp) if self._kind == "SRFRN" and pos is not None else None
        nfk = _ids(negative_fake_ids, dev, shp) if self._kind == "SRFRN" and neg is not None else None
        if self._kind.startswith("SRFU") and fk is None:
            raise ValueError("SRFU models need fake_ids to derive the user label")
        self._validate(inp, fk, pos, pfk, neg, nfk)
        return inp, fk, pos, pfk, neg, nfk

    def forward(self, user_ids, input_ids, fake_ids, positive_ids=None, positive_fake_ids=None, negative_ids=None,
                negative_fake_ids=None):
        """-> (hidden_state (B,L,d_out), pos_logits (B,L) | None, neg_logits (B,L) | None); ``user_ids`` is unused,
        exactly as in the reference (SRFR_model.py:92, :192, :473, :651)."""
        ids = self._prep(input_ids, fake_ids, positive_ids, positive_fake_ids, negative_ids, negative_fake_ids)
        p = self.dropout_rate if self.training else 0.0
        seed = self._next_seed() if p > 0 else 0
        grad = torch.is_grad_enabled() and any(q.requires_grad for q, _ in self._slots)
        if getattr(self, "library_ops", False):
            # torch.ops.srfrd.encoder_fwd (srfrd_amd/ops.py): the parameters are op inputs, its registered backward runs
            # srfrd::encoder_bwd and hands one gradient per parameter to autograd
            hidden, pl, nl, *_ = torch.ops.srfrd.encoder_fwd([q for q, _ in self._slots], *ids, ops.register_model(self), p, seed, 0, grad)
        elif grad:
            hidden, pl, nl = _EncoderFn.apply(self, p, seed, *ids, *[q for q, _ in self._slots])
        else:
            out = self._launch_fwd(*ids, p, seed, False)
            hidden, pl, nl = out["hidden"], out["pos_logits"], out["neg_logits"]
        return hidden, (pl if ids[2] is not None else None), (nl if ids[4] is not None else None)

    def _next_seed(self):
        """dropout seed of one forward: a host-side counter hashed with torch's seed (torch.manual_seed reproduces a run; no
        device random number, no host sync - the reference's nn.Dropout draws on the device stream without either)"""
        base = torch.initial_seed() & 0xFFFFFFFF
        if getattr(self, "_seed_base", None) != base:
            self._seed_base, self._seed_ctr = base, 0
        self._seed_ctr += 1
        h = (base * 0x9E3779B1 + self._seed_ctr * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 15
        return (h * 0x2C1B3C6D) & 0x7FFFFFFF

    def _grad_views(self, gflat):
        """one gradient view per parameter (order of _slots) of the flat gradient vector: a single split + reshapes"""
        if getattr(self, "_split_sizes", None) is None or self._split_n != gflat.numel():
            if any(b[1] < a[1] + a[0].numel() for a, b in zip(self._slots, self._slots[1:])):      # (never: the layout is ascending)
                return tuple(gflat[off:off + q.numel()].view(q.shape) for q, off in self._slots)
            sizes, keep, at = [], [], 0
            for q, off in self._slots:
                if off > at:
                    sizes.append(off - at); keep.append(False)
                sizes.append(q.numel()); keep.append(True)
                at = off + q.numel()
            if at < gflat.numel():
                sizes.append(gflat.numel() - at); keep.append(False)
            self._split_sizes, self._split_keep, self._split_n = sizes, keep, gflat.numel()
        parts = gflat.split_with_sizes(self._split_sizes)
        return tuple(t.view(q.shape) for (t, k), (q, _) in zip(((t, k) for t, k in zip(parts, self._split_keep) if k), self._slots))

    def _loss_inputs(self, name, hidden_state, positive_ids, reduction):
        """the checks the three loss methods share -> (contiguous hidden state, targets as int64 ids on the model's device)"""
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"reduction must be 'mean', 'sum' or 'none' (got {reduction!r})")
        self._ensure_flat()
        if self.bf16_table:
            raise RuntimeError(f"{name} needs the fp32 item table (use_bf16_table(False)); the bf16 form is not built")
        lay = self.layout
        dev = self._flat.device
        if hidden_state.dim() != 3 or hidden_state.shape[2] != lay.d_out or hidden_state.device != dev:
            raise ValueError(f"hidden_state must be the model's (B, L, {lay.d_out}) output on {dev}")
        if hidden_state.dtype != torch.float32:
            raise ValueError("hidden_state must be float32")
        return hidden_state.contiguous(), _ids(positive_ids, dev, hidden_state.shape[:2])

    def _check_item_ids(self, *ids):
        """validate_ids: one srfrd_check_ids launch per tensor of item ids; "eager" raises here (IndexError, one host sync)"""
        if not self.validate_ids:
            return
        for t in ids:
            call("srfrd_check_ids", item_a=t, item_b=None, item_c=None, fake_a=None, fake_b=None, fake_c=None, n=t.numel(),
                 n_items=self.layout.n_items, fake_hi=2, err_word=self._err_word(t.device))
        if self.validate_ids == "eager":
            self.check_ids()

    def full_catalog_loss(self, hidden_state, positive_ids, reduction="mean"):
        """Softmax cross-entropy of every target against the whole catalog: ``F.cross_entropy(logits[:, 1:], y - 1,
        ignore_index=-1, reduction=...)`` over the logits ``hidden_state[..., :d_item] @ item_table.T`` of the positions with
        ``positive_ids != 0``, without materialising them (``srfrd_xent_fwd`` / ``_bwd``).  ``hidden_state`` is the (B, L,
        d_out) first output of ``model(...)``; autograd carries the loss into it (and so through the encoder) and into the
        item table.  reduction: "mean" (over the targets; NaN when there are none, as torch gives), "sum" or "none" ((B, L),
        zeros at ignored positions).  SRFRN's fake slice adds one constant per row, which the softmax does not see: it
        gets a zero gradient."""
        h, y = self._loss_inputs("full_catalog_loss", hidden_state, positive_ids, reduction)
        self._check_item_ids(y)
        return _LossHeadFn.apply(self, loss_heads.XENT, reduction, (), h, self._slots[0][0], y)

    def sampled_softmax_loss(self, hidden_state, positive_ids, negative_ids, log_q=None, remove_accidental_hits=True,
                             reduction="mean"):
        """Sampled softmax cross-entropy with negatives shared by the whole batch (``srfrd_sxent_fwd`` / ``_bwd``): every
        position with ``positive_ids != 0`` is scored against its own target and the K items of ``negative_ids``,
        ``loss_t = logsumexp({s_t+} u {s_tj}) - s_t+`` with ``s_t+ = <h_t[:d_item], E[y_t]>`` and ``s_tj = <h_t[:d_item],
        E[n_j]> - log_q[j]``.  ``negative_ids`` (K,): id 0 marks an unused slot, duplicates count once each;
        ``log_q`` (K,) float32 or None (e.g. the second output of ``srfrd_amd.sample_negatives``), not differentiable;
        ``remove_accidental_hits`` drops, per token, the slots equal to its target.  The (tokens x (1 + K)) logits are
        never materialised.  reduction: "mean" (over the targets; NaN when there are none), "sum" or "none" ((B, L), zeros
        at ignored positions).  Autograd carries the loss into ``hidden_state`` and into the item table, whose gradient is
        reduced per item in a fixed order (bitwise reproducible).  SRFRN's fake slice gets a zero gradient, as in
        full_catalog_loss; ``negative_ids = arange(1, n_items + 1)`` without log_q is full_catalog_loss."""
        h, y = self._loss_inputs("sampled_softmax_loss", hidden_state, positive_ids, reduction)
        dev = h.device
        neg = torch.as_tensor(negative_ids)
        if neg.dim() != 1 or neg.numel() == 0 or neg.is_floating_point() or neg.is_complex() or neg.dtype == torch.bool:
            raise ValueError(f"negative_ids must be a non-empty 1-D integer tensor (got shape {tuple(neg.shape)}, {neg.dtype})")
        neg = _ids(neg, dev)
        K = neg.numel()
        if log_q is not None:
            if not isinstance(log_q, torch.Tensor) or log_q.dtype != torch.float32 or tuple(log_q.shape) != (K,):
                raise ValueError(f"log_q must be a float32 tensor of shape ({K},) or None")
            log_q = log_q.detach().to(dev).contiguous()
        self._check_item_ids(y, neg)
        return _LossHeadFn.apply(self, loss_heads.SXENT, reduction, (bool(remove_accidental_hits),), h, self._slots[0][0], y, neg, log_q)

    def token_negatives_loss(self, hidden_state, positive_ids, negative_ids, objective="softmax", log_q=None, beta=1.0,
                             remove_accidental_hits=True, reduction="mean"):
        """A loss with K negatives PER POSITION (``srfrd_tneg_fwd`` / ``_bwd``): ``negative_ids`` is (B, L, K), the form the
        reference's sampler draws in with K = 1 (``srfrd_amd.sample_token_negatives`` draws K).  Every position with
        ``positive_ids != 0`` is scored against its target, ``s_t+ = <h_t[:d_item], E[y_t]>``, and its own K items, ``s_tk =
        <h_t[:d_item], E[n_tk]>``; id 0 marks an unused slot, duplicates count once each, and ``remove_accidental_hits``
        drops the slots equal to the position's target.

        objective="softmax": ``loss_t = logsumexp({s_t+} u {s_tk - log_q[t, k]}) - s_t+``; ``log_q`` (B, L, K) float32 or
        None, not differentiable.  A position none of whose slots takes part has loss 0 and a zero gradient.  SRFRN's fake
        slice gets a zero gradient, as in full_catalog_loss.

        objective="gbce": ``loss_t = beta * softplus(-s_t+) + sum_k softplus(s_tk)``, gSASRec's generalised BCE (Petrov &
        Macdonald, RecSys 2023; ``srfrd_amd.gbce_beta`` gives beta from the sampling rate and the calibration t); beta = 1
        is plain BCE with K negatives, and with K = 1, ``remove_accidental_hits=False`` and reduction="mean" it is the
        reference's loss.  ``log_q`` must be None.  SRFRN is refused (ValueError): its logits include the fake slice, and
        BCE, unlike the softmax, is not invariant to that per-row term; that form is not built.

        The (tokens x (1 + K)) logits are never materialised.  reduction: "mean" (over the targets; NaN when there are
        none), "sum" or "none" ((B, L), zeros at ignored positions).  Autograd carries the loss into ``hidden_state`` and
        into the item table, whose gradient is reduced per item in a fixed order (bitwise reproducible)."""
        if objective not in _lib.TNEG_OBJECTIVES:
            raise ValueError(f"objective must be 'softmax' or 'gbce' (got {objective!r})")
        beta = float(beta)
        if not (beta >= 0.0) or beta == float("inf"):
            raise ValueError(f"beta must be finite and >= 0 (got {beta})")
        if objective == "gbce":
            if log_q is not None:
                raise ValueError("log_q belongs to the softmax objective: pass None with objective='gbce'")
            if self._kind == "SRFRN":
                raise ValueError("objective='gbce' is not built for SRFRN: its logits include the fake slice, which BCE "
                                 "(unlike the softmax) is not invariant to")
        h, y = self._loss_inputs("token_negatives_loss", hidden_state, positive_ids, reduction)
        dev = h.device
        neg = torch.as_tensor(negative_ids)
        B, L = hidden_state.shape[:2]
        if (neg.dim() != 3 or tuple(neg.shape[:2]) != (B, L) or neg.shape[2] == 0 or neg.is_floating_point() or neg.is_complex()
                or neg.dtype == torch.bool):
            raise ValueError(f"negative_ids must be a ({B}, {L}, K) integer tensor with K >= 1 (got shape {tuple(neg.shape)}, "
                             f"{neg.dtype})")
        neg = _ids(neg, dev)
        K = neg.shape[2]
        if B * L * (1 + K) >= 2 ** 31:
            raise ValueError(f"B * L * (1 + K) = {B * L * (1 + K)} must stay below 2^31")
        if log_q is not None:
            if not isinstance(log_q, torch.Tensor) or log_q.dtype != torch.float32 or tuple(log_q.shape) != (B, L, K):
                raise ValueError(f"log_q must be a float32 tensor of shape ({B}, {L}, {K}) or None")
            log_q = log_q.detach().to(dev).contiguous()
        self._check_item_ids(y, neg)
        scalars = (_lib.TNEG_OBJECTIVES[objective], beta, bool(remove_accidental_hits))
        return _LossHeadFn.apply(self, loss_heads.TNEG, reduction, scalars, h, self._slots[0][0], y, neg, log_q)

    def user_labels(self, fake_ids):
        """get_Labels (SRFU_*) / the predict-time label (SRFRN) as an int64 (B,) tensor, computed on device."""
        self._ensure_flat()
        fk = _ids(fake_ids, self._flat.device)
        kind = _lib.KINDS[self._kind] if self._kind != "SRFR" else _lib.KINDS["SRFRN"]
        return torch.ops.srfrd.user_labels(fk, kind)

    def _rank_inputs(self, input_ids, fake_ids, exclude=None):
        """what every ranking call starts from -> (last-position hidden state (B, 1, d_out), the user labels (SRFRN; else None),
        the exclusion triple of ops.excl_csr)"""
        with torch.no_grad():
            ids = self._prep(input_ids, fake_ids, None, None, None, None)
            hidden = self._launch_fwd_last(ids[0], ids[1])
        ulab = self.user_labels(ids[1]) if self._kind == "SRFRN" else None
        return hidden, ulab, ops.excl_csr(exclude, ids[0], hidden.shape[0], hidden.device)

    def predict(self, user_ids, input_ids, fake_ids, label):
        """reference predict(): logits of the candidate items ``label`` against the last position's state.
        ``label`` is (I_c,) shared by the batch (reference utils.py:589) or (B, I_c) per user (batched eval);
        returns (I_c,) for a single sequence, else (B, I_c) - the reference's ``.squeeze()`` behaviour."""
        hidden, ulab, _ = self._rank_inputs(input_ids, fake_ids)
        return self.candidate_logits(hidden, None, label, ulab).squeeze()

    def candidate_logits(self, hidden, fake_ids, cand, ulab=None):
        """``ulab``: SRFRN's user labels where the caller has them already (else derived from ``fake_ids``)"""
        cand = _ids(cand, hidden.device)
        if cand.dim() == 2 and cand.shape[0] != hidden.shape[0]:
            raise ValueError("per-user candidates must be (B, I_c)")
        if ulab is None and self._kind == "SRFRN":
            ulab = self.user_labels(fake_ids)
        self._check_item_ids(cand)
        return torch.ops.srfrd.predict_logits(hidden.contiguous(), cand.contiguous(), ulab, ops.register_model(self))

    def item_filter(self, mask):
        """``srfrd_amd.ItemFilter`` of ``mask`` ((n_items + 1,) or (G, n_items + 1)) for this model's catalog, on its device"""
        from .filters import ItemFilter
        return ItemFilter(mask, self.layout.n_items, self._item_param().device)

    def _allow_args(self, allow, allow_group, B, device, what):
        """the (words, group) pair of a filtered ranking call"""
        from .filters import ItemFilter
        if not isinstance(allow, ItemFilter):
            raise ValueError(f"{what}: allow must be an srfrd_amd.ItemFilter (got {type(allow).__name__})")
        if allow.n_items != self.layout.n_items:
            raise ValueError(f"{what}: the filter was built for n_items = {allow.n_items}, the model has {self.layout.n_items}")
        return allow.words, allow.group_arg(allow_group, B, device)

    def topk(self, user_ids, input_ids, fake_ids, k=10, exclude_pad=True, item_range=None, exclude=None, *, allow=None,
             allow_group=None):
        """Full-catalog ranking: (indices int64 (B,k), scores (B,k)); the (B, I) logits never reach HBM.
        ``exclude``: items never to return, per user - None, "input" (the ids of the user's input window), a (ptr, items)
        CSR tuple over the batch, or a list of B 1-D tensors.  Fewer than k rankable items leave trailing -1 / -inf slots.
        k <= 64 takes the threshold ranking built for evaluation; 64 < k <= srfrd_amd.TOPK_WIDE_MAX the wide one (the same
        scores and order law).
        ``allow``: an ``srfrd_amd.ItemFilter`` (``model.item_filter(mask)``) - only the items it allows are ranked, beside
        ``item_range``, ``exclude`` and ``exclude_pad``; ``allow_group`` int64 (B,): the filter row of each user (required when
        the filter has more than one group).  Any k in 1..TOPK_WIDE_MAX then takes the filtered ranking."""
        if not 1 <= k <= _lib.TOPK_WIDE_MAX:
            raise ValueError(f"topk: k = {k} is outside 1..srfrd_amd.TOPK_WIDE_MAX ({_lib.TOPK_WIDE_MAX})")
        if allow is None and allow_group is not None:
            raise ValueError("topk: allow_group needs allow")
        hidden, ulab, excl = self._rank_inputs(input_ids, fake_ids, exclude)
        lo, hi = item_range if item_range is not None else (0, self.layout.n_items + 1)
        if allow is not None:
            words, group = self._allow_args(allow, allow_group, hidden.shape[0], hidden.device, "topk")
            return tuple(torch.ops.srfrd.logits_topk_allow(hidden, ulab, ops.register_model(self), lo, hi, k, bool(exclude_pad), *excl,
                                                           words, group))
        if k > 64:
            return tuple(torch.ops.srfrd.logits_topk_wide(hidden, ulab, ops.register_model(self), lo, hi, k, bool(exclude_pad), *excl))
        if exclude is None:
            return tuple(torch.ops.srfrd.logits_topk(hidden, ulab, ops.register_model(self), lo, hi, k, bool(exclude_pad)))
        return tuple(torch.ops.srfrd.logits_topk_excl(hidden, ulab, ops.register_model(self), lo, hi, k, bool(exclude_pad), *excl))

    def target_rank(self, user_ids, input_ids, fake_ids, targets, exclude=None, item_range=None, exclude_pad=True, *, allow=None,
                    allow_group=None):
        """Full-catalog rank of ``targets`` (B,): int32 (B,) counts of the items in ``item_range`` (default: the whole
        catalog) that score strictly higher than the user's target, skipping the ``exclude`` set (as in ``topk``) and,
        with ``exclude_pad``, item 0.  The target itself is ranked even when it is excluded; ranks over disjoint item
        ranges add up.  ``rank < K`` is a hit at K; NDCG@K = 1 / log2(rank + 2).
        ``allow`` / ``allow_group``: as in ``topk`` - only allowed items are counted; a disallowed target is still ranked."""
        if allow is None and allow_group is not None:
            raise ValueError("target_rank: allow_group needs allow")
        hidden, ulab, excl = self._rank_inputs(input_ids, fake_ids, exclude)
        lo, hi = item_range if item_range is not None else (0, self.layout.n_items + 1)
        tg = _ids(targets, hidden.device).reshape(-1)
        if tg.numel() != hidden.shape[0]:
            raise ValueError("targets must hold one item id per user")
        if allow is not None:
            words, group = self._allow_args(allow, allow_group, hidden.shape[0], hidden.device, "target_rank")
            return torch.ops.srfrd.target_rank_allow(hidden, ulab, tg, ops.register_model(self), lo, hi, bool(exclude_pad), *excl,
                                                     words, group)
        return torch.ops.srfrd.target_rank(hidden, ulab, tg, ops.register_model(self), lo, hi, bool(exclude_pad), *excl)


class SRFR(_SRFRDBase):
    """reference SRFR_model.py:53-152: [item || fake] input channel, last_conv D -> d_item, item-only targets."""
    _kind = "SRFR"

    def __init__(self, item_number, max_len=20, item_embedding_size=50, fake_embedding_size=10, dropout_rate=0.5,
                 num_blocks=2, num_heads=1, device="cpu"):
        super().__init__()
        self.device = device
        self.total_hidden_size = item_embedding_size + fake_embedding_size
        self.embedding_layer = SRFR_Embedding(item_number, item_embedding_size, fake_embedding_size, dropout_rate,
                                              max_len, device)
        self._init_lists()
        self.last_conv = nn.Conv1d(self.total_hidden_size, item_embedding_size, kernel_size=1)
        self.last_layernorm = nn.LayerNorm(item_embedding_size, eps=1e-8)
        self._build_blocks(self.total_hidden_size, num_blocks, num_heads, dropout_rate)
        self._finish(item_number, max_len, item_embedding_size, fake_embedding_size, 0, num_blocks, num_heads, dropout_rate)

    def _item_param(self):
        return self.embedding_layer.item_embed.weight

    def _dense_params(self):
        lay = self.layout
        return ([(self.embedding_layer.pos_embed.weight, lay.off_pos), (self.embedding_layer.fake_embed.weight, lay.off_side)]
                + self._block_params(lay)
                + [(self.last_conv.weight, lay.off_lc_w), (self.last_conv.bias, lay.off_lc_b),
                   (self.last_layernorm.weight, lay.off_ll_w), (self.last_layernorm.bias, lay.off_ll_b)])


class SRFRN(_SRFRDBase):
    """reference SRFR_model.py:154-259: [item || fake] channel in and out; targets carry their fake embedding."""
    _kind = "SRFRN"

    def __init__(self, item_number, max_len=20, item_embedding_size=50, fake_embedding_size=10, dropout_rate=0.5,
                 num_blocks=2, num_heads=1, device="cpu"):
        super().__init__()
        self.device = device
        self.total_hidden_size = item_embedding_size + fake_embedding_size
        self.embedding_layer = SRFR_Embedding(item_number, item_embedding_size, fake_embedding_size, dropout_rate,
                                              max_len, device)
        self._init_lists()
        self.last_layernorm = nn.LayerNorm(self.total_hidden_size, eps=1e-8)
        self._build_blocks(self.total_hidden_size, num_blocks, num_heads, dropout_rate)
        self._finish(item_number, max_len, item_embedding_size, fake_embedding_size, 0, num_blocks, num_heads, dropout_rate)

    def _item_param(self):
        return self.embedding_layer.item_embed.weight

    def _dense_params(self):
        lay = self.layout
        return ([(self.embedding_layer.pos_embed.weight, lay.off_pos), (self.embedding_layer.fake_embed.weight, lay.off_side)]
                + self._block_params(lay)
                + [(self.last_layernorm.weight, lay.off_ll_w), (self.last_layernorm.bias, lay.off_ll_b)])


class SRFU(_SRFRDBase):
    """reference SRFR_model.py:429-540: per-user label embedding added to every position."""
    _kind = None

    def __init__(self, item_number, max_len=20, item_embedding_size=50, number_of_labels=2, dropout_rate=0.5,
                 num_blocks=2, num_heads=1, device="cpu"):
        super().__init__()
        self.device = device
        self.maxlen = max_len
        self.embedding_layer = SRFU_Embedding(item_number, item_embedding_size, number_of_labels, dropout_rate, max_len,
                                              device)
        self._init_lists()
        self.last_layernorm = nn.LayerNorm(item_embedding_size, eps=1e-8)
        self._build_blocks(item_embedding_size, num_blocks, num_heads, dropout_rate)
        self._finish(item_number, max_len, item_embedding_size, 0, number_of_labels, num_blocks, num_heads, dropout_rate)

    def get_Labels(self, fake_ids):
        if self._kind is None:      # the reference base class raises too (SRFR_model.py:467-471)
            raise TypeError("not implemented result")
        return self.user_labels(fake_ids)

    def _ensure_flat(self):
        if self._kind is None:
            raise TypeError("not implemented result")
        super()._ensure_flat()

    def _item_param(self):
        return self.embedding_layer.item_embed.weight

    def _dense_params(self):
        lay = self.layout
        return ([(self.embedding_layer.pos_embed.weight, lay.off_pos),
                 (self.embedding_layer.user_label_embed.weight, lay.off_side)]
                + self._block_params(lay)
                + [(self.last_layernorm.weight, lay.off_ll_w), (self.last_layernorm.bias, lay.off_ll_b)])


class SRFU_B(SRFU):
    """binary user label, reference SRFR_model.py:543-551 (more fake -> 2, more real -> 1, tie -> 2)."""
    _kind = "SRFU_B"


class SRFU_F(SRFU):
    """frequency user label = number of fake reviews, reference SRFR_model.py:553-560."""
    _kind = "SRFU_F"


class SRFU_R(SRFU):
    """ratio user label = floor(10 * fake / (fake + real)), reference SRFR_model.py:562-570."""
    _kind = "SRFU_R"


class SASRec(_SRFRDBase):
    """reference SRFR_model.py:572-681."""
    _kind = "SASRec"

    def __init__(self, item_number, maxlen=20, hidden_units=50, dropout_rate=0.5, num_blocks=2, num_heads=1, device="cpu"):
        super().__init__()
        self.item_num = item_number
        self.dev = device
        self.item_emb = nn.Embedding(self.item_num + 1, hidden_units, padding_idx=0)
        self.pos_emb = nn.Embedding(maxlen, hidden_units)
        self.emb_dropout = nn.Dropout(p=dropout_rate)
        self._init_lists()
        self.last_layernorm = nn.LayerNorm(hidden_units, eps=1e-8)
        self._build_blocks(hidden_units, num_blocks, num_heads, dropout_rate)
        self._finish(item_number, maxlen, hidden_units, 0, 0, num_blocks, num_heads, dropout_rate)

    def _item_param(self):
        return self.item_emb.weight

    def _dense_params(self):
        lay = self.layout
        return ([(self.pos_emb.weight, lay.off_pos)] + self._block_params(lay)
                + [(self.last_layernorm.weight, lay.off_ll_w), (self.last_layernorm.bias, lay.off_ll_b)])

    def log2feats(self, log_seqs):
        return self.forward(None, log_seqs, None)[0]

    def forward(self, user_ids, input_ids, fake_ids, positive_ids=None, positive_fake_ids=None, negative_ids=None,
                negative_fake_ids=None):
        return super().forward(user_ids, input_ids, None, positive_ids, None, negative_ids, None)

    def predict(self, user_ids, log_seqs, fake_ids, item_indices):
        return super().predict(user_ids, log_seqs, None, item_indices)
