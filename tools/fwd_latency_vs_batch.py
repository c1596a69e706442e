#!/usr/bin/env python3
"""Latency of the fused forward against the number of sequences in flight (diagnostic; run on the GPU box).

Times srfrd_encoder_fwd at the C2 geometry (SASRec, 50 k items, seq_len 50) in its three modes and, in inference mode, for
batches of 64 .. 512 sequences.  The point it makes: up to 256 sequences (one workgroup per CU) the launch takes the same
~34 us - the time of ONE sequence's dependency chain (2 blocks x ~10 dependent GEMM / row-op stages) - and 512 sequences
(two workgroups per CU) take 1.45 x that.  At BASELINE's batch of 512 the chip holds two sequences per CU: throughput is
set by the length of that chain, not by matrix-pipe or HBM throughput.
"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import srfrd_amd
dev = "cuda"
torch.manual_seed(0)
m = srfrd_amd.SASRec(50000, 50, 50, 0.5, 2, 1, dev)
for _, p in m.named_parameters():
    if p.dim() >= 2:
        torch.nn.init.xavier_normal_(p.data)
m = m.to(dev)
_, seq, rsq, pos, prs, neg, nrs = srfrd_amd.synthetic_batch(50000, 50, 512, seed=1, device=dev)
ids = m._prep(seq, None, pos, None, neg, None)
def t(fn, n=200):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000
m.pack_weights()
from srfrd_amd import _lib
lay, flat = m.layout, m._flat
B, L = 512, 50
hidden = torch.empty(B, L, 50, device=dev); pl = torch.empty(B, L, device=dev); nl = torch.empty(B, L, device=dev)
sx = torch.empty(3, B, L, 50, device=dev); sh = torch.empty(2, B, L, 50, device=dev)
sa = torch.empty(_lib.query("srfrd_aux_floats", lay=lay, B=B, L=L), device=dev); lp = torch.empty(B, 3, device=dev)
def launch(save, p):
    ckpt = (sx, sh, sa) if save else (None, None, None)
    _lib.call("srfrd_encoder_fwd", **_lib.encoder_head((lay, flat), flat, m.n_table_pad, m._packed, (ids[0], None, ids[2], None, ids[4], None),
                                                       B, L, p, 0, (hidden, pl, nl, *ckpt), seed=7),
              loss_part=lp if save else None, scratch=None, scratch_floats=0, dbg=None, dbg_seq=0)
for name, save, p in (("train (checkpoints, dropout 0.5)", True, 0.5), ("checkpoints, no dropout", True, 0.0), ("inference (no checkpoints)", False, 0.0)):
    print(f"{name:36s} {t(lambda: launch(save, p)):7.1f} us")
for Bx in (64, 128, 256, 384, 512):
    B = Bx
    print(f"inference, B = {Bx}: {t(lambda: launch(False, 0.0)):7.1f} us")
