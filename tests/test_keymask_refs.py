"""CPU side of the key-padding mask (``srfrd_layout.flags & SRFRD_LAYOUT_MASK_PAD_KEYS``; tests/keymask_refs.py is the
reference, tests/test_gpu_keymask.py the GPU side): the reference swaps in and out cleanly and is the unmasked oracle where
there is nothing to mask, a masked model's live rows do not depend on the padding in front of them (and an unmasked model's
do), the edges mean what the header says, every job of the gradient and the forward suite stays admissible under the masked
reference, and the C ABI carries the flag and refuses bits it does not know."""
import ctypes as C
import os
import re

import pytest
import torch

from oracle import srfrd_oracle as O
from srfrd_amd import _lib
from tests import fwd_refs as F
from tests import grad_refs as G
from tests import keymask_refs as K
from tests import test_encoder_entry_refusals as E
from tests.test_encoder_plan import N_CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_JOBS = [(c.id, mode) for c in G.ALL_CASES for mode in K.GRAD_MODES]
FWD_JOBS = [(c.id, mode) for c in G.ALL_CASES for mode in F.MODES]


def _sas(L=20, blocks=2, heads=1):
    from tests.gpu_util import random_sd
    cfg = O.Cfg("SASRec", G.I, L, 50, num_blocks=blocks, num_heads=heads)
    return cfg, random_sd(cfg, G.SD_SEED)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the reference swaps in and out; without pads it is the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_swap_is_undone_and_a_batch_without_pads_is_untouched():
    cfg, sd = _sas()
    g = torch.Generator().manual_seed(3)
    full = torch.randint(1, G.I + 1, (4, 20), generator=g)
    padded = full.clone()
    padded[0, :7] = 0
    padded[1, :19] = 0
    before = O.forward(cfg, sd, padded, None)[0]
    assert O.encoder_block is K._ORACLE_BLOCK
    for dt in (torch.float32, torch.float64):
        w = {k: v.to(dt) for k, v in sd.items()}
        plain = O.forward(cfg, w, full, None)[0]
        with K.masked():
            assert O.encoder_block is K.masked_encoder_block
            assert torch.equal(O.forward(cfg, w, full, None)[0], plain)            # nothing to mask: the same bits
    with K.masked():
        inside = O.forward(cfg, sd, padded, None)[0]
    assert O.encoder_block is K._ORACLE_BLOCK
    with pytest.raises(ZeroDivisionError):
        with K.masked():
            1 / 0
    assert O.encoder_block is K._ORACLE_BLOCK
    assert torch.equal(O.forward(cfg, sd, padded, None)[0], before)                # outside: the present bits
    assert float((inside - before)[0, 7:].abs().max()) > 1e-2                      # ... and inside the mask acts
    assert torch.equal(inside[0, :7], before[0, :7])                               # (pad rows: the last LayerNorm's bias)
    assert torch.equal(inside[2:], before[2:])


def test_the_masked_block_fills_the_oracles_taps():
    cfg, sd = _sas()
    seq = torch.randint(1, G.I + 1, (2, 20), generator=torch.Generator().manual_seed(4))
    seq[0, :5] = 0
    plain, masked = {}, {}
    O.forward(cfg, sd, seq, None, taps=plain)
    with K.masked():
        O.forward(cfg, sd, seq, None, taps=masked)
    assert set(plain) == set(masked)
    assert all(plain[k].shape == masked[k].shape for k in plain)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the window property, in fp64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.WINDOW_KINDS)
def test_live_rows_do_not_depend_on_the_window_under_the_mask_and_do_without_it(kind):
    (cl, sdl), (cs, sds) = K.window_weights(kind, 50, 20)
    long, short, ns = K.window_batch(50, 20)
    assert tuple(ns) == K.WINDOW_HISTORIES
    sdl, sds = ({k: v.double() for k, v in sd.items()} for sd in (sdl, sds))
    plain = K.window_difference(O.forward(cl, sdl, *long)[0], O.forward(cs, sds, *short)[0], ns)
    with K.masked():
        masked = K.window_difference(O.forward(cl, sdl, *long)[0], O.forward(cs, sds, *short)[0], ns)
    print(f"{kind}: window 50 against 20, live rows: masked {masked:.2e}, unmasked {plain:.2e}")
    assert masked <= 1e-12
    assert plain >= 1.0                                                            # the test is sharp: the pads do count there


# ---------------------------------------------------------------------------------------------------------------------------
# 3. edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_leading_pads_leave_the_keys_and_an_interior_zero_stays():
    cfg, sd = _sas(heads=2)
    sd = {k: v.double() for k, v in sd.items()}
    seq = torch.randint(1, G.I + 1, (4, 20), generator=torch.Generator().manual_seed(5))
    seq[0, :3] = 0
    seq[0, 7] = 0               # an interior zero: a key as ever
    seq[1, :19] = 0             # a single item
    seq[2, :] = 0               # all pad
    keep = (seq != 0).unsqueeze(-1).double()
    assert K.leading_pads(keep).tolist() == [3, 19, 20, 0]
    taps = {}
    with K.masked():
        h = O.forward(cfg, sd, seq, None, taps=taps)[0]
    assert bool(torch.isfinite(h).all())
    for i in range(cfg.num_blocks):
        p = taps[f"p{i}"]                                       # (B, H, L, L)
        assert bool(torch.isfinite(p).all())
        assert bool((p[0, :, 3:, :3] == 0).all())               # exact zeros on the leading pads
        assert bool((p[0, :, 7:, 7] > 0).all())                 # the interior zero is a key of every later row
        assert torch.allclose(p[0, :, 3:].sum(-1), torch.ones(2, 17, dtype=torch.float64), atol=1e-14)
        assert bool((p[1, :, 19, 19] == 1).all()) and bool((p[1, :, 19, :19] == 0).all())
        assert bool((p[3] == taps_plain(cfg, sd, seq)[f"p{i}"][3]).all())           # no pads: the oracle's own probabilities
        assert bool((taps[f"y{i}"][2] == 0).all())              # the all-pad sequence: zeros behind every block
    assert torch.equal(h[2], h[2, :1].expand_as(h[2]))          # ... and the last LayerNorm's bias on every row


def taps_plain(cfg, sd, seq):
    taps = {}
    O.forward(cfg, sd, seq, None, taps=taps)
    return taps


def test_pad_keys_get_no_gradient_under_the_mask():
    """dk / dv of a leading pad are exact zeros: the key bias has the oracle's true gradient 0 either way, the VALUE bias
    loses the pads' terms - with one live row per sequence its gradient comes through that row's own value alone"""
    cfg, sd = _sas(blocks=1)
    g = torch.Generator().manual_seed(6)
    seq, pos, neg = (torch.randint(1, G.I + 1, (3, 20), generator=g) for _ in range(3))
    for x in (seq, pos, neg):
        x[:, :12] = 0
    batch = (seq, None, pos, None, neg, None)
    sd = {k: v.double() for k, v in sd.items()}
    with K.masked():
        masked = O.grads_of(cfg, sd, batch)[1]
    plain = O.grads_of(cfg, sd, batch)[1]
    D = cfg.D
    bm, bp = masked["attention_layers.0.in_proj_bias"], plain["attention_layers.0.in_proj_bias"]
    assert float((bm[2 * D:] - bp[2 * D:]).abs().max()) > 1e-6                    # the pads' dv terms are gone
    assert all(bool(torch.isfinite(v).all()) for v in masked.values())
    assert bool((masked[O.key_pos(cfg)][:12] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 4. every job stays admissible under the masked reference
# ---------------------------------------------------------------------------------------------------------------------------
def test_seed_table_names_jobs_and_adds_no_clamp():
    assert set(K.KEYMASK_SEEDS) <= set(GRAD_JOBS) | set(FWD_JOBS)
    assert all(K.grad_seed(cid, m) == G.SEEDS[cid, m] for cid, m in GRAD_JOBS if (cid, m) not in K.KEYMASK_SEEDS)
    assert all(K.fwd_seed(cid, m) == F.seed_of(cid, m) for cid, m in FWD_JOBS if (cid, m) not in K.KEYMASK_SEEDS)
    ref = K.grad_reference("s", "autograd")
    assert ref.clamp == (("s", "autograd") in G.OVER_CAP)
    assert K.fwd_reference("s", "train").clamp == (("s", "train") in F.FWD_OVER_CAP)
    assert O.encoder_block is K._ORACLE_BLOCK


@pytest.mark.parametrize("cid,mode", GRAD_JOBS, ids=[f"{cid}-{mode}" for cid, mode in GRAD_JOBS])
def test_gradient_job_is_admissible_under_the_mask(cid, mode):
    ref = K.grad_reference(cid, mode)
    assert ref.clamp == ((cid, mode) in G.OVER_CAP)
    G.assert_admissible(ref, f"case {cid} {mode} (key-padding mask)")
    assert O.encoder_block is K._ORACLE_BLOCK


@pytest.mark.parametrize("cid,mode", FWD_JOBS, ids=[f"{cid}-{mode}" for cid, mode in FWD_JOBS])
def test_forward_job_is_admissible_under_the_mask(cid, mode):
    ref = K.fwd_reference(cid, mode)
    assert ref.clamp == ((cid, mode) in F.FWD_OVER_CAP)
    F.assert_admissible(ref, f"case {cid} {mode} (key-padding mask)")
    if mode != "last":
        loss64, e32 = F.loss_reference(ref)
        assert F.FACTOR_FWD * e32 <= F.CAP_FWD and loss64 > 0.0
    assert O.encoder_block is K._ORACLE_BLOCK


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


def test_header_names_the_flag():
    text = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    assert re.search(r"#define\s+SRFRD_LAYOUT_MASK_PAD_KEYS\s+1\b", text)
    assert re.search(r"int32_t\s+flags;", text) and "reserved0" not in text
    assert _lib.LAYOUT_MASK_PAD_KEYS == 1
    names = [n for n, _ in _lib.Layout._fields_]
    assert names[names.index("table_bf16") + 1] == "flags" and names[names.index("flags") + 1] == "off_pos"
    assert _lib.Layout.flags.offset == 13 * 4 and _lib.Layout.off_pos.offset == 14 * 4      # the struct did not move


def test_layout_init_writes_no_flag(lib):
    lay = _lib.Layout()
    C.memset(C.byref(lay), 0xFF, C.sizeof(lay))
    assert lib.srfrd_layout_init(C.byref(lay), 0, 300, 50, 50, 0, 0, 2, 1) == 0
    assert lay.flags == 0 and lay.table_bf16 == 0
    assert _lib.make_layout("SRFRN", 300, 50, 45, 5, 0, 2, 1).flags == 0


SHAPES = [("SASRec", 50, 0, 1, 50, 6), ("SRFRN", 45, 5, 1, 50, 17), ("SASRec", 50, 0, 2, 50, 6), ("SASRec", 50, 0, 1, 20, 6),
          ("SASRec", 50, 0, 1, 100, 5), ("SRFRN", 45, 5, 1, 203, 5), ("SASRec", 40, 0, 1, 37, 6)]


def _plans(lay, B, L):
    out = []
    for mode in (0, _lib.PLAN_POS | _lib.PLAN_NEG, _lib.PLAN_POS | _lib.PLAN_NEG | _lib.PLAN_CKPT | _lib.PLAN_LOSS
                 | _lib.PLAN_DROPOUT | _lib.PLAN_FUSED_BCE):
        for sw in (0, _lib.SWITCHES["SRFRD_NO_RAGGED"], _lib.SWITCHES["SRFRD_ROWS_ALWAYS"]):
            scratch = max(_lib.scratch_floats(lay, B, L))
            out.append(_lib.encoder_plan(lay, B, L, mode, sw, N_CU, scratch))
            out.append(_lib.encoder_plan_train(lay, B, L, mode, sw, N_CU, scratch))
    return out


@pytest.mark.parametrize("kind,di,df,heads,L,B", SHAPES)
def test_the_flag_moves_no_plan_and_an_unknown_bit_is_refused(lib, kind, di, df, heads, L, B):
    lay = _lib.make_layout(kind, 300, L, di, df, 0, 2, heads)
    plain = _plans(lay, B, L)
    assert plain[0][0][0].startswith("srfrd") and plain[0][0][1] > 0      # ((forward, grid), (backward, grid)) | (train, grid)
    lay.flags = _lib.LAYOUT_MASK_PAD_KEYS
    assert _plans(lay, B, L) == plain                           # every name and every grid
    refused = ("", E.E_UNSUPPORTED)
    for flags in (2, 3, 1 << 30, -1):
        lay.flags = flags
        assert _lib.encoder_plan(lay, B, L, _lib.PLAN_POS | _lib.PLAN_NEG, 0, N_CU, 1 << 24) == (refused, refused), flags
        assert _lib.encoder_plan_train(lay, B, L, _lib.PLAN_POS | _lib.PLAN_NEG | _lib.PLAN_CKPT | _lib.PLAN_LOSS
                                       | _lib.PLAN_FUSED_BCE, 0, N_CU, 1 << 24) == refused, flags


def test_the_model_switch_sets_the_layouts_bit_and_nothing_else():
    import srfrd_amd
    m = srfrd_amd.SASRec(G.I, 20, 50, 0.0, 2, 1, "cpu")
    before = bytes(m.layout)
    keys = list(m.state_dict())
    assert m.key_padding_mask is False and m.layout.flags == 0
    assert m.use_key_padding_mask() is m and m.key_padding_mask is True and m.layout.flags == _lib.LAYOUT_MASK_PAD_KEYS
    after = bytearray(bytes(m.layout))
    after[_lib.Layout.flags.offset] = 0
    assert bytes(after) == before                               # the one bit
    assert m.use_key_padding_mask(on=False) is m and m.key_padding_mask is False and bytes(m.layout) == before
    assert list(m.state_dict()) == keys


@pytest.mark.parametrize("entry", E.ENTRIES)
def test_every_encoder_entry_point_refuses_an_unknown_bit(lib, entry):
    """dummy pointers, as tests/test_encoder_entry_refusals.py: the call returns before any launch"""
    lay = _lib.make_layout("SASRec", 300, 200, 50, 0, 0, 2, 1)
    lay.flags = _lib.LAYOUT_MASK_PAD_KEYS | 4
    assert E._call(lib, {"sas": lay}, entry, scratch=E._d(), scratch_floats=1 << 24) == E.E_UNSUPPORTED
    lay.flags = 2
    assert E._call(lib, {"sas": lay}, entry, scratch=E._d(), scratch_floats=1 << 24) == E.E_UNSUPPORTED
    # an argument defect is still judged first, a known bit changes no refusal
    lay.flags = _lib.LAYOUT_MASK_PAD_KEYS
    assert E._call(lib, {"sas": lay}, entry, B=0) == E.E_ARG
    assert E._call(lib, {"sas": lay}, entry, L=201) == E.E_ARG
