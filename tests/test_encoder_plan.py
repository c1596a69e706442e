"""CPU: the encoder's kernel plan (srfrd_encoder_plan) pinned against the dispatch rules it replaced.

Every parity test passes whichever kernel family runs, because every fallback is correct: only this table notices a shape
that slips from one family to another.  `expected` is the launchers' selection as it stood before the plan existed (forward:
row-owner, global-scratch build, ragged, first-generation specialisations; backward: ragged, slot-placed, row-chunked,
global-scratch build, first-generation), written out independently of the C++; `PINNED` holds literal rows confirmed by
kernel traces of the benchmark workloads and of one call per switch on an MI355X.
"""
import itertools
import json
import os

import pytest

from srfrd_amd import _lib
from tests.helpers import GOLDEN

N_CU = 256
# (kind, d_item, d_fake, n_labels, heads): every kind and item width the project uses, one width without a specialisation
LAYOUTS = [("SASRec", 50, 0, 0, 1), ("SRFR", 45, 5, 0, 1), ("SRFRN", 45, 5, 0, 1), ("SRFU_B", 50, 0, 3, 1),
           ("SRFU_F", 50, 0, 3, 1), ("SRFU_R", 50, 0, 3, 1), ("SASRec", 40, 0, 0, 1), ("SASRec", 50, 0, 0, 2),
           ("SRFRN", 45, 5, 0, 5)]
LENGTHS = [20, 32, 50, 64, 100, 112, 113, 128, 200, 208]
P = _lib
TRAIN = P.PLAN_POS | P.PLAN_NEG | P.PLAN_CKPT | P.PLAN_LOSS | P.PLAN_FUSED_BCE
MODES = {
    "eval": P.PLAN_POS | P.PLAN_NEG,                # model.eval() forward with target logits
    "eval_last": 0,                                 # srfrd_encoder_fwd_last: hidden states only
    "fused_p": TRAIN | P.PLAN_DROPOUT,              # FusedTrainer step, dropout > 0
    "fused_p0": TRAIN,                              # FusedTrainer step, dropout 0
    "autograd": P.PLAN_POS | P.PLAN_NEG | P.PLAN_CKPT | P.PLAN_DROPOUT,   # module forward + upstream-gradient backward
    "taps": TRAIN | P.PLAN_DROPOUT | P.PLAN_TAPS,
}
SWITCH_SETS = [None] + list(P.SWITCHES)


SIZE_DEPTHS = (1, 2, 3, 8)   # tests/golden/encoder_plan_sizes.json
DEPTHS = (1, 2, 3, 4, 8)    # 2: every existing row; 4: the first depth without the row-chunked backward at seq_len 200


def _layout(kind, di, df, nl, heads, nb=2):
    return _lib.make_layout(kind, 300, 208, di, df, nl, nb, heads)


def _variant(kind, di, D, heads):
    if D != 50 or heads != 1:
        return None
    return {"SASRec": (0, 50), "SRFR": (1, 45) if di == 45 else None, "SRFRN": (2, 45) if di == 45 else None}.get(
        kind, (-1, 50) if di == 50 else None)


def _lds_floats(L, D, nb, bwd):
    LP, DK = (L + 15) & ~15, (D + 3) & ~3
    DS, SLD, ln = DK + 2, LP + 2, (4 * nb + 2) * 64
    if bwd:
        return 8 * LP * DS + 2 * max(LP * SLD, LP * DS) + 2 * 64 + 10 * LP + 64 + 2 * ln
    return max(LP * DS, LP * SLD) + 4 * LP * DS + 64 + 4 * LP + 64 + ln


def expected(kind, di, df, heads, B, L, mode, sw, scratch, nb):
    """(forward name, grid), (backward name, grid) as the launchers chose them before the plan (hidden 50 = d_item + d_fake);
    nb: the depth, which enters through the LayerNorm caches of every LDS size below and through nothing else"""
    D, LIM = di + df, 160 * 1024
    kv = _variant(kind, di, D, heads)
    on = lambda s: sw == s
    taps = bool(mode & P.PLAN_TAPS)
    spec = not on("SRFRD_GENERIC") and D == 50 and heads == 1
    ragged = (L == 50 and kv is not None and not taps and
              not any(on(s) for s in ("SRFRD_NO_RAGGED", "SRFRD_GENERIC", "SRFRD_NO_SLOTS50", "SRFRD_ROWS_ALWAYS")))
    ftrain = all(mode & b for b in (P.PLAN_POS, P.PLAN_NEG, P.PLAN_CKPT, P.PLAN_LOSS, P.PLAN_DROPOUT)) and not taps
    btrain = all(mode & b for b in (P.PLAN_POS, P.PLAN_NEG, P.PLAN_FUSED_BCE, P.PLAN_DROPOUT)) and not taps
    plain = not mode & (P.PLAN_POS | P.PLAN_NEG | P.PLAN_CKPT | P.PLAN_LOSS | P.PLAN_DROPOUT)
    K, DI = kv if kv else (-1, 0)
    first = lambda d, t: f"srfrd::encoder_{d}_kernel<{','.join(map(str, t))}>"
    gen = (0, 0, 0, 0, -1, 0, 0)
    LP = (L + 15) & ~15
    tf = lambda b: "true" if b else "false"

    # forward
    fl = _lds_floats(L, D, nb, False)
    g1 = min(N_CU, B)
    rows_lds = 2 * LP * 54 + 8 * 2 * 16 * 54 + 5 * LP + 64 + (4 * nb + 2) * 64 + 64
    if ((fl * 4 > LIM or on("SRFRD_ROWS_ALWAYS")) and not taps and kv and not on("SRFRD_NO_ROWS") and not on("SRFRD_GENERIC")
            and L <= 208 and rows_lds * 4 <= LIM):
        fwd = (f"srfrd::encoder_fwd_rows_kernel<50,{K},{DI},{0 if plain else 1}>", g1)
    elif fl * 4 > LIM:
        stride = (fl + 128 + 63) & ~63
        fwd = ("", -2) if scratch < stride * g1 else ("srfrd_long::encoder_fwd_kernel<0,0,0,0,-1,0,0>", g1)
    else:
        g = min(N_CU * max(1, min(2, LIM // (fl * 4))), B)
        if ragged:
            fwd = (f"srfrd::encoder_fwd_ragged_kernel<{K},{int(ftrain)},{DI}>", g)
        elif spec and L == 50:
            fwd = (first("fwd", (50, 64, 8, 50, K, int(ftrain), DI) if kv else (50, 64, 8, 50, -1, 0, 0)), g)
        elif spec and L == 100 and kind == "SASRec":
            fwd = (first("fwd", (50, 112, 16 if ftrain else 8, 100, 0, int(ftrain), 50)), g)
        elif spec and LP in (32, 64):
            fwd = (first("fwd", (50, LP, 8, 0, -1, 0, 0)), g)
        else:
            fwd = (first("fwd", gen), g)

    # backward
    bl = _lds_floats(L, D, nb, True)
    gb = min(B, N_CU * (2 if L == 50 and kv else 1))
    rmw = B > gb
    stride = (bl + 128 + 63) & ~63
    LR = (L + 3) & ~3
    slots_lds = 6 * LR * 54 + 11 * LP + 64 + 2 * (4 * nb + 2) * 64 + 64
    pool = max(48 * (LR + 2) + 2 * 48 * 54, 5 * 48 * 54)
    chunks_lds = 2 * LR * 54 + pool + 11 * LP + 64 + 2 * (4 * nb + 2) * 64 + 64
    long_ok = bl * 4 > LIM and not taps and kv and not on("SRFRD_NO_SLOTS") and not on("SRFRD_GENERIC")
    if ragged:
        bwd = f"srfrd::encoder_bwd_ragged_kernel<{K},{DI},{tf(rmw)}>"
    elif L == 50 and kv and not taps and not on("SRFRD_NO_SLOTS50") and not on("SRFRD_GENERIC"):
        bwd = f"srfrd::encoder_bwd_slots_kernel<50,50,{K},{DI},{tf(rmw)}>"
    elif long_ok and L in (50, 100) and slots_lds * 4 <= LIM:
        bwd = f"srfrd::encoder_bwd_slots_kernel<50,{L},{K},{DI},{tf(rmw)}>"
    elif (long_ok and scratch >= stride * gb and 17 <= L <= 208 and chunks_lds * 4 <= LIM and
          stride >= 3 * (LR * 50 + 64)):
        bwd = f"srfrd::encoder_bwd_chunks_kernel<50,{K},{DI},{tf(rmw)}>"
    elif bl * 4 > LIM:
        c4 = spec and kind == "SASRec" and L == 100 and btrain
        bwd = "" if scratch < stride * gb else \
            f"srfrd_long::encoder_bwd_kernel<{'50,112,8,100,0,1,50' if c4 else '0,0,0,0,-1,0,0'}>"
    elif spec and L == 50:
        bwd = first("bwd", (50, 64, 8, 50, K, int(btrain), DI) if kv else (50, 64, 8, 50, -1, 0, 0))
    elif spec and LP in (32, 64):
        bwd = first("bwd", (50, LP, 8, 0, -1, 0, 0))
    else:
        bwd = first("bwd", gen)
    return fwd, (bwd, gb if bwd else -2)


def _rows():
    for (kind, di, df, nl, heads), L, mname, sw, B in itertools.product(LAYOUTS, LENGTHS, MODES, SWITCH_SETS, (6, 600)):
        yield kind, di, df, nl, heads, L, mname, sw, B


def _mismatches(nb, nb_expected):
    """rows at which the plan of a depth-`nb` layout differs from expected(..., nb_expected)"""
    bad = []
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        lay = _layout(kind, di, df, nl, heads, nb)
        sw_bits = P.SWITCHES[sw] if sw else 0
        for scratch in (max(_lib.scratch_floats(lay, B, L)), 0):
            got = _lib.encoder_plan(lay, B, L, MODES[mname], sw_bits, N_CU, scratch)
            want = expected(kind, di, df, heads, B, L, MODES[mname], sw, scratch, nb_expected)
            if got != want:
                bad.append((kind, di, heads, L, mname, sw, B, scratch, got, want))
    return bad


@pytest.mark.parametrize("nb", DEPTHS)
def test_plan_matches_the_dispatch_rules(nb):
    bad = _mismatches(nb, nb)
    assert not bad, f"{len(bad)} rows differ, first: {bad[:3]}"


@pytest.mark.parametrize("nb,other", [(2, 8), (8, 7), (3, 4), (4, 3)])
def test_the_dispatch_rules_notice_a_wrong_depth(nb, other):
    """the table above is not blind to the depth: `expected` handed another one differs from the plan (8 against 7: the
    first-generation forward's grid and backward; 3 against 4: the row-chunked backward at seq_len 200)"""
    assert _mismatches(nb, other)


def test_forward_is_ragged_iff_backward_is():
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        lay = _layout(kind, di, df, nl, heads)
        (f, _), (b, _) = _lib.encoder_plan(lay, B, L, MODES[mname], P.SWITCHES[sw] if sw else 0, N_CU,
                                           max(_lib.scratch_floats(lay, B, L)))
        assert ("encoder_fwd_ragged" in f) == ("encoder_bwd_ragged" in b), (kind, di, heads, L, mname, sw, f, b)


@pytest.mark.parametrize("n_cu", [256, 80])
def test_backward_grid_follows_srfrd_bwd_grid(n_cu):
    """B capped at CUs x 2 for the seq_len-50 slot shapes (hidden 50, one head, a specialised kind), CUs x 1 otherwise"""
    for (kind, di, df, nl, heads), L in itertools.product(LAYOUTS, LENGTHS):
        lay = _layout(kind, di, df, nl, heads)
        slot50 = L == 50 and _variant(kind, di, di + df, heads) is not None
        for B in (1, 6, n_cu, n_cu + 1, 2 * n_cu, 2 * n_cu + 1, 4096):
            grid = _lib.encoder_plan(lay, B, L, MODES["fused_p"], 0, n_cu, 1 << 40)[1][1]
            assert grid == min(B, n_cu * (2 if slot50 else 1)), (kind, di, heads, L, B)
            if n_cu == 256:                      # the library's own count on a machine without a GPU
                assert _lib.lib().srfrd_bwd_grid(lay, B, L) == grid


def test_scratch_and_lds_sizes_are_unchanged():
    """srfrd_scratch_floats / srfrd_lds_bytes are ABI: the values pinned before the plan existed"""
    pinned = json.load(open(os.path.join(GOLDEN, "encoder_plan_sizes.json")))
    seen = set()
    for ((kind, di, df, nl, heads), L), nb in itertools.product(itertools.product(LAYOUTS, LENGTHS), SIZE_DEPTHS):
        lay = _layout(kind, di, df, nl, heads, nb)
        for B in (6, 600):
            got = list(_lib.scratch_floats(lay, B, L)) + list(_lib.lds_bytes(lay, L))
            key = f"{kind}/{di}/{heads}/{L}/{B}" + ("" if nb == 2 else f"/b{nb}")      # depth 2: the keys as they were
            seen.add(key)
            assert got == pinned[key], (kind, di, heads, L, B, nb)
    assert seen == set(pinned)


# (layout, L, mode, switch) -> (forward, backward): rows seen in kernel traces (B = 6 unless noted)
PINNED = [
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", None, "srfrd::encoder_fwd_ragged_kernel<0,1,50>", "srfrd::encoder_bwd_ragged_kernel<0,50,false>"),
    (("SRFRN", 45, 5, 0, 1), 50, "fused_p", None, "srfrd::encoder_fwd_ragged_kernel<2,1,45>", "srfrd::encoder_bwd_ragged_kernel<2,45,false>"),
    (("SASRec", 50, 0, 0, 1), 100, "fused_p", None, "srfrd::encoder_fwd_kernel<50,112,16,100,0,1,50>", "srfrd::encoder_bwd_slots_kernel<50,100,0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 200, "fused_p", None, "srfrd::encoder_fwd_rows_kernel<50,0,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "eval_last", None, "srfrd::encoder_fwd_ragged_kernel<0,0,50>", "srfrd::encoder_bwd_ragged_kernel<0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 20, "autograd", None, "srfrd::encoder_fwd_kernel<50,32,8,0,-1,0,0>", "srfrd::encoder_bwd_kernel<50,32,8,0,-1,0,0>"),
    (("SASRec", 50, 0, 0, 2), 50, "fused_p", None, "srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    (("SASRec", 40, 0, 0, 1), 50, "fused_p", None, "srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    (("SASRec", 50, 0, 0, 1), 200, "eval", None, "srfrd::encoder_fwd_rows_kernel<50,0,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,0,50,false>"),
    (("SRFU_B", 50, 0, 3, 1), 113, "fused_p", None, "srfrd::encoder_fwd_rows_kernel<50,-1,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,-1,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", "SRFRD_NO_RAGGED", "srfrd::encoder_fwd_kernel<50,64,8,50,0,1,50>", "srfrd::encoder_bwd_slots_kernel<50,50,0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", "SRFRD_NO_SLOTS50", "srfrd::encoder_fwd_kernel<50,64,8,50,0,1,50>", "srfrd::encoder_bwd_kernel<50,64,8,50,0,1,50>"),
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", "SRFRD_GENERIC", "srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
    (("SASRec", 50, 0, 0, 1), 100, "fused_p", "SRFRD_NO_SLOTS", "srfrd::encoder_fwd_kernel<50,112,16,100,0,1,50>", "srfrd_long::encoder_bwd_kernel<50,112,8,100,0,1,50>"),
    (("SASRec", 50, 0, 0, 1), 200, "fused_p", "SRFRD_NO_ROWS", "srfrd_long::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_chunks_kernel<50,0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", "SRFRD_ROWS_ALWAYS", "srfrd::encoder_fwd_rows_kernel<50,0,50,1>", "srfrd::encoder_bwd_slots_kernel<50,50,0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "fused_p", "SRFRD_RAGGED_FULL_ROWS", "srfrd::encoder_fwd_ragged_kernel<0,1,50>", "srfrd::encoder_bwd_ragged_kernel<0,50,false>"),
    (("SASRec", 50, 0, 0, 1), 50, "taps", None, "srfrd::encoder_fwd_kernel<50,64,8,50,0,0,50>", "srfrd::encoder_bwd_kernel<50,64,8,50,0,0,50>"),
]


@pytest.mark.parametrize("lay,L,mname,sw,fwd,bwd", PINNED)
def test_pinned_rows(lay, L, mname, sw, fwd, bwd):
    layout = _layout(*lay)
    (f, _), (b, _) = _lib.encoder_plan(layout, 6, L, MODES[mname], P.SWITCHES[sw] if sw else 0, N_CU,
                                       max(_lib.scratch_floats(layout, 6, L)))
    assert (f, b) == (fwd, bwd)


# The LayerNorm caches ((4 nb + 2) * 64 floats, twice in a backward) are the only depth-dependent term of every LDS size, and
# they move three boundaries of the plan.  Rows as the built library answers them:
# (layout, depth, L, B, mode, switch) -> ((forward, grid), (backward, grid)), srfrd_lds_bytes, srfrd_scratch_floats
_S = ("SASRec", 50, 0, 0, 1)
_S2 = ("SASRec", 50, 0, 0, 2)
_GENF, _GENB = "srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_bwd_kernel<0,0,0,0,-1,0,0>"
_F50 = "srfrd::encoder_fwd_kernel<50,64,8,50,0,{},50>"
DEPTH_PINNED = [
    # first-generation backward at LP = 64, D = 50: 40 768 floats at depth 7, 41 280 (> 40 960 = 160 KB) at depth 8
    (_S2, 7, 50, 6, "fused_p", None, ((_GENF, 6), (_GENB, 6)), (81408, 163072), (0, 0)),
    (_S2, 8, 50, 6, "fused_p", None, ((_GENF, 6), ("srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>", 6)), (82432, 0), (0, 248448)),
    (_S, 7, 50, 600, "fused_p", "SRFRD_NO_SLOTS50", ((_F50.format(1), 512), ("srfrd::encoder_bwd_kernel<50,64,8,50,0,1,50>", 512)),
     (81408, 163072), (0, 0)),
    # ... where the working set is over the limit the slot-placed backward is the long-sequence answer at seq_len 50 too, and
    # SRFRD_NO_SLOTS50 (a switch of the LDS-resident selection) no longer reaches the first-generation kernel
    (_S, 8, 50, 600, "fused_p", "SRFRD_NO_SLOTS50", ((_F50.format(1), 256), ("srfrd::encoder_bwd_slots_kernel<50,50,0,50,true>", 512)),
     (82432, 0), (0, 21200896)),
    # row-chunked backward at seq_len 200: 40 688 floats at depth 3, 41 200 at depth 4
    (_S, 3, 200, 6, "fused_p", None, (("srfrd::encoder_fwd_rows_kernel<50,0,50,1>", 6), ("srfrd::encoder_bwd_chunks_kernel<50,0,50,false>", 6)),
     (0, 0), (543744, 1088640)),
    (_S, 4, 200, 6, "fused_p", None, (("srfrd::encoder_fwd_rows_kernel<50,0,50,1>", 6), ("srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>", 6)),
     (0, 0), (545280, 1091712)),
    # first-generation forward at seq_len 50: two workgroups per CU up to depth 7 (81 408 B each), one at depth 8 (82 432 B)
    (_S, 7, 50, 600, "eval", "SRFRD_NO_RAGGED", ((_F50.format(0), 512), ("srfrd::encoder_bwd_slots_kernel<50,50,0,50,true>", 512)),
     (81408, 163072), (0, 0)),
    (_S, 8, 50, 600, "eval", "SRFRD_NO_RAGGED", ((_F50.format(0), 256), ("srfrd::encoder_bwd_slots_kernel<50,50,0,50,true>", 512)),
     (82432, 0), (0, 21200896)),
    # the ragged pair follows the same forward grid; its backward keeps 2 x CUs at every depth (one workgroup fits a CU from
    # depth 3 on; no workgroup of it waits on another)
    (_S, 7, 50, 600, "eval", None, (("srfrd::encoder_fwd_ragged_kernel<0,0,50>", 512), ("srfrd::encoder_bwd_ragged_kernel<0,50,true>", 512)),
     (81408, 163072), (0, 0)),
    (_S, 8, 50, 600, "eval", None, (("srfrd::encoder_fwd_ragged_kernel<0,0,50>", 256), ("srfrd::encoder_bwd_ragged_kernel<0,50,true>", 512)),
     (82432, 0), (0, 21200896)),
]


@pytest.mark.parametrize("lay,nb,L,B,mname,sw,plan,lds,scratch", DEPTH_PINNED)
def test_depth_moves_the_family_boundaries(lay, nb, L, B, mname, sw, plan, lds, scratch):
    layout = _layout(*lay, nb)
    assert _lib.lds_bytes(layout, L) == lds and _lib.scratch_floats(layout, B, L) == scratch
    assert _lib.encoder_plan(layout, B, L, MODES[mname], P.SWITCHES[sw] if sw else 0, N_CU, max(scratch)) == plan


def test_c2_geometry_and_unsupported_cases():
    lay = _layout("SASRec", 50, 0, 0, 1)
    (f, gf), (b, gb) = _lib.encoder_plan(lay, 512, 50, MODES["fused_p"], 0, N_CU, 0)
    assert (f, gf, b, gb) == ("srfrd::encoder_fwd_ragged_kernel<0,1,50>", 512, "srfrd::encoder_bwd_ragged_kernel<0,50,false>", 512)
    # a long sequence whose scratch is too small: the global-scratch builds refuse (SRFRD_E_UNSUPPORTED)
    h2 = _layout("SASRec", 50, 0, 0, 2)
    need = _lib.scratch_floats(h2, 6, 200)
    assert _lib.encoder_plan(h2, 6, 200, MODES["fused_p"], 0, N_CU, min(need) - 1) == (("", -2), ("", -2))
    wide = _lib.make_layout("SASRec", 300, 50, 72, 0, 0, 2, 1)              # hidden width > 64
    assert _lib.encoder_plan(wide, 6, 50, MODES["fused_p"]) == (("", -2), ("", -2))
    with pytest.raises(RuntimeError):
        _lib.encoder_plan(lay, 6, 50, 0, 0, 0, 0)                            # n_cu 0: SRFRD_E_ARG
