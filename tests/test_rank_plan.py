"""CPU: the ranking's kernel plan (srfrd_rank_plan) pinned against the dispatch rules it replaced.

Every ranking path is exact, so no parity test notices a shape that moves from one stream to another: only this table
does.  `expected` restates the launchers' choices as they stood before the plan existed (the bf16 matrix-core stream's
switch-on rule and geometry, the fp32 stream's split search, the tau block rule and every SRFRD_E_UNSUPPORTED), written
out independently of the C++.  `PINNED` holds literal launch sequences read from kernel traces of tools/rank_latency.py on
an MI355X (names, workgroups, workgroup sizes; the trace's LDS column shows static LDS only).
"""
import ctypes as C
import json
import os

import pytest

from srfrd_amd import _lib
from tests.helpers import GOLDEN

E_ARG, E_UNSUPPORTED = -1, -2
N_CU = 256
LIMIT = 160 * 1024
LDS16 = 2 * 512 * 72 * 2                       # two 512-row chunks of bf16 rows, 144 B apart
LDS16X = LDS16 + 2 * 2 * 16 * 64 * 4           # + the item masks of the masked forms
OPS = (_lib.RANK_TOPK, _lib.RANK_TARGET, _lib.RANK_TARGET_METRIC)


def _cdiv(a, b):
    return -(-a // b)


def _layout(n_items, d_item, bf16):
    lay = _lib.make_layout("SRFRN", n_items, 20, 45, 5) if d_item == 45 else _lib.make_layout("SASRec", n_items, 20, d_item)
    lay.table_bf16 = int(bf16)
    return lay


def expected(lay, op, B, k, lo, hi, excl, sw, n_cu=N_CU):
    """[(kernel, workgroups, threads, dynamic LDS)] or SRFRD_E_UNSUPPORTED, as the launchers chose before the plan"""
    di, bf16, topk = lay.d_item, bool(lay.table_bf16), op == _lib.RANK_TOPK
    if lay.D > 64:
        return E_UNSUPPORTED
    n_rows, tiles = hi - lo, _cdiv(B, 16)
    nc = _cdiv(n_rows, 256)
    DSi = ((di + 3) & ~3) + 2
    lds = (256 * DSi + 16 * DSi + 16 * 258 + 16 + 64) * 4
    lds_stream = (256 * DSi + 2 * 16 * DSi + 32 + 8 * 16 + 64) * 4
    lds_x = lds_stream + 16 * 8 * 4
    lds_score = (2 * 16 * DSi + 16 + 64) * 4
    if (lds > LIMIT or (excl and lds_x > LIMIT)) if topk else lds_x > LIMIT:
        return E_UNSUPPORTED
    on = not (sw & _lib.SW_TOPK_FP32) and ((di <= 64 and (di % 2 == 0 or di <= 51)) if bf16 else di <= 52)
    se, x = ("false" if bf16 else "true"), ("true" if excl else "false")
    if on:
        nu = 2 if tiles > 16 else 1
        groups = _cdiv(tiles, 16 * nu)
        crows = 512 if bf16 else 256
        if di % 2 or _cdiv(n_rows, crows) * groups < 2 * n_cu:
            crows = 256
        if excl:
            crows, nu, groups = 256, 1, _cdiv(tiles, 16)
        copy_w = (di // 2 if di % 2 == 0 else di) if bf16 else di
        if crows * copy_w > 13 * 1024:
            crows = 256
        if crows * copy_w > 13 * 1024:
            return E_UNSUPPORTED
        nch = _cdiv(n_rows, crows)
        if nch * groups < n_cu and nu == 2:
            nu, groups = 1, _cdiv(tiles, 16)
        per = min(max(n_cu // groups, 1), nch)
        grid, chunks = groups * per, nch
        pass_lds = LDS16X if excl else LDS16
    else:
        chunks, pass_lds = nc, (lds_x if excl else lds_stream)
        if topk:
            slots = 256 * (2 if lds_stream * 2 <= LIMIT else 1)
            best, splits = 1e30, 1
            for sp in range(1, min(tiles, 64) + 1):
                cost = _cdiv(nc * sp, slots) * (7.0 + _cdiv(tiles, sp))
                if cost < best:
                    best, splits = cost, sp
        else:
            splits = min(tiles, 8)
        grid = nc * splits
    out = [("srfrd::excl_prep_kernel", B, 1024, 0)] if excl else []
    per4 = _cdiv(B, 4)
    if topk:
        row = chunks * 4
        wpb = 4 if 4 * row <= 64 * 1024 else 1
        if wpb * row > LIMIT:
            return E_UNSUPPORTED
        tau = ("srfrd::topk_tau_kernel", _cdiv(B, wpb), 64 * wpb, wpb * row)
        if on:
            out += [(f"srfrd::topk_max16_kernel<{nu},{se},{x}>", grid, 1024, pass_lds), tau,
                    (f"srfrd::topk_collect16_kernel<{nu},{se}>", grid, 1024, LDS16)]
        else:
            out += [(f"srfrd::topk_max_kernel<{x}>", grid, 512, pass_lds), tau, ("srfrd::topk_collect_kernel", grid, 512, lds_stream)]
        if excl:
            out.append(("srfrd::topk_excl_filter_kernel", per4, 256, 0))
        out += [("srfrd::topk_select_kernel", per4, 256, 0), (f"srfrd::topk_stage1_kernel<{x}>", nc, 256, lds),
                ("srfrd::topk_stage2_kernel", per4, 256, 0)]
    else:
        if on:
            out += [(f"srfrd::target_score16_kernel<{se}>", tiles, 64, 0), (f"srfrd::target_count16_kernel<{nu},{se},{x}>", grid, 1024, pass_lds)]
        else:
            out += [("srfrd::target_score_kernel", tiles, 64, lds_score), (f"srfrd::target_count_kernel<{x}>", grid, 512, pass_lds)]
        if op == _lib.RANK_TARGET_METRIC:
            out.append(("srfrd::target_metric_kernel", _cdiv(B, 256), 256, 0))
    return out


# catalogs of 1000, 50 k and 1 M items over the whole range, and one shard of the 1 M catalog
RANGES = [(1000, 0, 1001), (50_000, 0, 50_001), (1_000_000, 0, 1_000_001), (1_000_000, 333_334, 666_667)]


@pytest.mark.parametrize("d_item", [45, 50, 51, 52, 53, 64, 65])
@pytest.mark.parametrize("bf16", [False, True])
def test_plan_matches_the_dispatch_rules(d_item, bf16):
    n = 0
    for n_items, lo, hi in RANGES:
        lay = _layout(n_items, d_item, bf16)
        for B in (1, 16, 100, 512, 4096):
            for op in OPS:
                for k in ((1, 10, 64) if op == _lib.RANK_TOPK else (1,)):
                    for excl in (False, True):
                        for sw in (0, _lib.SW_TOPK_FP32):
                            got = _lib.rank_plan(lay, op, B, k, lo, hi, excl, sw, N_CU)
                            assert got == expected(lay, op, B, k, lo, hi, excl, sw), (n_items, lo, hi, B, op, k, excl, sw)
                            n += 1
    assert n == 4 * 5 * 5 * 2 * 2


def test_the_encoder_switches_leave_ranking_alone_and_n_cu_counts():
    lay = _layout(50_000, 50, False)
    base = _lib.rank_plan(lay, _lib.RANK_TOPK, 512, 10, 0, 50_001)
    for bit in _lib.SWITCHES.values():
        assert _lib.rank_plan(lay, _lib.RANK_TOPK, 512, 10, 0, 50_001, switches=bit) == base
    for n_cu in (80, 304):
        assert _lib.rank_plan(lay, _lib.RANK_TOPK, 512, 10, 0, 50_001, n_cu=n_cu) == expected(lay, 0, 512, 10, 0, 50_001, False, 0, n_cu)


def _seq(*rows):
    return [r for r in rows if r]


def _topk_rows(max_, tau, collect, stage1, excl):
    sel = [("srfrd::topk_select_kernel", 128, 256), (stage1[0], stage1[1], 256), ("srfrd::topk_stage2_kernel", 128, 256)]
    return _seq(("srfrd::excl_prep_kernel", 512, 1024) if excl else None, max_, tau, collect,
                ("srfrd::topk_excl_filter_kernel", 128, 256) if excl else None) + sel


TAU = ("srfrd::topk_tau_kernel", 128, 256)
PREP = ("srfrd::excl_prep_kernel", 512, 1024)
# tools/rank_latency.py --child <config> (SASRec, d_item 50, B 512, k 10, the whole catalog): topk, topk excluding the input
# window, target_rank excluding it - (config, items, bf16 table, SRFRD_TOPK_FP32, topk, topk excl, target rank excl)
PINNED = [
    ("C2", 50_000, False, False,
     _topk_rows(("srfrd::topk_max16_kernel<1,true,false>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<1,true>", 256, 1024),
                ("srfrd::topk_stage1_kernel<false>", 196), False),
     _topk_rows(("srfrd::topk_max16_kernel<1,true,true>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<1,true>", 256, 1024),
                ("srfrd::topk_stage1_kernel<true>", 196), True),
     [PREP, ("srfrd::target_score16_kernel<true>", 32, 64), ("srfrd::target_count16_kernel<1,true,true>", 256, 1024)]),
    ("C5", 1_000_000, False, False,
     _topk_rows(("srfrd::topk_max16_kernel<2,true,false>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<2,true>", 256, 1024),
                ("srfrd::topk_stage1_kernel<false>", 3907), False),
     _topk_rows(("srfrd::topk_max16_kernel<1,true,true>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<1,true>", 256, 1024),
                ("srfrd::topk_stage1_kernel<true>", 3907), True),
     [PREP, ("srfrd::target_score16_kernel<true>", 32, 64), ("srfrd::target_count16_kernel<1,true,true>", 256, 1024)]),
    ("C5_bf16", 1_000_000, True, False,
     _topk_rows(("srfrd::topk_max16_kernel<2,false,false>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<2,false>", 256, 1024),
                ("srfrd::topk_stage1_kernel<false>", 3907), False),
     _topk_rows(("srfrd::topk_max16_kernel<1,false,true>", 256, 1024), TAU, ("srfrd::topk_collect16_kernel<1,false>", 256, 1024),
                ("srfrd::topk_stage1_kernel<true>", 3907), True),
     [PREP, ("srfrd::target_score16_kernel<false>", 32, 64), ("srfrd::target_count16_kernel<1,false,true>", 256, 1024)]),
    ("C5_bf16", 1_000_000, True, True,
     _topk_rows(("srfrd::topk_max_kernel<false>", 3907, 512), TAU, ("srfrd::topk_collect_kernel", 3907, 512),
                ("srfrd::topk_stage1_kernel<false>", 3907), False),
     _topk_rows(("srfrd::topk_max_kernel<true>", 3907, 512), TAU, ("srfrd::topk_collect_kernel", 3907, 512),
                ("srfrd::topk_stage1_kernel<true>", 3907), True),
     [PREP, ("srfrd::target_score_kernel", 32, 64), ("srfrd::target_count_kernel<true>", 31256, 512)]),
    ("C2", 50_000, False, True,
     _topk_rows(("srfrd::topk_max_kernel<false>", 392, 512), TAU, ("srfrd::topk_collect_kernel", 392, 512),
                ("srfrd::topk_stage1_kernel<false>", 196), False),
     _topk_rows(("srfrd::topk_max_kernel<true>", 392, 512), TAU, ("srfrd::topk_collect_kernel", 392, 512),
                ("srfrd::topk_stage1_kernel<true>", 196), True),
     [PREP, ("srfrd::target_score_kernel", 32, 64), ("srfrd::target_count_kernel<true>", 1568, 512)]),
]


@pytest.mark.parametrize("cfg,n_items,bf16,fp32sw,topk,topk_excl,rank_excl", PINNED)
def test_pinned_rows(cfg, n_items, bf16, fp32sw, topk, topk_excl, rank_excl):
    lay = _layout(n_items, 50, bf16)
    sw = _lib.SW_TOPK_FP32 if fp32sw else 0
    trim = lambda plan: [r[:3] for r in plan]
    assert trim(_lib.rank_plan(lay, _lib.RANK_TOPK, 512, 10, 0, n_items + 1, False, sw)) == topk
    assert trim(_lib.rank_plan(lay, _lib.RANK_TOPK, 512, 10, 0, n_items + 1, True, sw)) == topk_excl
    assert trim(_lib.rank_plan(lay, _lib.RANK_TARGET, 512, 1, 0, n_items + 1, True, sw)) == rank_excl


def test_c2_dynamic_lds():
    plan = _lib.rank_plan(_layout(50_000, 50, False), _lib.RANK_TOPK, 512, 10, 0, 50_001)
    assert [r[3] for r in plan] == [147456, 3136, 147456, 0, 75584, 0]      # (tau: 4 users' rows of 196 chunk maxima)


def test_arguments_and_refusals():
    lay = _layout(1000, 50, False)
    assert _lib.rank_plan(lay, _lib.RANK_TOPK, 0, 10, 0, 1001) == E_ARG
    assert _lib.rank_plan(lay, _lib.RANK_TOPK, 4, 65, 0, 1001) == E_ARG
    assert _lib.rank_plan(lay, _lib.RANK_TOPK, 4, 10, 0, 1002) == E_ARG
    assert _lib.rank_plan(lay, _lib.RANK_TOPK, 4, 10, 5, 5) == E_ARG
    assert _lib.rank_plan(lay, 3, 4, 10, 0, 1001) == E_ARG
    assert _lib.rank_plan(lay, _lib.RANK_TOPK, 4, 10, 0, 1001, n_cu=0) == E_ARG
    assert _lib.rank_plan(_layout(1000, 65, False), _lib.RANK_TARGET, 4, 1, 0, 1001) == E_UNSUPPORTED
    # tau holds one user's row of chunk maxima in at most 160 KiB: 40960 chunks of the stream
    big = _layout(11_000_000, 50, False)
    assert _lib.rank_plan(big, _lib.RANK_TOPK, 4, 10, 0, 10_485_760) != E_UNSUPPORTED
    assert _lib.rank_plan(big, _lib.RANK_TOPK, 4, 10, 0, 10_485_761) == E_UNSUPPORTED
    assert _lib.rank_plan(big, _lib.RANK_TOPK, 4, 10, 0, 11_000_001, switches=_lib.SW_TOPK_FP32) == E_UNSUPPORTED
    assert _lib.rank_plan(big, _lib.RANK_TARGET, 4, 1, 0, 11_000_001) != E_UNSUPPORTED          # (no tau pass)


def test_refused_call_launches_nothing():
    """An 11 M-row fp32 catalog is refused by the plan, before the first launch: the dummy pointers are never used."""
    lay = _layout(11_000_000, 50, False)
    d = C.c_void_p(64)
    assert _lib.lib().srfrd_logits_topk(C.byref(lay), d, d, d, 4, 1, 0, 11_000_001, 1, None, 10, d, d, d, None) == E_UNSUPPORTED
    assert _lib.lib().srfrd_logits_topk_excl(C.byref(lay), d, d, d, 4, 1, 0, 11_000_001, 1, None, 10, d, d, 8, d, d, d, d,
                                             None) == E_UNSUPPORTED


def test_workspace_bytes_are_unchanged():
    pinned = json.load(open(os.path.join(GOLDEN, "rank_workspace_bytes.json")))
    L = _lib.lib()
    for B, k, n, want in pinned["topk_workspace_bytes"]:
        assert L.srfrd_topk_workspace_bytes(B, k, n) == want, (B, k, n)
    for B, m, n, want in pinned["excl_workspace_bytes"]:
        assert L.srfrd_excl_workspace_bytes(B, m, n) == want, (B, m, n)
