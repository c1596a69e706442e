"""-m gpu: full-catalog ranking at every item width.  srfrd_logits_topk, srfrd_logits_topk_excl, srfrd_target_rank and
srfrd_predict_logits run on hidden states the test supplies (no encoder), at every d_item in 1..64 on the three table routes
(fp32 table; fp32 table under SRFRD_TOPK_FP32=1; bf16 shadow) and on the SRFRN cases with their side term, over one catalog of
2601 rows (eleven 256-row chunks, the last of 41 rows) and 17 users (one past a user tile).

Every result is held to the fp64 host reference of tests/rank_refs.py, never to another kernel: values within
4 max(E32, 2^-23) A of s64 at the returned id, the reference's order at every adjacent pair whose fp64 gap exceeds twice that
bound and the same id set inside runs of closer pairs (at most 10 % of a case's (user, slot) pairs; tests/test_rank_width_cover.py
proves the cap from the reference alone), exact ties by ascending id, -1 / -inf behind the last rankable item, equal bits on a
second call.  k = 64 exceeds the eleven chunks, so tau is -inf and the 2601 candidates overflow kCandMax: the exhaustive
path runs on distinct scores.  Each case prints the largest |val - s64| / (max(E32, 2^-23) A) it saw (allowed: 4);
profiles/rank_width_margins.txt records the largest per route."""
import numpy as np
import pytest
import torch

from tests import rank_refs as R

pytestmark = pytest.mark.gpu

CASES = [(d, f, route) for d, f in R.WIDTH_CASES for route in R.ROUTES]
FULL = (0, R.N_ITEMS + 1)


Tally = R.Tally


def _start(d, f, route, case, monkeypatch, what):
    R.set_route(monkeypatch, route)
    run = R.Runner(case, route)
    return run, run.ref(), Tally(f"{what} d_item {d} d_fake {f} {route}")


@pytest.mark.parametrize("d, f, route", CASES)
def test_topk_values_order_ranges(d, f, route, monkeypatch):
    """k in {1, 10, 64} over the catalog with and without item 0; every row start alignment, one-row and sub-k ranges"""
    run, ref, T = _start(d, f, route, R.base_case(d, f), monkeypatch, "topk")
    for k in R.KS:
        for pad in (True, False):
            a = T.topk(run, ref, k, *FULL, exclude_pad=pad, what=("pad", pad))
            b = run.topk(k, *FULL, pad)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)), (T.tag, k, "second call")
    for lo, hi in R.ranges():
        for k in (10, 64):
            T.topk(run, ref, k, lo, hi, exclude_pad=True, what="range")
            if lo == 0:                                   # (0, 1) then holds item 0 alone
                T.topk(run, ref, k, lo, hi, exclude_pad=False, what="range with item 0")
    T.close()


@pytest.mark.parametrize("d, f, route", CASES)
def test_nothing_but_real_items_ranks(d, f, route, monkeypatch):
    """every true score <= -1: a zero-padded row, a stale row behind the tail, item 0 or a padding column would lead the list"""
    run, ref, T = _start(d, f, route, R.leak_case(d, f), monkeypatch, "leak")
    for lo, hi in R.LEAK_RANGES:
        idx, val = T.topk(run, ref, 64, lo, hi, what="leak range")
        assert (idx >= max(lo, 1)).all() and (idx < hi).all() and (val <= -1.0 + 1e-3).all(), T.tag
    idx, val = T.topk(run, ref, 64, *FULL, what="leak catalog")
    assert (idx >= 1).all() and (val <= -1.0 + 1e-3).all(), T.tag
    t = np.full(run.case.B, R.LEAK_RANGES[1][0] + 255)
    T.rank(run, ref, t, *R.LEAK_RANGES[1], what="leak rank")
    T.close()


@pytest.mark.parametrize("d, f, route", CASES)
def test_exclusion_and_target_rank(d, f, route, monkeypatch):
    run, ref, T = _start(d, f, route, R.base_case(d, f), monkeypatch, "excl")
    rows = R.exclusion_rows(ref, *FULL, R.N_ITEMS, d)
    top3, _ = R.topk_ref(ref.s, 3, *FULL, True)
    for k in R.KS:
        idx, _ = T.topk(run, ref, k, *FULL, excl_rows=rows, what="excl")
        for b in range(run.case.B - 1):
            assert not set(idx[b].tolist()) & set(top3[b].tolist()), (T.tag, b)
    sub = (257, 257 + 300)
    T.topk(run, ref, 64, *sub, excl_rows=R.exclusion_rows(ref, *sub, R.N_ITEMS, d + 1), what="excl range")
    t = R.rank_targets(ref, d)
    plain = T.rank(run, ref, t, *FULL, what="rank")
    T.rank(run, ref, t, *FULL, excl_rows=rows, what="rank excl")
    T.rank(run, ref, t, *FULL, exclude_pad=False, what="rank with item 0")
    lo_part = T.rank(run, ref, t, 0, 1000, what="rank part") + T.rank(run, ref, t, 1000, FULL[1], what="rank part")
    assert np.array_equal(lo_part, plain), T.tag                       # ranks over disjoint ranges add up
    assert np.array_equal(run.rank(t, *FULL), plain), T.tag
    T.close()


@pytest.mark.parametrize("d, f, route", CASES)
def test_exact_ties_go_to_the_lower_id(d, f, route, monkeypatch):
    """bit-identical rows across the 256- and 512-row seams, at slot k / k + 1, and as copies of the target"""
    run, ref, T = _start(d, f, route, R.tie_case(d, f), monkeypatch, "ties")
    R.check_tie_case(run.case, run.table_seen())
    for k in (1, 2, 4, 10, 64):
        idx, val = T.topk(run, ref, k, *FULL, what="ties")
        n = min(k, 10)
        assert (idx[:, :n] == np.array(R.TIE_ORDER[:n])).all(), (T.tag, k, idx[:, :n])
        bits = val.view(np.int32)
        for ids in (R.TIE_IDS_A, R.TIE_IDS_B):
            at = [R.TIE_ORDER.index(i) for i in ids if R.TIE_ORDER.index(i) < k]
            assert (bits[:, at] == bits[:, at[:1]]).all(), (T.tag, k, "identical rows, different scores")
    idx, _ = T.topk(run, ref, 10, 256, 2001, what="ties from a chunk seam")    # 256 leads its range; 2000 is the last row
    assert (idx[:, :9] == np.array([256, 257] + R.TIE_ORDER[3:10])).all() and (idx[:, 9] == 2000).all(), T.tag
    B = run.case.B
    for tgt, dups, want in ((512, (511, 513), 3), (511, (512, 513), 3), (2000, (700,), 9), (700, (2000,), 9), (256, (255, 257), 0)):
        got = T.rank(run, ref, np.full(B, tgt), *FULL, dups=dups, what=("dup target", tgt))
        assert (got == want).all(), (T.tag, tgt, got)
        got = T.rank(run, ref, np.full(B, tgt), *FULL, excl_rows=[np.array(dups)] * B, dups=dups, what=("dup target excl", tgt))
        assert (got == want).all(), (T.tag, tgt, got)
    T.close()


@pytest.mark.parametrize("d, f, route", CASES)
def test_magnitudes(d, f, route, monkeypatch):
    run = None
    for kind in R.MAGNITUDES:
        case = R.magnitude_case(d, f, kind)
        if run is None:
            run, _, _ = _start(d, f, route, case, monkeypatch, kind)
        ref, T = run.load(case).ref(), Tally(f"{kind} d_item {d} d_fake {f} {route}")
        for k in (10, 64):
            T.topk(run, ref, k, *FULL, what=kind)
        T.rank(run, ref, R.rank_targets(ref, d), *FULL, what=kind)
        if kind == "zero_row":
            got = run.predict(torch.tensor([R.ZERO_ROW]))
            side = ref.s[:, R.ZERO_ROW]
            assert (np.abs(got[:, 0] - side) <= ref.eps * ref.A[:, R.ZERO_ROW]).all(), T.tag
            T.rank(run, ref, np.full(case.B, R.ZERO_ROW), *FULL, what="zero row as target")
        if kind == "own_row":
            T.rank(run, ref, R.OWN_ROW0 + np.arange(case.B), *FULL, what="own row as target")
        T.close()


@pytest.mark.parametrize("d, f, route", CASES)
def test_predict(d, f, route, monkeypatch):
    """predict_logits against s64: a shared and a per-user candidate list, n_cand 1 and 101, duplicates, id 0 and ids outside
    the catalog (they read the clamped row)"""
    run, ref, T = _start(d, f, route, R.base_case(d, f), monkeypatch, "predict")
    g = torch.Generator().manual_seed(d)
    n, B = R.N_ITEMS, run.case.B
    worst = 0.0
    for n_cand in (1, 101):
        shared = torch.randint(1, n + 1, (n_cand,), generator=g)
        per = torch.randint(1, n + 1, (B, n_cand), generator=g)
        if n_cand > 1:
            shared[:6] = torch.tensor([0, n, n + 5, -3, 7, 7])
            per[:, :6] = torch.tensor([7, 7, 0, n + 1, 10 * n, n])
        else:
            per[:4, 0] = torch.tensor([0, n, n + 9, -1])
        for cand in (shared, per):
            got = run.predict(cand)
            worst = max(worst, R.check_predict(got, ref, cand, tag=T.tag))
            assert np.array_equal(got.view(np.int32), run.predict(cand).view(np.int32)), T.tag
    everything = torch.arange(n + 1)
    worst = max(worst, R.check_predict(run.predict(everything), ref, everything, tag=T.tag))
    print(f"RANK_MARGIN {T.tag} ratio {worst:.3f}")
