"""-m gpu: batch tails and plan corners of the full-catalog ranking, against the fp64 host reference of tests/rank_refs.py, at
widths 32, 50, 64 (fp32 table) and 50, 51, 64 (bf16 shadow): B in {1, 15, 16, 17, 33} (users past B in the last tile), two user
tiles per wave (B = 257 and 300 over the smallest catalog for which srfrd_rank_plan, asked with the device's CU count, names a
<2,...> kernel), 512-row chunks with exact ties across their seam, a one-chunk catalog (n_items = 17) with k = 64, the
exhaustive path on distinct scores (k = 50 over fewer than 50 chunks and more than 2048 rows), k = 50 on the threshold path,
one user per block in topk_tau_kernel (4097 chunks), and ShardedRanker with 3 and 8 shards at k = 64.  The inputs come from
tests/rank_refs.py; tests/test_rank_width_cover.py shows from the reference alone that each stays under the near-tie cap."""
import numpy as np
import pytest
import torch

from tests import rank_refs as R

pytestmark = pytest.mark.gpu
Tally = R.Tally


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _start(case, d, route, monkeypatch, what):
    R.set_route(monkeypatch, route)
    run = R.Runner(case, route)
    return run, run.ref(), Tally(f"{what} d_item {d} {route} B {case.B} rows {case.n_items + 1}")


@pytest.mark.parametrize("B", R.SHAPE_BATCHES)
@pytest.mark.parametrize("d, route", R.SHAPE_WIDTHS)
def test_batch_tails(d, route, B, monkeypatch):
    run, ref, T = _start(R.tail_case(d, B), d, route, monkeypatch, "tail")
    full = (0, R.N_ITEMS + 1)
    rows = R.exclusion_rows(ref, *full, R.N_ITEMS, B)
    for k in (10, 64):
        T.topk(run, ref, k, *full, what="plain")
        T.topk(run, ref, k, *full, excl_rows=rows, what="excl")
    t = R.rank_targets(ref, B)
    T.rank(run, ref, t, *full, what="rank")
    T.rank(run, ref, t, *full, excl_rows=rows, what="rank excl")
    T.close()


@pytest.mark.parametrize("B", R.NU2_BATCHES)
@pytest.mark.parametrize("d, route", [(d, r) for d, r in R.SHAPE_WIDTHS if R.is_stream16(d, r)])
def test_two_user_tiles_per_wave(d, route, B, monkeypatch):
    from srfrd_amd import _lib
    n_cu = _n_cu()
    n_items = R.first_n_items(d, route, _lib.RANK_TOPK, B, 10, n_cu, R.is_nu2)
    for op, k in ((_lib.RANK_TOPK, 10), (_lib.RANK_TARGET, 1)):
        p = R.plan(d, 0, n_items, route, op, B, k, 0, n_items + 1, False, n_cu)
        assert R.is_nu2(p), p
    assert not R.is_nu2(R.plan(d, 0, n_items - 256, route, _lib.RANK_TOPK, B, 10, 0, n_items - 255, False, n_cu))
    run, ref, T = _start(R.nu2_case(d, n_items, B), d, route, monkeypatch, "nu2")
    T.topk(run, ref, 10, 0, n_items + 1, what="nu2")
    T.rank(run, ref, R.rank_targets(ref, B), 0, n_items + 1, what="nu2 rank")
    T.close()


def test_512_row_chunks_and_their_seam(monkeypatch):
    from srfrd_amd import _lib
    B = R.B_WIDTHS
    n_items = R.first_n_items(50, "bf16", _lib.RANK_TOPK, B, 10, _n_cu(), R.is_chunk512)
    run, ref, T = _start(R.chunk512_case(n_items), 50, "bf16", monkeypatch, "chunk512")
    idx, val = T.topk(run, ref, 10, 0, n_items + 1, what="512")
    assert (idx[:, :6] == np.array(R.TIE_IDS_A + R.TIE_IDS_B)).all(), idx[:, :6]
    assert (val[:, 3:6].view(np.int32) == val[:, 3:4].view(np.int32)).all()
    assert (T.rank(run, ref, np.full(B, 512), 0, n_items + 1, dups=(511, 513), what="512 rank") == 3).all()
    T.close()


@pytest.mark.parametrize("d, route", R.SHAPE_WIDTHS)
def test_one_chunk_catalog(d, route, monkeypatch):
    run, ref, T = _start(R.one_chunk_case(d), d, route, monkeypatch, "one chunk")
    hi = R.ONE_CHUNK_ITEMS + 1
    for k in (1, 10, 64):
        T.topk(run, ref, k, 0, hi, what="one chunk")
        T.topk(run, ref, k, 0, hi, exclude_pad=False, what="one chunk with item 0")
    T.rank(run, ref, np.arange(R.B_WIDTHS) % hi, 0, hi, what="one chunk rank")
    T.close()


@pytest.mark.parametrize("rows", R.EXHAUSTIVE_ROWS + (R.K50_THRESHOLD_ROWS,))
@pytest.mark.parametrize("d, route", R.SHAPE_WIDTHS)
def test_k50(d, route, rows, monkeypatch):
    """k = 50 on distinct scores.  With fewer than 50 chunks tau is -inf, every row is a candidate and more than kCandMax of
    them overflow the list: the exhaustive path by rule.  (The plan lists topk_stage1 / stage2 for every top-k call - they
    return at once unless the overflow flag is set - so only the rule, not a kernel name, says that they ran.)  16 384 rows
    are 64 chunks: the same k on the threshold path."""
    p = R.plan(d, 0, rows - 1, route, 0, R.B_WIDTHS, 50, 0, rows, False, _n_cu())
    chunks = -(-rows // R.plan_chunk_rows(p, rows))
    assert (chunks < 50 and rows > R.K_CAND_MAX) if rows in R.EXHAUSTIVE_ROWS else chunks >= 50
    run, ref, T = _start(R.k50_case(d, rows), d, route, monkeypatch, "k50")
    T.topk(run, ref, 50, 0, rows, what="k50")
    T.topk(run, ref, 50, 0, rows, excl_rows=R.exclusion_rows(ref, 0, rows, rows - 1, d), what="k50 excl")
    T.close()


def test_tau_one_user_per_block(monkeypatch):
    """more than 4096 chunk maxima per user no longer fit four users' rows in 64 KiB: topk_tau_kernel runs one user per block"""
    d, B, n_items = R.WPB1
    p = R.plan(d, 0, n_items, "fp32", 0, B, 10, 0, n_items + 1, False, _n_cu())
    assert R.plan_wpb(p) == 1
    run, ref, T = _start(R.base_case(d, 0, 0, n_items=n_items, B=B), d, "fp32", monkeypatch, "wpb1")
    T.topk(run, ref, 10, 0, n_items + 1, what="wpb1")
    T.close()


@pytest.mark.parametrize("n_shards", R.SHARD_COUNTS)
@pytest.mark.parametrize("d, route", R.SHARD_CASES)
def test_sharded_ranking(d, route, n_shards, monkeypatch):
    """ShardedRanker.topk_hidden on the test's hidden states at k = 10 and k = 64, with a bit-identical pair of rows across
    every shard boundary.  The sharded and the unsharded list are each held to the fp64 reference (values, order, exact ties)
    and to each other: the same id in a slot with values within twice the bound, or two ids whose fp64 scores are that close.
    Where both lists come from one arithmetic they must agree bit for bit: always at k = 10 (threshold scheme on both sides),
    and at k = 64 on the fp32 stream (d_item 64).

    Finding (include/srfrd_hip.h now says so): at k = 64 the 2601 rows overflow kCandMax and the unsharded call is re-ranked by
    the exhaustive path on the fp32 matrix cores, while a shard of at most 867 rows stays on the bf16 stream; at d_item 50
    the same (user, item) score then differs in its last bit (2623.3130 against 2623.3132 on an MI355X), so bit equality
    holds for the ids of these inputs but not for the values."""
    import srfrd_amd
    run, ref, T = _start(R.sharded_case(d, n_shards), d, route, monkeypatch, f"sharded {n_shards}")
    full = (0, R.N_ITEMS + 1)
    r = srfrd_amd.ShardedRanker(run.m, n_shards=n_shards)
    want = np.array([i for c in R.shard_cuts(n_shards) for i in (c - 1, c)])
    for k in (10, 64):
        idx, val = T.topk(run, ref, k, *full, what="unsharded")
        n = min(k, want.size)
        assert (idx[:, :n] == want[:n]).all(), (idx[0, :n], want)
        si, sv = (t.cpu().numpy() for t in r.topk_hidden(run.hidden[:, -1, :].contiguous(), run.ulab, None, k=k))
        T.add(si, sv, ref, k, *full, what=("sharded", k))
        swaps, bits = R.check_same_lists(si, sv, idx, val, ref, tag=(T.tag, k))
        print(f"SHARD_VALUES {T.tag} k {k}: {swaps} slots with another id, {bits} of {sv.size} values differ in bits")
        if k == 10 or not R.is_stream16(d, route):
            assert swaps == 0 and bits == 0, (T.tag, k, swaps, bits)
    T.close()
