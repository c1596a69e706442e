"""Host-only guards of the ranking width and shape tests (tests/test_gpu_rank_widths.py, test_gpu_rank_shapes.py): the call
shapes they are parametrised over reach every kernel instantiation srfrd_rank_plan can name, both chunk sizes and both tau
block shapes; every generated input holds the situation it is named after; the share of near ties stays under the cap by the
fp64 reference alone; and the value bound of tests/rank_refs.py is sharp - ordinary fp32 evaluations of the test's own
inputs pass it, the defects a matrix-core ranking kernel can have do not.

Corners of the plan.  wpb = 1 of topk_tau_kernel needs more than 4096 stream chunks, a catalog above 1 048 576 rows: the
1 M-item tests (3907 chunks) stay on wpb = 4, so tests/test_gpu_rank_shapes.py runs one narrow catalog of 4097 chunks for it.
target_metric_kernel is launched only with a metric accumulator, which the torch op never passes: evaluation(full_catalog=True)
in tests/test_gpu_rank_exclude.py keeps it.  nu = 2 together with 512-row chunks needs 131 k rows at B > 512 and stays with the
1 M-item property tests; here nu = 2 runs on 256-row chunks and the 512-row chunks at nu = 1."""
import numpy as np
import pytest
import torch

from tests import rank_refs as R

N_CU = 256


def _names(calls):
    names, chunks, wpb = set(), set(), set()
    for d, f, n_items, route, op, B, k, lo, hi, excl in calls:
        p = R.plan(d, f, n_items, route, op, B, k, lo, hi, excl, N_CU)
        assert not isinstance(p, int), (d, f, n_items, route, op, B, k, lo, hi, excl, p)
        names |= {l[0] for l in p}
        if op == 0:
            chunks.add(R.plan_chunk_rows(p, hi - lo))
            wpb.add(R.plan_wpb(p))
    return names, chunks, wpb


def _every_name():
    s16 = ["<1,true,false>", "<1,true,true>", "<1,false,false>", "<1,false,true>", "<2,true,false>", "<2,false,false>"]
    out = {"srfrd::topk_max16_kernel" + t for t in s16} | {"srfrd::target_count16_kernel" + t for t in s16}
    out |= {"srfrd::topk_collect16_kernel" + t for t in ("<1,true>", "<1,false>", "<2,true>", "<2,false>")}
    for n in ("topk_max_kernel", "topk_stage1_kernel", "target_count_kernel"):
        out |= {f"srfrd::{n}<true>", f"srfrd::{n}<false>"}
    out |= {"srfrd::target_score16_kernel<true>", "srfrd::target_score16_kernel<false>"}
    out |= {"srfrd::" + n for n in ("excl_prep_kernel", "topk_tau_kernel", "topk_collect_kernel", "topk_excl_filter_kernel",
                                    "topk_select_kernel", "topk_stage2_kernel", "target_score_kernel")}
    return out


def test_width_lists():
    assert R.WIDTHS == list(range(1, 65)) and set(R.REQUIRED_WIDTHS) <= set(R.WIDTHS)
    assert {1, 32, 33, 51, 52, 53, 63, 64} <= set(R.REQUIRED_WIDTHS)
    assert len(R.WIDTH_CASES) == 64 + 13 and all(d + f <= 64 for d, f in R.WIDTH_CASES)
    # the route by width, as rank_plan takes it, has each of its seams inside the list
    for route in ("fp32", "bf16"):
        flips = [d for d in range(2, 65) if R.is_stream16(d, route) != R.is_stream16(d - 1, route)]
        # (the bf16 shadow alternates from 53 on - odd widths leave the stream: the first and the last change are required)
        assert flips and all(d in R.REQUIRED_WIDTHS and d - 1 in R.REQUIRED_WIDTHS for d in (flips[0], flips[-1]))
    for d in R.WIDTHS:
        for route in R.ROUTES:
            p = R.plan(d, 0, R.N_ITEMS, route, 0, R.B_WIDTHS, 10, 0, R.N_ITEMS + 1, False, N_CU)
            assert p[0][0].startswith("srfrd::topk_max16_kernel") == R.is_stream16(d, route), (d, route)


def test_calls_reach_every_instantiation_and_chunk_size():
    wn, wc, ww = _names(R.width_calls())
    sn, sc, sw = _names(R.shape_calls(N_CU))
    assert wn | sn == _every_name(), sorted(_every_name() - (wn | sn)) + sorted((wn | sn) - _every_name())
    # the width sweep alone reaches every nu = 1 form; nu = 2 and the 512-row chunks are the shape file's
    assert {n for n in _every_name() if "<2," not in n} <= wn
    assert wc == {256} and sc == {256, 512}
    assert ww | sw == {4}
    big = R.plan(8, 0, R.WPB1[2], "fp32", 0, 5, 10, 0, R.WPB1[2] + 1, False, N_CU)
    assert R.plan_wpb(big) == 1                       # test_tau_one_user_per_block of tests/test_gpu_rank_shapes.py


def test_exhaustive_sizes_overflow_by_rule():
    """fewer chunks than k -> tau = -inf -> every row a candidate; more rows than kCandMax -> the list overflows.  (The plan
    lists topk_stage1 / stage2 for every top-k call and they return at once unless the flag is set: the rule carries the
    claim, no kernel name does.)"""
    for d, route in R.SHAPE_WIDTHS:
        for rows in R.EXHAUSTIVE_ROWS + (R.N_ITEMS + 1,):
            k = 64 if rows == R.N_ITEMS + 1 else 50
            p = R.plan(d, 0, rows - 1, route, 0, R.B_WIDTHS, k, 0, rows, False, N_CU)
            chunks = -(-rows // R.plan_chunk_rows(p, rows))
            assert chunks < k and rows > R.K_CAND_MAX


@pytest.mark.parametrize("d_item, d_fake", R.WIDTH_CASES)
def test_cases_hold_their_situations(d_item, d_fake):
    full = (0, R.N_ITEMS + 1)
    for shadow in (False, True):
        seen = (lambda c: R.bf16_round(c.table)) if shadow else (lambda c: c.table)
        c = R.base_case(d_item, d_fake)
        ref = c.ref(seen(c))
        rows = R.exclusion_rows(ref, *full, c.n_items, d_item)
        for k in R.KS:
            assert R.skip_share(ref, k, *full, True) <= R.SKIP_CAP
            assert R.skip_share(ref, k, *full, True, rows) <= R.SKIP_CAP
        for lo, hi in R.ranges():
            for k in (10, 64):
                assert R.skip_share(ref, k, lo, hi, True) <= R.SKIP_CAP, (lo, hi)
                assert R.skip_share(ref, k, lo, hi, False) <= R.SKIP_CAP, (lo, hi)
        t = R.rank_targets(ref, d_item)
        near = R.check_rank(R.rank_ref(ref.s, t, *full, True, rows), ref, t, *full, True, rows)
        assert near <= R.SKIP_CAP * c.B
        lc = R.leak_case(d_item, d_fake)
        R.check_leak_case(lc)
        for lo, hi in R.LEAK_RANGES:
            assert R.skip_share(lc.ref(seen(lc)), 64, lo, hi, True) <= R.SKIP_CAP
        tc = R.tie_case(d_item, d_fake)
        R.check_tie_case(tc, seen(tc))
        tref = tc.ref(seen(tc))
        for k in (1, 2, 4, 10, 64):
            assert R.skip_share(tref, k, *full, True) <= R.SKIP_CAP
        assert R.skip_share(tref, 10, 256, 2001, True) <= R.SKIP_CAP
        for kind in R.MAGNITUDES:
            mc = R.magnitude_case(d_item, d_fake, kind)
            mref = mc.ref(seen(mc))
            assert R.skip_share(mref, 64, *full, True) <= R.SKIP_CAP, kind
            if kind == "zero_row":
                assert float(mc.table[R.ZERO_ROW].abs().max()) == 0.0
            if kind == "own_row" and not shadow:       # <h, h> is the user's best score by Cauchy-Schwarz only among equal norms:
                assert torch.equal(mc.table[R.OWN_ROW0 + 3], mc.hidden[3, -1, :d_item])    # the row is there, bit for bit


def _shape_cases():
    """(name, case, route, [(k, lo, hi)], seed of the exclusion rows and targets or None) of tests/test_gpu_rank_shapes.py, with
    the catalog sizes the plan gives at 256 CUs"""
    full = (0, R.N_ITEMS + 1)
    for d, route in R.SHAPE_WIDTHS:
        for B in R.SHAPE_BATCHES:
            yield f"tail {d} {route} {B}", R.tail_case(d, B), route, [(10,) + full, (64,) + full], B
        hi = R.ONE_CHUNK_ITEMS + 1
        yield f"one chunk {d} {route}", R.one_chunk_case(d), route, [(k, 0, hi) for k in (1, 10, 64)], None
        for rows in R.EXHAUSTIVE_ROWS + (R.K50_THRESHOLD_ROWS,):
            yield f"k50 {d} {route} {rows}", R.k50_case(d, rows), route, [(50, 0, rows)], d
        if R.is_stream16(d, route):
            for B in R.NU2_BATCHES:
                n = R.first_n_items(d, route, 0, B, 10, N_CU, R.is_nu2)
                yield f"nu2 {d} {route} {B}", R.nu2_case(d, n, B), route, [(10, 0, n + 1)], None
    n = R.first_n_items(50, "bf16", 0, R.B_WIDTHS, 10, N_CU, R.is_chunk512)
    yield "chunk512", R.chunk512_case(n), "bf16", [(10, 0, n + 1)], None
    d, B, n = R.WPB1
    yield "wpb1", R.base_case(d, 0, 0, n_items=n, B=B), "fp32", [(10, 0, n + 1)], None
    for d, route in R.SHARD_CASES:
        for ns in R.SHARD_COUNTS:
            yield f"sharded {d} {route} {ns}", R.sharded_case(d, ns), route, [(10,) + full, (64,) + full], None


def test_shape_cases_stay_under_the_cap():
    for name, c, route, calls, seed in _shape_cases():
        ref = c.ref(R.bf16_round(c.table) if route == "bf16" else c.table)
        for k, lo, hi in calls:
            assert R.skip_share(ref, k, lo, hi, True) <= R.SKIP_CAP, (name, k)
            if name.startswith("one chunk"):
                assert R.skip_share(ref, k, lo, hi, False) <= R.SKIP_CAP, (name, k)
            if seed is not None:
                rows = R.exclusion_rows(ref, lo, hi, c.n_items, seed)
                assert R.skip_share(ref, k, lo, hi, True, rows) <= R.SKIP_CAP, (name, k, "excl")
        if name.startswith(("tail", "nu2")):
            t = R.rank_targets(ref, c.B)
            lo, hi = calls[0][1:]
            rows = R.exclusion_rows(ref, lo, hi, c.n_items, c.B) if seed is not None else None
            assert R.check_rank(R.rank_ref(ref.s, t, lo, hi, True, rows), ref, t, lo, hi, True, rows) <= R.SKIP_CAP * c.B, name


def test_reference_functions():
    """topk_ref / rank_ref on a hand-made matrix: stable order, masks, trailing slots, the target's own exclusion"""
    s = np.array([[5.0, 1.0, 3.0, 3.0, 2.0, 9.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    idx, val = R.topk_ref(s, 3, 0, 6, True)
    assert idx.tolist() == [[5, 2, 3], [1, 2, 3]] and val[0].tolist() == [9.0, 3.0, 3.0]
    idx, val = R.topk_ref(s, 3, 0, 6, False, [[5, 5, -1, 77], []])
    assert idx.tolist() == [[0, 2, 3], [0, 1, 2]]
    idx, val = R.topk_ref(s, 4, 1, 3, True)
    assert idx.tolist() == [[2, 1, -1, -1], [1, 2, -1, -1]] and np.isneginf(val[:, 2:]).all()
    assert R.rank_ref(s, [2, 0], 0, 6, True).tolist() == [1, 0]             # item 0 (5.0) is the pad, 3.0 ties, 9.0 counts
    assert R.rank_ref(s, [2, 0], 0, 6, False).tolist() == [2, 0]
    assert R.rank_ref(s, [4, 4], 0, 6, False, [[4, 5], []]).tolist() == [3, 0]


# ------------------------------------------------------------------------------------------------ the bound is sharp
def _planes(x):
    p1 = R.bf16_round(x)
    r1 = x - p1
    p2 = R.bf16_round(r1)
    return p1, p2, R.bf16_round(r1 - p2)


SIX = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))       # (hidden plane, table plane), smallest product first


@pytest.mark.parametrize("d", [5, 32, 50, 64])
def test_bound_is_sharp(d):
    """On the width tests' own operands (fp32 table, the reference's top 64 of every user as the returned (b, i)):
    pass - an fp32 dot product in reversed channel order; an fp32 pairwise sum;
    fail for at least one returned (b, i) - the six-product sum of the three-plane split with any ONE product left out (the
    three smallest are 2^-16 of the largest: the bound tells a five-product kernel from a six-product one at every one of
    these widths, measured margins of the weakest product are printed); the hidden state rounded to one bf16 plane; column
    d_item - 1 dropped; h[d_item - 1] used once more against a pad of 1."""
    c = R.base_case(d)
    ref = c.ref()
    h, t = c.hidden[:, -1, :d], c.table
    idx, _ = R.topk_ref(ref.s, 64, 0, c.n_items + 1, True)
    tol = ref.eps * np.take_along_axis(ref.A, idx, 1)
    want = np.take_along_axis(ref.s, idx, 1)

    def worst(s):                                    # largest |s - s64| / bound over the returned (b, i)
        return float((np.abs(np.take_along_axis(np.asarray(s, np.float64), idx, 1) - want) / tol).max())

    rev = torch.zeros(c.B, c.n_items + 1)
    for k in reversed(range(d)):
        rev = rev + h[:, k:k + 1] * t[:, k]
    p = h[:, None, :] * t[None, :, :]
    p = torch.cat([p, torch.zeros(*p.shape[:2], 64 - d)], 2)
    while p.shape[2] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    assert worst(rev.numpy()) <= 1.0 and worst(p[..., 0].numpy()) <= 1.0
    hp, tp = _planes(h), _planes(t)
    prod = {q: hp[q[0]].double() @ tp[q[1]].double().T for q in SIX}
    assert worst(sum(prod.values()).numpy()) <= 1.0          # (all six: inside the bound, as the kernels claim)
    for q in SIX:
        w = worst(sum(v for qq, v in prod.items() if qq != q).numpy())
        print(f"d_item {d}: six products without (h{q[0] + 1}, e{q[1] + 1}): {w:.2f} x the bound")
        assert w > 1.0, (d, q, w)
    assert worst((R.bf16_round(h).double() @ t.double().T).numpy()) > 1.0
    hd, td = h.double().numpy(), t.double().numpy()
    assert worst(ref.s - hd[:, d - 1:d] * td[:, d - 1]) > 1.0
    assert worst(ref.s + hd[:, d - 1:d] * 1.0) > 1.0
