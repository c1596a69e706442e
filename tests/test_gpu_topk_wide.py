"""-m gpu: srfrd::logits_topk_wide, the exact full-catalog top-k for k up to 1024.

Every list is held to the fp64 host reference of tests/rank_refs.py under the bar of the k <= 64 ranking, unchanged: values
within 4 max(E32, 2^-23) A of s64 at the returned id, the reference's order wherever its gap exceeds twice that bound, the same
id set inside closer runs (at most SKIP_CAP of a case's filled slots; tests/test_topk_wide_refs.py proves the cap from the
reference alone), exact ties by ascending id, -1 / -inf behind the last rankable item.  The shapes are the smallest that reach
each seam: every required item width on the three table routes over 2601 rows at k = 65, 100 and 1024; the three planned paths
(fine group maxima, chunk maxima, no threshold) with the plan's kernels asserted before the launch; the fallback on mass ties,
beside users it must not disturb; ranges shorter than k and batch tails; the k <= 64 op beside it; a second call, a captured
graph and the two skew libraries giving the same bits; model.topk."""
import numpy as np
import pytest
import torch

from tests import rank_refs as R
from tests import topk_wide_refs as W

pytestmark = pytest.mark.gpu

FULL = (0, W.N_ITEMS + 1)
Tally = R.Tally


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _start(d, f, route, case, monkeypatch, what):
    R.set_route(monkeypatch, route)
    run = W.Runner(case, route)
    return run, run.ref(), Tally(f"wide {what} d_item {d} d_fake {f} {route}")


def _planned(run, route, k, lo, hi, excl=False, path=None):
    c = run.case
    return W.check_plan(W.plan(c.d_item, c.d_fake, c.n_items, route, c.B, k, lo, hi, excl, _n_cu()), path)


# ---- width cover ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", R.ROUTES)
@pytest.mark.parametrize("d, f", W.CASES)
def test_values_and_order_at_every_width(d, f, route, monkeypatch):
    run, ref, T = _start(d, f, route, R.base_case(d, f), monkeypatch, "base")
    rows = R.exclusion_rows(ref, *FULL, W.N_ITEMS, d)
    top3, _ = R.topk_ref(ref.s, 3, *FULL, True)
    for k in W.KS:
        _planned(run, route, k, *FULL, path=W.ALL if k == 1024 else W.FINE)
        a = T.topk(run, ref, k, *FULL, what=("k", k))
        assert W.same_bits(a, run.topk(k, *FULL)), (T.tag, k, "second call")
        idx, _ = T.topk(run, ref, k, *FULL, excl_rows=rows, what=("excl", k))
        for b in range(run.case.B - 1):
            assert not set(idx[b].tolist()) & set(top3[b].tolist()), (T.tag, b)
    T.topk(run, ref, 100, *FULL, exclude_pad=False, what="with item 0")
    T.close()


@pytest.mark.parametrize("route", R.ROUTES)
@pytest.mark.parametrize("d, f", W.CASES)
def test_exact_ties_and_nothing_but_real_items(d, f, route, monkeypatch):
    """bit-identical rows across the 256- and 512-row seams lead every list in id order with equal bits; with every true score
    <= -1, a zero-padded row, a stale row behind the tail, item 0 or a padding column would lead the list"""
    run, ref, T = _start(d, f, route, R.tie_case(d, f), monkeypatch, "ties")
    R.check_tie_case(run.case, run.table_seen())
    for k in W.KS:
        idx, val = T.topk(run, ref, k, *FULL, what=("ties", k))
        assert (idx[:, :11] == np.array(R.TIE_ORDER)).all(), (T.tag, k, idx[:, :11])
        bits = val.view(np.int32)
        for ids in (R.TIE_IDS_A, R.TIE_IDS_B, R.TIE_EDGE):
            at = [R.TIE_ORDER.index(i) for i in ids]
            assert (bits[:, at] == bits[:, at[:1]]).all(), (T.tag, k, "identical rows, different scores")
    T.close()
    leak = R.leak_case(d, f)
    ref, T = run.load(leak).ref(), Tally(f"wide leak d_item {d} d_fake {f} {route}")
    for lo, hi in R.LEAK_RANGES + (FULL,):
        idx, val = T.topk(run, ref, 100, lo, hi, what="leak")
        assert (idx >= max(lo, 1)).all() and (idx < hi).all() and (val <= -1.0 + 1e-3).all(), T.tag
        # the planted rows lead (the best in the last row of its chunk; the bf16 shadow rounds the first four to one row value,
        # an exact tie that goes to the lowest id): the reference's own leader, nothing from behind the tail or from padding
        assert (idx[:, 0] == R.topk_ref(ref.s, 1, lo, hi, True)[0][:, 0]).all(), T.tag
    T.close()


# ---- the planned paths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route, B, k", W.CHUNK_CASES)
def test_chunk_maxima_path(d, route, B, k, monkeypatch):
    rows = W.first_rows(d, route, B, k, W.CHUNK, _n_cu())
    run, ref, T = _start(d, 0, route, R.base_case(d, 0, k, n_items=rows - 1, B=B), monkeypatch, f"chunk rows {rows}")
    _, cap, groups = _planned(run, route, k, 0, rows, path=W.CHUNK)
    assert groups >= 2 * k
    T.topk(run, ref, k, 0, rows, what="chunk")
    T.close()


@pytest.mark.parametrize("d, route", W.RANGE_WIDTHS)
def test_no_threshold_path_and_a_catalog_shorter_than_k(d, route, monkeypatch):
    run, ref, T = _start(d, 0, route, R.one_chunk_case(d), monkeypatch, "one chunk")
    n = W.ONE_CHUNK_ITEMS
    _planned(run, route, 100, 0, n + 1, path=W.ALL)
    idx, val = T.topk(run, ref, 100, 0, n + 1, what="17 items")
    assert (idx[:, :n - 1] >= 1).all() and (idx[:, n:] == -1).all() and np.isneginf(val[:, n:]).all() and (idx[:, n - 1] >= 1).all()
    idx, _ = T.topk(run, ref, 1024, 0, n + 1, exclude_pad=False, what="17 items with item 0")
    assert (np.sort(idx[:, :n + 1], axis=1) == np.arange(n + 1)).all() and (idx[:, n + 1:] == -1).all()
    T.close()


@pytest.mark.parametrize("d, route", W.FALLBACK_CASES)
def test_fallback_on_mass_ties_leaves_the_other_users_alone(d, route, monkeypatch):
    """a table of identical rows one row larger than the capacity: every list is the first k rankable ids.  Then one user with
    a zero hidden state among ordinary ones: its list is the ids ascending at value 0 (its capacity + 1 tied candidates
    overflow), the other users' lists are, bit for bit, those of the same call without that user"""
    cap = W.capacity()
    rows = cap + 1
    run, ref, T = _start(d, 0, route, W.identical_rows_case(d, rows), monkeypatch, "identical rows")
    ref.s[:], ref.A[:] = ref.s[:, 1:2], ref.A[:, 1:2]     # one row, one score: a blocked fp64 matmul may differ in its last bit by column
    for k in (100, 1024):
        _planned(run, route, k, 0, rows, path=W.FINE)
        idx, val = T.topk(run, ref, k, 0, rows, exclude_pad=False, what="all tied")
        assert (idx == np.arange(k)).all() and (val.view(np.int32) == val.view(np.int32)[:, :1]).all(), (T.tag, k)
        idx, _ = T.topk(run, ref, k, 5, rows, what="all tied, a range")
        assert (idx == np.arange(5, 5 + k)).all(), (T.tag, k)
    T.close()
    zero = W.zero_user_case(d, rows)
    ref, T = run.load(zero).ref(), Tally(f"wide zero user d_item {d} {route}")
    lists = {}
    for k in (100, 1024):
        idx, val = lists[k] = T.topk(run, ref, k, 0, rows, exclude_pad=False, what="zero user")
        assert (idx[1] == np.arange(k)).all() and (val[1] == 0.0).all(), (T.tag, k)
    T.close()
    two = W.Runner(W.without_user(zero, 1), route)
    for k in (100, 1024):
        idx, val = two.topk(k, 0, rows, exclude_pad=False)
        assert W.same_bits((lists[k][0][[0, 2]], lists[k][1][[0, 2]]), (idx, val)), (T.tag, k, "a user's overflow changed its neighbours")


# ---- ranges and tails ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route", W.RANGE_WIDTHS)
def test_ranges_shorter_than_k_and_every_row_alignment(d, route, monkeypatch):
    run, ref, T = _start(d, 0, route, R.base_case(d), monkeypatch, "ranges")
    for lo, hi in R.ranges():
        T.topk(run, ref, 100, lo, hi, what="range")
        if lo == 0:
            T.topk(run, ref, 100, lo, hi, exclude_pad=False, what="range with item 0")
    sub = (257, 257 + 300)
    T.topk(run, ref, 100, *sub, excl_rows=R.exclusion_rows(ref, *sub, W.N_ITEMS, d + 1), what="excl range")
    T.close()


@pytest.mark.parametrize("B", W.TAIL_BATCHES)
@pytest.mark.parametrize("d, route", W.RANGE_WIDTHS)
def test_batch_tails(d, route, B, monkeypatch):
    run, ref, T = _start(d, 0, route, R.tail_case(d, B), monkeypatch, f"B {B}")
    T.topk(run, ref, 100, *FULL, what="tail")
    T.topk(run, ref, 100, *FULL, excl_rows=R.exclusion_rows(ref, *FULL, W.N_ITEMS, B), what="tail excl")
    T.close()


# ---- beside the k <= 64 op -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route", W.BESIDE_CASES)
def test_beside_the_narrow_op(d, route, monkeypatch):
    """the wide list at k = 64 and the head of the k = 100 list against logits_topk at k = 64 (which takes the exhaustive path
    here): the same ids up to near ties.  The count of values that differ in bits is printed, not asserted."""
    run, ref, T = _start(d, 0, route, R.base_case(d), monkeypatch, "beside")
    ni, nv = run.narrow(64, *FULL)
    T.add(ni, nv, ref, 64, *FULL, what="narrow")
    wi, wv = T.topk(run, ref, 64, *FULL, what="wide 64")
    hi_, hv = T.topk(run, ref, 100, *FULL, what="wide 100")
    s1, b1 = R.check_same_lists(wi, wv, ni, nv, ref, tag=T.tag)
    s2, b2 = R.check_same_lists(hi_[:, :64], hv[:, :64], ni, nv, ref, tag=T.tag)
    print(f"WIDE_BESIDE {T.tag}: k 64 swaps {s1} bit-different values {b1}; head of k 100 swaps {s2} bit-different values {b2}")
    T.close()


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route, k", [(50, "fp32", 100), (50, "bf16", 1024)])
def test_a_captured_call_replays_on_new_hidden_states(d, route, k, monkeypatch):
    R.set_route(monkeypatch, route)
    cases = [R.base_case(d, 0, s) for s in (0, 1)]
    run = W.Runner(cases[0], route)
    rows = R.exclusion_rows(run.ref(), *FULL, W.N_ITEMS, d)
    eager = []
    for c in cases:
        hidden = c.hidden.cuda().contiguous()
        eager.append([t.clone() for t in run.topk_dev(k, *FULL, True, rows, hidden=hidden)])
    torch.cuda.synchronize()
    static = cases[0].hidden.cuda().contiguous()
    x = run._excl(rows)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.ops.srfrd.logits_topk_wide(static, run.ulab, run.key, *FULL, k, True, *x)
    for c, want in list(zip(cases, eager))[::-1] + list(zip(cases, eager)):
        static.copy_(c.hidden.cuda())
        out[0].fill_(-7)
        out[1].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1].view(torch.int32), want[1].view(torch.int32))


# ---- skewed barriers ----------------------------------------------------------------------------------------------------------------
def _skew_runs():
    """one case per path - fine groups, no threshold (both also with an exclusion set), chunk maxima, fallback - on both
    streams -> [(list as numpy)]"""
    out = []
    for d, route in ((50, "fp32"), (50, "bf16"), (60, "fp32")):
        run = W.Runner(R.base_case(d), route)
        rows = R.exclusion_rows(run.ref(), *FULL, W.N_ITEMS, d)
        out += [run.topk(100, *FULL), run.topk(1024, *FULL), run.topk(100, *FULL, excl_rows=rows)]
    d, route, B, k = W.CHUNK_CASES[0]
    rows = W.first_rows(d, route, B, k, W.CHUNK, _n_cu())
    run = W.Runner(R.base_case(d, 0, k, n_items=rows - 1, B=B), route)
    _planned(run, route, k, 0, rows, path=W.CHUNK)
    out.append(run.topk(k, 0, rows))
    cap = W.capacity()
    run = W.Runner(W.zero_user_case(8, cap + 1), "fp32")
    out.append(run.topk(100, 0, cap + 1, exclude_pad=False))
    return out


@pytest.mark.parametrize("lib", ["even", "odd"])
def test_same_bits_under_skewed_barriers(lib, monkeypatch):
    from tests import skew_cases as S
    monkeypatch.delenv("SRFRD_TOPK_FP32", raising=False)
    want = _skew_runs()
    mask = S.libraries()[lib][2]
    with S.use(lib) as rec:
        assert rec._handle.srfrd_skew_mask(None, None) == mask != 0
        got = _skew_runs()
    assert {"srfrd_logits_topk_wide", "srfrd_topk_wide_workspace_bytes"} <= rec.called
    for i, (a, b) in enumerate(zip(want, got)):
        assert W.same_bits(a, b), (lib, i)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_model_topk_is_the_op_on_the_models_last_hidden_state():
    import srfrd_amd
    from srfrd_amd import ops
    torch.manual_seed(0)
    (I, B, k), L = W.MODEL_CASE, 20
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda").to("cuda").eval()
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=5, device="cuda")
    idx, val = m.topk(None, seq, rsq, k=k, exclude="input")
    hidden, ulab, excl = m._rank_inputs(seq, rsq, "input")
    oi, ov = torch.ops.srfrd.logits_topk_wide(hidden, ulab, ops.register_model(m), 0, I + 1, k, True, *excl)
    assert torch.equal(idx, oi) and torch.equal(val.view(torch.int32), ov.view(torch.int32))
    assert idx.shape == (B, k) and (idx >= 1).all() and (val[:, :-1] >= val[:, 1:]).all()
    for b in range(B):
        assert not set(idx[b].tolist()) & set(seq[b][seq[b] != 0].tolist())
    with pytest.raises(ValueError, match="TOPK_WIDE_MAX"):
        m.topk(None, seq, rsq, k=1025)
