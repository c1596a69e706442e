"""-m gpu: item filters - srfrd_item_mask_pack, srfrd::logits_topk_allow and srfrd::target_rank_allow.

Every list is held to the fp64 host reference of tests/rank_refs.py under its unchanged bar (values within 4 max(E32, 2^-23) A of
s64 at the returned id, the order law, at most SKIP_CAP of a case's filled slots left to near ties), every rank to check_rank;
the filter folds into the reference's exclusion rows (tests/test_topk_allow_refs.py proves the cap from the reference alone).
Shapes: the packing at the word seams; every required item width on the three table routes over 2601 rows (no maxima: the
collection hook at every width); 20 001 rows, just over the capacity, under six filters (the threshold path); every row
alignment with the filter's edge on each side of a word boundary; three groups against their single-group calls; exclusion
sets, exclude_pad, SRFRN's side term and the bf16 shadow together; the filtered list as the first allowed entries of the
unfiltered ranking, bit for bit; the fallback beside users it must not disturb; the target rank; a captured graph and the two
skew libraries giving the same bits; the model methods."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rank_refs as R
from tests import topk_allow_refs as A

pytestmark = pytest.mark.gpu

FULL, BIG = (0, A.N_ITEMS + 1), (0, A.BIG_ITEMS + 1)
Tally = R.Tally
ONE = [0] * A.B


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _start(d, f, route, case, monkeypatch, what):
    R.set_route(monkeypatch, route)
    run = A.Runner(case, route)
    return run, run.ref(), Tally(f"allow {what} d_item {d} d_fake {f} {route}")


def _planned(run, route, k, lo, hi, excl=False, path=None):
    c = run.case
    return A.check_plan(A.plan(c.d_item, c.d_fake, c.n_items, route, c.B, k, lo, hi, excl, _n_cu()), path, excl)


def _topk(T, run, ref, filt, k, lo, hi, pad=True, excl_rows=None, group=None, what=""):
    """the filtered op's list, held to the reference with the filter folded into its exclusion rows"""
    idx, val = run.topk(filt, k, lo, hi, pad, excl_rows, group)
    T.add(idx, val, ref, k, lo, hi, pad, A.union_rows(filt.mask, ONE[:run.case.B] if group is None else group, excl_rows), what)
    return idx, val


def _rank(T, run, ref, filt, t, lo, hi, pad=True, excl_rows=None, group=None, dups=(), what=""):
    got = run.rank(filt, t, lo, hi, pad, excl_rows, group)
    assert got.dtype == np.int32 and got.shape == (len(t),)
    rows = A.union_rows(filt.mask, ONE[:run.case.B] if group is None else group, excl_rows)
    T.near += R.check_rank(got, ref, t, lo, hi, pad, rows, dups, tag=(T.tag, what))
    T.targets += len(t)
    return got


# ---- packing ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n_rows", A.PACK_ROWS)
def test_packing_is_the_numpy_restatement(n_rows, G):
    from srfrd_amd import _lib
    g = np.random.RandomState(n_rows + G)
    W = A.words_of(n_rows)
    assert _lib.query("srfrd_item_mask_words", n_rows=n_rows) == W
    words = torch.full((G, W), -1, device="cuda", dtype=torch.int32)              # a dirty buffer
    for density in (0.5, 1.0, 0.03):
        m = g.random_sample((G, n_rows)) < density
        _lib.call("srfrd_item_mask_pack", mask=torch.from_numpy(m).cuda().to(torch.uint8), n_groups=G, n_rows=n_rows, words=words)
        got = words.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, A.pack_ref(m)), (n_rows, G, density)
        assert (got[:, -1] == 0).all()
    if n_rows >= 2601:                                                            # a mask of other nonzero bytes, and the class
        import srfrd_amd
        m = g.randint(0, 3, (G, n_rows))
        f = srfrd_amd.ItemFilter(torch.from_numpy(m), n_rows - 1, "cuda")
        assert np.array_equal(f.words.cpu().numpy().view(np.uint32), A.pack_ref(m != 0))
        assert f.n_groups == G and f.counts.tolist() == (m != 0).sum(1).tolist() and f.words.dtype == torch.int32
        ids = [torch.from_numpy(np.nonzero(r)[0]) for r in m]
        f2 = srfrd_amd.ItemFilter.from_ids(ids, n_rows - 1, "cuda")
        assert torch.equal(f2.words, f.words)


# ---- width and route sweep: no maxima, the collection hook at every width ---------------------------------------------------------
@pytest.mark.parametrize("route", R.ROUTES)
@pytest.mark.parametrize("d, f", A.SWEEP_CASES)
def test_values_and_order_at_every_width(d, f, route, monkeypatch):
    run, ref, T = _start(d, f, route, R.base_case(d, f), monkeypatch, "sweep")
    filt = A.Filter(A.filter_mask("random_0.5", A.N_ITEMS, d), A.N_ITEMS)
    for k in A.SWEEP_KS:
        _planned(run, route, k, *FULL, path=A.ALL)
        a = _topk(T, run, ref, filt, k, *FULL, what=("k", k))
        assert (a[0][:, 0] >= 1).all()
    assert A.same_bits(a, run.topk(filt, 1024, *FULL)), (T.tag, "second call")
    _rank(T, run, ref, filt, R.rank_targets(ref, d), *FULL, what="rank")
    T.close()


# ---- the threshold path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", A.FILTERS)
@pytest.mark.parametrize("d, route", R.SHAPE_WIDTHS)
def test_threshold_path_under_every_filter(d, route, kind, monkeypatch):
    run, ref, T = _start(d, 0, route, R.base_case(d, 0, 1, n_items=A.BIG_ITEMS), monkeypatch, f"threshold {kind}")
    mask = A.filter_mask(kind, A.BIG_ITEMS, d)
    filt = A.Filter(mask, A.BIG_ITEMS)
    assert int(filt.f.counts[0]) == int(mask.sum())
    n_ok = int(mask[1:].sum())
    for k in A.BIG_KS:
        _planned(run, route, k, *BIG, path=A.FINE)
        idx, val = _topk(T, run, ref, filt, k, *BIG, what=(kind, k))
        filled = min(k, n_ok)
        assert (idx[:, :filled] >= 1).all() and (idx[:, filled:] == -1).all() and np.isneginf(val[:, filled:]).all(), (T.tag, k)
    if kind == "block":
        # the unfiltered wide list over the block as an item range: the same ids and value bits, so no user went to the
        # fallback (whose fp64 chain gives other bits) although 18 000 allowed ids sit in one run
        assert A.same_bits((idx, val), run.wide(1024, *A.BLOCK)), (T.tag, "block against the range")
    _rank(T, run, ref, filt, R.rank_targets(ref, d), *BIG, what="rank")
    T.close()


# ---- alignment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route", A.RANGE_WIDTHS)
def test_every_row_alignment_with_the_edge_at_a_word_boundary(d, route, monkeypatch):
    run, ref, T = _start(d, 0, route, R.base_case(d), monkeypatch, "alignment")
    t = R.rank_targets(ref, d)
    for edge in A.EDGES:
        filt = A.Filter(A.edge_mask(edge, A.N_ITEMS), A.N_ITEMS)
        for lo, hi in R.ranges():
            idx, _ = _topk(T, run, ref, filt, 100, lo, hi, what=("edge", edge, lo, hi))
            assert (idx[idx >= 0] >= max(edge, lo)).all()
        _rank(T, run, ref, filt, t, 3, A.N_ITEMS + 1, what=("edge rank", edge))
    T.close()


# ---- groups --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [A.N_ITEMS, A.BIG_ITEMS])
@pytest.mark.parametrize("d, route", A.RANGE_WIDTHS)
def test_three_groups_equal_their_single_group_calls(d, route, n_items, monkeypatch):
    full = (0, n_items + 1)
    run, ref, T = _start(d, 0, route, R.base_case(d, 0, 1 if n_items == A.BIG_ITEMS else 0, n_items=n_items), monkeypatch,
                         f"groups {n_items}")
    masks = A.group_masks(n_items)
    filt = A.Filter(masks, n_items)
    group = [b % 3 for b in range(A.B)]
    idx, val = _topk(T, run, ref, filt, 100, *full, group=group, what="three groups")
    t = R.rank_targets(ref, d)
    rk = _rank(T, run, ref, filt, t, *full, group=group, what="three groups rank")
    for g in range(3):
        one = filt.row(g)
        si, sv = run.topk(one, 100, *full)                                     # allow_group None on G = 1
        sr = run.rank(one, t, *full)
        users = [b for b in range(A.B) if group[b] == g]
        assert A.same_bits((idx[users], val[users]), (si[users], sv[users])), (T.tag, g)
        assert (rk[users] == sr[users]).all(), (T.tag, g)
    # group values are clamped like every id
    wild = [(-5, 0), (7, 2), (1 << 40, 2)]
    gi = np.array([g for g, _ in wild] + group[3:], np.int64)
    ci, cv = run.topk(filt, 100, *full, group=gi)
    ei, ev = run.topk(filt, 100, *full, group=[c for _, c in wild] + group[3:])
    assert A.same_bits((ci, cv), (ei, ev))
    T.close()


# ---- composition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [A.N_ITEMS, A.BIG_ITEMS])
@pytest.mark.parametrize("d, f, route", [(d, 0, r) for d, r in A.RANGE_WIDTHS] + [(d, f, r) for d, f in R.FAKE_CASES for r in ("fp32", "bf16")])
def test_filter_exclusion_sets_and_pad_together(d, f, route, n_items, monkeypatch):
    full = (0, n_items + 1)
    run, ref, T = _start(d, f, route, R.base_case(d, f, 1 if n_items == A.BIG_ITEMS else 0, n_items=n_items), monkeypatch,
                         f"composition {n_items}")
    mask = A.filter_mask("random_0.5", n_items, d)
    mask[0] = True                                                        # item 0 allowed: exclude_pad alone decides about it
    filt = A.Filter(mask, n_items)
    rows = R.exclusion_rows(ref, *full, n_items, d)
    _planned(run, route, 100, *full, excl=True)
    top3, _ = R.topk_ref(ref.s, 3, *full, True)
    idx, _ = _topk(T, run, ref, filt, 100, *full, excl_rows=rows, what="excl")
    for b in range(A.B - 1):
        assert not set(idx[b].tolist()) & set(top3[b].tolist()), (T.tag, b)
    if f == 0:
        idx, _ = _topk(T, run, ref, filt, 100, *full, pad=False, excl_rows=rows, what="excl, item 0 rankable")
        _topk(T, run, ref, filt, 100, *full, pad=False, what="item 0 rankable")
    t = R.rank_targets(ref, d)
    _rank(T, run, ref, filt, t, *full, excl_rows=rows, what="rank excl")
    T.close()


# ---- the same bits as the unfiltered ranking ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route", [(50, "fp32"), (50, "bf16"), (64, "fp32"), (50, "fp32_forced")])
def test_the_filtered_list_is_the_first_allowed_entries_of_the_whole_ranking(d, route, monkeypatch):
    run, ref, T = _start(d, 0, route, R.base_case(d), monkeypatch, "same bits")
    lo, hi = 300, 1300                                                    # 1000 rows: the wide list at k = 1024 is the whole ranking
    whole = run.wide(1024, lo, hi)
    assert (whole[0][:, :1000] >= lo).all() and (whole[0][:, 1000:] == -1).all()
    for kind in ("random_0.5", "random_0.05"):
        mask = A.filter_mask(kind, A.N_ITEMS, d)
        filt = A.Filter(mask, A.N_ITEMS)
        for k in (1, 10, 100, 1024):
            got = _topk(T, run, ref, filt, k, lo, hi, what=(kind, k))
            assert A.same_bits(got, A.first_allowed(whole, [mask] * A.B, k)), (T.tag, kind, k)
    T.close()


# ---- the fallback ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route", A.FALLBACK_CASES)
def test_fallback_under_a_filter_leaves_the_other_users_alone(d, route, monkeypatch):
    """one user's hidden state zeroed: its 17 143 allowed scores tie at 0 and overflow the list; the fallback gives the first k
    allowed ids in ascending order, and the other users' bits are those of the call without that user"""
    zero = A.zero_user_case(d, A.BIG_ITEMS)
    run, ref, T = _start(d, 0, route, zero, monkeypatch, "zero user")
    mask = A.fallback_mask(A.BIG_ITEMS)
    filt = A.Filter(mask, A.BIG_ITEMS)
    allowed = np.nonzero(mask)[0]
    lists = {}
    for k in (100, 1024):
        _planned(run, route, k, *BIG, path=A.FINE)
        idx, val = lists[k] = _topk(T, run, ref, filt, k, *BIG, what="zero user")
        assert (idx[1] == allowed[:k]).all() and (val[1] == 0.0).all(), (T.tag, k)
    T.close()
    two = A.Runner(A.without_user(zero, 1), route)
    for k in (100, 1024):
        idx, val = two.topk(filt, k, *BIG)
        assert A.same_bits((lists[k][0][[0, 2]], lists[k][1][[0, 2]]), (idx, val)), (T.tag, k, "a user's overflow changed its neighbours")


# ---- the target rank -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [A.N_ITEMS, A.BIG_ITEMS])
@pytest.mark.parametrize("d, route", A.RANGE_WIDTHS)
def test_target_rank_under_a_filter(d, route, n_items, monkeypatch):
    from srfrd_amd import _lib
    full = (0, n_items + 1)
    case = R.base_case(d, 0, 1 if n_items == A.BIG_ITEMS else 0, n_items=n_items)
    ref0 = case.ref(R.bf16_round(case.table) if route == "bf16" else None)
    t = R.rank_targets(ref0, d)
    # bit-identical copies of the first user's target row, allowed by the filter: never counted, for that user
    dups = (n_items // 3, n_items - 5)
    case.table[list(dups)] = case.table[int(t[0])].clone()
    run, ref, T = _start(d, 0, route, case, monkeypatch, f"rank {n_items}")
    mask = A.filter_mask("random_0.5", n_items, d)
    mask[list(dups)] = True
    mask[t[::2]] = False                                                  # every other target disallowed: still ranked
    mask[t[1::2]] = True
    filt = A.Filter(mask, n_items)
    rows = A.union_rows(mask, ONE)
    got = run.rank(filt, t, *full)
    T.near += R.check_rank(got[:1], R_first(ref), t[:1], *full, True, rows[:1], dups, tag=T.tag)
    T.near += R.check_rank(got[1:], R_rest(ref), t[1:], *full, True, rows[1:], (), tag=T.tag)
    T.targets += len(t)
    # ranks over three disjoint ranges add up to the whole
    cuts = [0, n_items // 3 + 1, 2 * n_items // 3 + 2, n_items + 1]
    parts = sum(run.rank(filt, t, a, b).astype(np.int64) for a, b in zip(cuts[:-1], cuts[1:]))
    assert (parts == got).all(), (T.tag, parts, got)
    # metric_acc accumulates as srfrd_target_rank's does
    acc = torch.zeros(3, device="cuda", dtype=torch.float64)
    rank = torch.empty(A.B, device="cuda", dtype=torch.int32)
    ws = torch.empty(max(_lib.query("srfrd_excl_workspace_bytes", B=A.B, max_row=0, n_rows=n_items + 1), 8), device="cuda", dtype=torch.uint8)
    from srfrd_amd import ops
    for _ in range(2):
        _lib.call("srfrd_target_rank_allow", **ops.rank_head(run.m, run.hidden, run.ulab, item_range=full, exclude_pad=True,
                                                              excl=(None, None, 0)),
                  targets=torch.as_tensor(t).cuda(), cut_k=10, rank=rank, metric_acc=acc, workspace=ws, allow_words=filt.f.words,
                  n_groups=1, words_per_group=filt.f.words.shape[1], allow_group=None)
    assert (rank.cpu().numpy() == got).all()
    hits = got[got < 10]
    want_acc = np.array([2 * (1.0 / np.log2(hits + 2.0)).sum(), 2.0 * len(hits), 2.0 * A.B])
    assert np.allclose(acc.cpu().numpy(), want_acc, rtol=1e-12, atol=0), (acc, want_acc)
    T.close()


def R_first(ref):
    """the reference restricted to the first user"""
    return _slice(ref, slice(0, 1))


def R_rest(ref):
    return _slice(ref, slice(1, None))


def _slice(ref, s):
    out = R.Ref.__new__(R.Ref)
    out.s, out.A, out.e32, out.unit, out.eps = ref.s[s], ref.A[s], ref.e32, ref.unit, ref.eps
    return out


# ---- graph capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, route, n_items, k", [(50, "fp32", A.N_ITEMS, 1024), (50, "bf16", A.BIG_ITEMS, 100), (64, "fp32", A.BIG_ITEMS, 1024)])
def test_a_captured_call_replays_with_the_eager_bits(d, route, n_items, k, monkeypatch):
    R.set_route(monkeypatch, route)
    full = (0, n_items + 1)
    cases = [R.base_case(d, 0, s, n_items=n_items) for s in (1, 2)]
    run = A.Runner(cases[0], route)
    _planned(run, route, k, *full, excl=True, path=A.ALL if n_items == A.N_ITEMS else A.FINE)
    filt = A.Filter(A.filter_mask("random_0.5", n_items, d), n_items)
    rows = R.exclusion_rows(run.ref(), *full, n_items, d)
    t = torch.as_tensor(R.rank_targets(run.ref(), d)).cuda()
    eager = []
    for c in cases:
        hidden = c.hidden.cuda().contiguous()
        lists = [x.clone() for x in run.topk_dev(filt, k, *full, True, rows, hidden=hidden)]
        rk = torch.ops.srfrd.target_rank_allow(hidden, run.ulab, t, run.key, *full, True, *run._excl(rows), filt.f.words, None).clone()
        eager.append(lists + [rk])
    torch.cuda.synchronize()
    static = cases[0].hidden.cuda().contiguous()
    x = run._excl(rows)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream
        out = torch.ops.srfrd.logits_topk_allow(static, run.ulab, run.key, *full, k, True, *x, filt.f.words, None)
        rk = torch.ops.srfrd.target_rank_allow(static, run.ulab, t, run.key, *full, True, *x, filt.f.words, None)
    for c, want in list(zip(cases, eager))[::-1] + list(zip(cases, eager)):
        static.copy_(c.hidden.cuda())
        out[0].fill_(-7)
        out[1].fill_(7.0)
        rk.fill_(-3)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], want[0]) and torch.equal(out[1].view(torch.int32), want[1].view(torch.int32))
        assert torch.equal(rk, want[2])


# ---- skewed barriers ----------------------------------------------------------------------------------------------------------------
def _skew_runs():
    """one case per path - no maxima, fine groups on both streams (with and without exclusion sets), the fallback - and the
    target rank and the packing beside them -> [arrays]"""
    out = []
    for d, route, n_items in ((50, "fp32", A.N_ITEMS), (50, "fp32", A.BIG_ITEMS), (50, "bf16", A.BIG_ITEMS), (60, "fp32", A.BIG_ITEMS)):
        full = (0, n_items + 1)
        run = A.Runner(R.base_case(d, 0, 1, n_items=n_items), route)
        filt = A.Filter(A.group_masks(n_items), n_items)
        group = [b % 3 for b in range(A.B)]
        rows = R.exclusion_rows(run.ref(), *full, n_items, d)
        t = R.rank_targets(run.ref(), d)
        out += [*run.topk(filt, 100, *full, group=group), *run.topk(filt, 1024, *full, True, rows, group),
                run.rank(filt, t, *full, group=group), run.rank(filt, t, *full, True, rows, group), filt.f.words.cpu().numpy()]
    run = A.Runner(A.zero_user_case(8, A.BIG_ITEMS), "fp32")
    out += [*run.topk(A.Filter(A.fallback_mask(A.BIG_ITEMS), A.BIG_ITEMS), 100, *BIG)]
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
    assert {"srfrd_logits_topk_allow", "srfrd_target_rank_allow", "srfrd_item_mask_pack", "srfrd_topk_allow_workspace_bytes"} <= rec.called
    assert len(want) == len(got)
    for i, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b), (lib, i)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def test_model_methods_are_the_ops_on_the_models_last_hidden_state():
    import srfrd_amd
    from srfrd_amd import ops
    torch.manual_seed(0)
    (I, B, k), L = A.MODEL_CASE, 20
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda").to("cuda").eval()
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=5, device="cuda")
    mask = torch.from_numpy(A.group_masks(I))
    filt = m.item_filter(mask)
    assert isinstance(filt, srfrd_amd.ItemFilter) and filt.n_groups == 3 and filt.words.is_cuda
    grp = torch.arange(B, dtype=torch.int64) % 3
    for kk in (10, k):                                                  # k <= 64 goes to the filtered op too
        idx, val = m.topk(None, seq, rsq, k=kk, exclude="input", allow=filt, allow_group=grp)
        hidden, ulab, excl = m._rank_inputs(seq, rsq, "input")
        oi, ov = torch.ops.srfrd.logits_topk_allow(hidden, ulab, ops.register_model(m), 0, I + 1, kk, True, *excl, filt.words, grp.cuda())
        assert torch.equal(idx, oi) and torch.equal(val.view(torch.int32), ov.view(torch.int32))
        assert idx.shape == (B, kk) and (idx >= 1).all() and (val[:, :-1] >= val[:, 1:]).all()
        for b in range(B):
            got = idx[b].cpu()
            assert mask[int(grp[b])][got].all() and not set(got.tolist()) & set(seq[b][seq[b] != 0].tolist())
    tg = idx[:, 3].clone()
    rk = m.target_rank(None, seq, rsq, tg, exclude="input", allow=filt, allow_group=grp)
    assert rk.dtype == torch.int32 and (rk.cpu() == 3).all()           # three allowed, not excluded items score higher than slot 3
    plain = m.topk(None, seq, rsq, k=kk, exclude="input")
    one = m.item_filter(torch.ones(I + 1, dtype=torch.bool))
    same = m.topk(None, seq, rsq, k=kk, exclude="input", allow=one)
    assert torch.equal(plain[0], same[0]) and torch.equal(plain[1].view(torch.int32), same[1].view(torch.int32))
    with pytest.raises(ValueError, match="allow_group is required"):
        m.topk(None, seq, rsq, k=10, allow=filt)
