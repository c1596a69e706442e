"""-m gpu: the kernels that feed a run its batches and report its metric - srfrd_sample_batch, srfrd_eval_rank,
srfrd_check_ids, srfrd_topk_merge, srfrd_user_labels - against the plain references and case lists of
tests/data_path_refs.py (held to independent statements by tests/test_data_path_refs.py).  Integer or bit equality
throughout; the one floating-point sum (metric_acc[0]) is held to the bound of a B-term fp64 sum."""
import math

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests import data_path_refs as R

pytestmark = pytest.mark.gpu
SENTINEL = -7


# ------------------------------------------------------------------------------------------------------------------ sampler
_CSR = {}


def _device_csr(case):
    """(ptr int64, items int32, reviews int32) of a case's histories on the device, built once per history set"""
    key = id(case.hist)
    if key not in _CSR:
        ptr, items, usernum = R.csr(case.hist)
        _, revs, _ = R.csr(case.revs)
        assert usernum == case.usernum
        _CSR[key] = (case.hist, torch.from_numpy(ptr).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(revs).cuda())
    return _CSR[key][1:]


def _sample(case, batch=None):
    from srfrd_amd._lib import call
    ptr, items, revs = _device_csr(case)
    user = torch.full((case.B,), SENTINEL, device="cuda", dtype=torch.int64)
    packed = torch.full((6, case.B, case.L), SENTINEL, device="cuda", dtype=torch.int64)
    call("srfrd_sample_batch", user_ptr=ptr, items=items, reviews=revs, usernum=case.usernum, itemnum=case.itemnum, B=case.B,
         L=case.L, seed=case.seed, batch_index=case.batch if batch is None else batch, out_user=user, out_packed=packed)
    return user.cpu().numpy(), packed.cpu().numpy()


def _sampler_bit_exact(case):
    ru, rp = R.sampler_ref(case)
    user, packed = _sample(case)
    assert not (user == SENTINEL).any() and not (packed == SENTINEL).any(), case.name     # all 6 B L + B elements written
    bad = np.argwhere(packed != rp)
    assert (user == ru).all() and bad.size == 0, (case.name, user.tolist(), ru.tolist(), bad[:8].tolist())
    user2, packed2 = _sample(case)                                    # a second call: equal bits
    assert (user2 == user).all() and (packed2 == packed).all(), case.name
    return user, packed


@pytest.mark.parametrize("L", R.AROUND_LS)
def test_sample_batch_bit_exact_around_L(L):
    for case in R.around_L(L):
        _sampler_bit_exact(case)
    # another batch index gives another batch, and that one is the oracle's too (B = 5, seed 5: batch 0 -> 7)
    case = R.around_L(L)[4]
    _, packed = _sample(case)
    _, other = _sample(case, batch=7)
    assert (other == R.sampler_ref(case, batch=7)[1]).all() and not (other == packed).all()


def test_sample_batch_tiny_catalog_falls_back_to_a_history_item():
    case = R.tiny_catalog()
    user, packed = _sampler_bit_exact(case)
    assert set(user.tolist()) == {1, 2}
    for b in range(case.B):
        if user[b] == 1:                                              # all five items held: the 256th candidate, whatever it is
            assert ((packed[4, b] >= 1) & (packed[4, b] <= 5)).all()
        else:
            assert (packed[4, b] == R.TINY_FREE_ITEM).all()


def test_sample_batch_rows_without_an_eligible_user_come_out_all_pad():
    case = R.one_eligible()
    user, packed = _sampler_bit_exact(case)
    assert user.tolist() == R.ONE_ELIGIBLE_USERS
    for b in range(case.B):
        assert (user[b] == 4097) == bool(packed[:, b].any())


def test_sample_batch_distribution_is_uniform():
    case = R.uniformity()
    ru, rp = R.sampler_ref(case)
    cu, cn = R.uniformity_stats(case, ru, rp)
    assert cu < R.CHI2_999[19] and cn < R.CHI2_999[46]               # the reference alone, first (tests/test_data_path_refs.py)
    user, packed = _sample(case)
    assert (user == ru).all() and (packed == rp).all()
    chi_user, chi_neg = R.uniformity_stats(case, user, packed)
    print(f"chi-square users {chi_user:.2f} (19 dof), negatives {chi_neg:.2f} (46 dof)")
    assert chi_user < R.CHI2_999[19] and chi_neg < R.CHI2_999[46]


def test_device_sampler_at_maxlen_200_equals_the_oracle():
    import srfrd_amd
    case = R.around_L(200)[4]
    assert (case.B, case.seed, case.batch) == (5, 5, 0)
    ptr, items, usernum = R.csr(case.hist)
    _, revs, _ = R.csr(case.revs)
    z = np.zeros(usernum + 1, np.int32)
    data = srfrd_amd.InteractionData(usernum, case.itemnum, ptr, items, revs, z, z.copy())
    s = srfrd_amd.DeviceSampler(data, batch_size=case.B, maxlen=200, seed=case.seed)
    for batch in range(2):
        got = s.next_batch()
        ru, rp = R.sampler_ref(case, batch=batch)
        assert (got[0].cpu().numpy() == ru).all()
        for plane in range(6):
            assert got[1 + plane].shape == (case.B, 200) and (got[1 + plane].cpu().numpy() == rp[plane]).all(), (batch, plane)


# ---------------------------------------------------------------------------------------------------------------- eval_rank
def _metric_terms(ranks):
    return [1.0 / math.log2(r + 2.0) for r in ranks if r < 10]


def _check_acc(acc, ranks, calls, name):
    """acc after `calls` accumulations of the same rows: the counts exact, the NDCG sum inside the bound of an fp64 sum of
    calls * B terms in (0, 1], (terms + 2) * 2^-53 relative, whatever the order the atomics landed in"""
    a = acc.cpu().tolist()
    terms = _metric_terms(ranks) * calls
    want = math.fsum(terms)
    n = calls * len(ranks)
    print(f"{name}: acc {a}, fp64 sum {want!r}, |diff| {abs(a[0] - want):.3e}, bound {(n + 2) * 2.0 ** -53 * want:.3e}")
    assert a[2] == float(n) and a[1] == float(len(terms)), (name, a)
    assert abs(a[0] - want) <= (n + 2) * 2.0 ** -53 * want, (name, a[0], want)


@pytest.mark.parametrize("case", R.rank_cases(), ids=lambda c: c.name)
def test_eval_rank_equals_rank_ref(case):
    from srfrd_amd import ranks_from_logits
    from srfrd_amd._lib import call
    want = list(case.ranks)
    B, n = case.logits.shape
    logits = torch.from_numpy(case.logits.copy()).cuda()
    keep = logits.clone()
    # ranks_from_logits with the metric sums; twice: the second call adds to acc
    acc = torch.zeros(3, device="cuda", dtype=torch.float64)
    r1 = ranks_from_logits(logits, acc)
    assert r1.dtype == torch.int32 and r1.cpu().tolist() == want
    _check_acc(acc, want, 1, case.name)
    r2 = ranks_from_logits(logits, acc)
    assert r2.cpu().tolist() == want
    _check_acc(acc, want, 2, case.name + " (second call)")
    # the op: metric_acc = NULL
    assert torch.ops.srfrd.eval_rank(logits).cpu().tolist() == want
    assert ranks_from_logits(logits).cpu().tolist() == want
    # the C entry with rank = NULL: the metric alone
    acc3 = torch.zeros(3, device="cuda", dtype=torch.float64)
    call("srfrd_eval_rank", logits=logits, B=B, n_cand=n, rank=None, metric_acc=acc3)
    _check_acc(acc3, want, 1, case.name + " (rank NULL)")
    assert torch.equal(logits.view(torch.int32), keep.view(torch.int32))


def test_eval_rank_nan_rows_are_misses():
    """a diverged model (every logit NaN) and a NaN target among finite competitors: rank n_cand - 1, no hit, NDCG 0"""
    from srfrd_amd import ranks_from_logits
    rows = torch.full((2, 101), float("nan"))
    rows[1, 1:] = torch.arange(100.0)
    acc = torch.zeros(3, device="cuda", dtype=torch.float64)
    r = ranks_from_logits(rows.cuda(), acc)
    assert r.cpu().tolist() == [100, 100] == R.rank_ref(rows.numpy())
    assert acc.cpu().tolist() == [0.0, 0.0, 2.0]


# ---------------------------------------------------------------------------------------------------------------- check_ids
@pytest.mark.parametrize("n", R.CHECK_N)
def test_check_ids_word_per_plane_position_and_value(n):
    from srfrd_amd._lib import call
    cases = [c for c in R.check_cases() if c.n == n]
    assert cases
    clean = [torch.from_numpy(p).cuda() for p in R.check_planes(n)]
    planes = [p.clone() for p in clean]
    for c in cases:
        for plane, pos, value in c.bad:
            planes[plane][pos] = value
        before = [p.clone() for p in planes]
        used = [planes[p] if c.others == "clean" or any(b[0] == p for b in c.bad) else None for p in range(6)]
        word = torch.tensor([c.preset], device="cuda", dtype=torch.int32)
        call("srfrd_check_ids", item_a=used[0], item_b=used[1], item_c=used[2], fake_a=used[3], fake_b=used[4], fake_c=used[5],
             n=n, n_items=c.n_items, fake_hi=c.fake_hi, err_word=word)
        assert int(word.item()) == c.expected, c.name
        assert all(torch.equal(a, b) for a, b in zip(planes, before)), c.name      # the input planes are unchanged
        for plane, pos, _ in c.bad:
            planes[plane][pos] = clean[plane][pos]
    assert all(torch.equal(a, b) for a, b in zip(planes, clean))


def test_check_ids_of_no_elements_returns_zero_and_writes_nothing():
    from srfrd_amd._lib import query
    bad = torch.full((4,), -1, device="cuda", dtype=torch.int64)
    for preset in (0, 5):
        word = torch.tensor([preset], device="cuda", dtype=torch.int32)
        rc = query("srfrd_check_ids", item_a=bad, item_b=None, item_c=None, fake_a=bad, fake_b=None, fake_c=None, n=0, n_items=60,
                   fake_hi=2, err_word=word)
        assert rc == 0 and int(word.item()) == preset


# --------------------------------------------------------------------------------------------------------------- topk_merge
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n_cand", R.MERGE_N)
def test_topk_merge_equals_merge_ref(n_cand):
    import srfrd_amd
    cases = [c for c in R.merge_cases() if c.idx.shape[1] == n_cand]
    assert len(cases) == len(R.MERGE_B) * len(R.MERGE_K)
    for c in cases:
        ids, pos = R.merge_ref(c.idx, c.val, c.k)
        idx, val = torch.from_numpy(c.idx.copy()).cuda(), torch.from_numpy(c.val.copy()).cuda()
        mi, mv = srfrd_amd.topk_merge(idx, val, c.k)
        assert mi.dtype == torch.int64 and tuple(mi.shape) == tuple(mv.shape) == (c.idx.shape[0], c.k)
        assert (mi.cpu().numpy() == ids).all(), c.name
        # values by bits: the input value at the reference's chosen position, -inf behind the live count
        src = torch.from_numpy(c.val.copy())
        p = torch.from_numpy(pos)
        want = torch.where(p >= 0, torch.gather(src, 1, p.clamp(min=0)), torch.full((), float("-inf")))
        assert torch.equal(_bits(mv.cpu()), _bits(want)), c.name
        assert ((mi.cpu() == -1) == (p < 0)).all()
        mi2, mv2 = srfrd_amd.topk_merge(idx, val, c.k)              # a second call: equal bits
        assert torch.equal(mi2, mi) and torch.equal(_bits(mv2), _bits(mv)), c.name
        assert torch.equal(idx.cpu(), torch.from_numpy(c.idx.copy())) and torch.equal(_bits(val.cpu()), _bits(src))


def test_topk_merge_refuses_more_than_4096_candidates():
    import srfrd_amd
    from srfrd_amd._lib import query
    idx = torch.arange(4097, device="cuda", dtype=torch.int64).repeat(2, 1)
    val = torch.zeros(2, 4097, device="cuda")
    with pytest.raises(RuntimeError, match="SRFRD_E_ARG"):
        srfrd_amd.topk_merge(idx, val, 10)
    # the C entry: the refusal comes back before anything is launched - the outputs keep their sentinels
    oi = torch.full((2, 10), SENTINEL, device="cuda", dtype=torch.int64)
    ov = torch.full((2, 10), float(SENTINEL), device="cuda")
    rc = query("srfrd_topk_merge", cand_idx=idx, cand_val=val, B=2, n_cand=4097, k=10, topk_idx=oi, topk_val=ov)
    torch.cuda.synchronize()
    assert rc == -1 and bool((oi == SENTINEL).all()) and bool((ov == float(SENTINEL)).all())


# -------------------------------------------------------------------------------------------------------------- user_labels
@pytest.mark.parametrize("L", R.LABEL_LS)
def test_user_labels_direct_at_long_windows(L):
    """get_Labels / user_labels called directly (not through the encoder) at one lane's share, the wave's width and its
    neighbours, and L = 200: every exact-decile window, one all-pad row; batches of all rows, 5 rows and 1 row"""
    import srfrd_amd
    rows = torch.cat([torch.zeros(1, L, dtype=torch.int64), R._decile_rows(L)])           # (row 0 is all-pad)
    models = [(kind, getattr(srfrd_amd, kind)(50, L, 50, nl, 0.0, 1, 1, "cuda").cuda())
              for kind, nl in (("SRFU_B", 3), ("SRFU_F", L + 1), ("SRFU_R", 11))]
    srfrn = srfrd_amd.SRFRN(50, L, 45, 5, 0.0, 1, 1, "cuda").cuda()
    for batch in (rows, rows[-5:], rows[:5], rows[:1], rows[-1:]):
        dev = batch.cuda()
        for kind, m in models:
            want = O.get_labels(kind, batch).to(torch.int64)
            got = m.get_Labels(dev).cpu()
            assert got.dtype == torch.int64 and torch.equal(got, want), (kind, L, tuple(batch.shape))
        assert torch.equal(srfrn.user_labels(dev).cpu(), O.srfrn_predict_label(batch).to(torch.int64)), (L, tuple(batch.shape))
    # the all-pad row of SRFU_R is 0 / 0 in the reference: pinned at the guarded 0
    assert int(models[2][1].get_Labels(rows[:1].cuda())[0]) == 0
