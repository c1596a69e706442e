"""CPU only: the references and case lists of tests/data_path_refs.py against independent statements of the same operations
(torch's argsort, numpy's lexsort, the sampler's invariants of reference utils.py:27-57), so that the GPU tests of
tests/test_gpu_data_path.py compare the kernels with something that was itself checked."""
import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests import data_path_refs as R


# ---------------------------------------------------------------------------------------------------------------- eval_rank
def test_rank_cases_cover_the_listed_shapes_and_state_their_ranks():
    cases = R.rank_cases()
    assert {c.logits.shape[0] for c in cases} >= {1, 3, 4, 5, 300}
    assert {c.logits.shape[1] for c in cases} >= {1, 2, 63, 64, 65, 101, 129}
    ranks = [r for c in cases for r in c.ranks]
    assert 9 in ranks and 10 in ranks
    for c in cases:
        assert c.logits.dtype == np.float32
        assert R.rank_ref(c.logits) == list(c.ranks), c.name       # the ranks written out by hand


def test_rank_ref_equals_torch_argsort_without_ties():
    n_rows = 0
    for c in R.rank_cases():
        x = torch.from_numpy(c.logits.copy())
        want = R.rank_ref(c.logits)
        for b in range(x.shape[0]):
            row = x[b]
            nan_target_only = bool(row[0] != row[0]) and bool((row[1:] == row[1:]).all()) and bool(torch.isfinite(row[1:]).all())
            plain = not bool(torch.isnan(row).any()) and not bool((row[1:] == row[0]).any())
            if not (plain or nan_target_only):
                continue
            got = int((-row).argsort(stable=True).argsort()[0])
            assert got == want[b], (c.name, b)
            n_rows += 1
    assert n_rows > 200                                                # (200 of B300_n101's rows alone carry no tie)
    # the row the issue names: a NaN target among finite competitors sorts last
    x = torch.tensor([float("nan")] + [float(j) for j in range(100)])
    assert int((-x).argsort(stable=True).argsort()[0]) == 100 == R.rank_ref(x.numpy()[None])[0]


def test_oracle_rank_of_first_equals_rank_ref_on_every_case():
    for c in R.rank_cases():
        got = O.rank_of_first(torch.from_numpy(c.logits.copy()))
        assert got.tolist() == list(c.ranks), c.name
    # and the metric of the two NaN rows at 101 candidates: misses
    nan_rows = torch.full((2, 101), float("nan"))
    nan_rows[1, 1:] = torch.arange(100.0)
    assert O.hr_ndcg_at_10(O.rank_of_first(nan_rows)) == (0.0, 0.0)


# --------------------------------------------------------------------------------------------------------------- topk_merge
def test_merge_cases_cover_the_listed_shapes():
    cases = R.merge_cases()
    assert len(cases) == len(R.MERGE_N) * len(R.MERGE_B) * len(R.MERGE_K) == 72
    assert max(int(c.idx.max()) for c in cases) == 2 ** 31 - 2
    kinds = {"inf": 0, "ninf": 0, "zero_pair": 0, "empty_row": 0, "few_row": 0, "k_over_n": 0}
    for c in cases:
        live = c.idx >= 0
        assert not np.isnan(c.val).any()
        kinds["inf"] += int((np.isposinf(c.val) & live).any())
        kinds["ninf"] += int((np.isneginf(c.val) & live).any())
        kinds["empty_row"] += int((~live).all(axis=1).any())
        kinds["few_row"] += int(((live.sum(axis=1) > 0) & (live.sum(axis=1) < c.k)).any())
        kinds["k_over_n"] += int(c.k > c.idx.shape[1])
        for b in range(c.idx.shape[0]):
            ids = c.idx[b][live[b]]
            assert len(set(ids.tolist())) == ids.size               # ids are unique inside a row
            z = c.val[b][live[b] & (c.val[b] == 0)]
            kinds["zero_pair"] += int(z.size >= 2 and np.signbit(z).any() and not np.signbit(z).all())
    assert all(v > 0 for v in kinds.values()), kinds


def test_merge_ref_equals_lexsort_without_signed_zero_ties():
    n_rows = 0
    for c in R.merge_cases():
        ids, pos = R.merge_ref(c.idx, c.val, c.k)
        for b in range(c.idx.shape[0]):
            live = np.flatnonzero(c.idx[b] >= 0)
            z = c.val[b][live][c.val[b][live] == 0]
            if z.size and np.signbit(z).any() and not np.signbit(z).all():
                continue
            order = live[np.lexsort((c.idx[b][live], -c.val[b][live].astype(np.float64)))][:c.k]
            assert pos[b, :order.size].tolist() == order.tolist(), (c.name, b)
            assert (pos[b, order.size:] == -1).all() and (ids[b, order.size:] == -1).all()
            assert ids[b, :order.size].tolist() == c.idx[b][order].tolist()
            n_rows += 1
    assert n_rows > 100
    # the +0 / -0 tie by hand: equal values, the lower id first, whichever sign it carries
    idx = np.array([[7, 3, 9], [3, 7, 9]], np.int64)
    val = np.array([[0.0, -0.0, -1.0], [0.0, -0.0, -1.0]], np.float32)
    ids, pos = R.merge_ref(idx, val, 2)
    assert ids.tolist() == [[3, 7], [3, 7]] and pos.tolist() == [[1, 0], [0, 1]]


# ---------------------------------------------------------------------------------------------------------------- check_ids
def test_check_cases_cover_the_listed_edges():
    cases = R.check_cases()
    assert 100 <= len(cases) <= 160
    assert {c.n for c in cases} == set(R.CHECK_N)
    for n in (131073, 262149):
        for plane in range(6):
            assert any(c.n == n and c.expected and c.bad == ((plane, n - 1, c.bad[0][2]),) for c in cases), (n, plane)
            assert any(c.n == n and c.expected and c.bad[0][:2] == (plane, 131072) for c in cases), (n, plane)
    assert all(any(c.n == 131072 and c.bad and c.bad[0][:2] == (plane, 131071) for c in cases) for plane in range(6))
    assert {c.expected for c in cases} >= {0, 1, 2, 3, 4, 5, 6, 7}
    assert {c.others for c in cases} == {"null", "clean"}
    values = {v for c in cases if c.expected & 3 for _, _, v in c.bad}
    assert values >= {-1, 2 ** 32, 2 ** 63 - 1, -2 ** 63, 3, 2 ** 32 + 1, 2, 61, 2 ** 32 + 60, 2 ** 32 + 1}
    for c in cases:                                                    # the expected word, restated
        word = c.preset
        for plane, pos, v in c.bad:
            assert 0 <= pos < c.n
            word |= (1 if not 0 <= v <= c.n_items else 0) if plane < 3 else (2 if not 0 <= v <= c.fake_hi else 0)
        assert word == c.expected, c.name
    for n in (1, 65):
        planes = R.check_planes(n)
        assert all(p.min() >= 0 for p in planes) and all(p.max() <= 1 for p in planes[:3]) and all(p.max() <= 2 for p in planes[3:])


# ------------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("L", R.AROUND_LS)
def test_around_L_reference_keeps_the_sampler_invariants(L):
    cases = R.around_L(L)
    assert len(cases) == (12 if L == 65 else 8)
    lens = sorted(len(h) for h in cases[0].hist[1:])
    assert lens == sorted([0, 1, 2, 3, L, L + 1, L + 2, 2 * L + 7])
    filled_seen = set()
    for c in cases:
        user, p = R.sampler_ref(c)
        seq, rsq, pos, prs, neg, nrs = p
        for b in range(c.B):
            h = c.hist[int(user[b])]
            assert len(h) > 1                                       # every row's user has more than one item
            m = min(len(h) - 1, L)
            filled_seen.add(m)
            live = seq[b] != 0
            assert int(live.sum()) == m and live[L - m:].all()      # filled from the end
            assert seq[b][live].tolist() == h[len(h) - 1 - m:-1] and pos[b][live].tolist() == h[len(h) - m:]
            assert (rsq[b][live] > 0).all() and set(rsq[b][live].tolist()) <= {1, 2}
            assert ((neg[b] != 0) == live).all() and (nrs[b] == live).all() and ((pos[b] != 0) == live).all()
            assert not set(neg[b][live].tolist()) & set(h) and (neg[b][live] >= 1).all() and (neg[b][live] <= c.itemnum).all()
        assert (pos[:, :-1][seq[:, :-1] != 0] == seq[:, 1:][seq[:, :-1] != 0]).all()
    if L > 2:
        assert filled_seen >= {L - 1, L}
    # another batch index, another batch (B = 5)
    c = cases[4]
    assert not (R.sampler_ref(c)[1] == R.sampler_ref(c, batch=c.batch + 1)[1]).all()


def test_tiny_catalog_reference_falls_back_to_a_history_item():
    c = R.tiny_catalog()
    assert set(c.hist[1]) == {1, 2, 3, 4, 5} and set(c.hist[2]) == {1, 2, 3, 4} and len(c.hist[1]) > 5
    user, p = R.sampler_ref(c)
    assert set(user.tolist()) == {1, 2}                              # both users occur among the six rows
    for b in range(c.B):
        live = p[0, b] != 0
        assert live.all()                                            # L = 4 <= n - 1 for both users
        if user[b] == 1:
            assert ((p[4, b] >= 1) & (p[4, b] <= 5)).all()
        else:
            assert (p[4, b] == R.TINY_FREE_ITEM).all()


def test_one_eligible_reference_rows_find_the_user_or_come_out_all_pad():
    c = R.one_eligible()
    user, p = R.sampler_ref(c)
    assert user.tolist() == R.ONE_ELIGIBLE_USERS
    assert len(R.sampler_dicts(c)[0]) == 8192
    for b in range(c.B):
        if user[b] == 4097:
            assert p[0, b].tolist() == [0, 1, 2] and p[2, b].tolist() == [0, 2, 3] and (p[4, b, 1:] > 3).all()
        else:
            assert (p[:, b] == 0).all()                              # 4096 draws used up: all six planes pad
    assert sum(int(u) == 4097 for u in user) == 2


def test_uniformity_reference_is_uniform_at_the_fixed_seed():
    c = R.uniformity()
    assert sorted(len(h) for h in c.hist[1:]) == [1] * 20 + [3] * 20
    user, p = R.sampler_ref(c)
    chi_user, chi_neg = R.uniformity_stats(c, user, p)
    print(f"chi-square users {chi_user:.2f} (19 dof), negatives {chi_neg:.2f} (46 dof)")
    assert chi_user < R.CHI2_999[19] and chi_neg < R.CHI2_999[46]
    # the statistic does see a skew: every negative of one place moved to its neighbour
    bent = p.copy()
    for b in range(c.B):
        free = [i for i in range(1, 51) if i not in c.hist[int(user[b])]]
        if bent[4, b, 0] == free[0]:
            bent[4, b, 0] = free[1]
    assert R.uniformity_stats(c, user, bent)[1] > R.CHI2_999[46]


# ------------------------------------------------------------------------------------------------------------- user_labels
def test_decile_rows_hold_every_exact_decile_ratio():
    for L in R.LABEL_LS:
        rows = R._decile_rows(L)
        assert rows.shape[1] == L and rows.shape[0] >= 2
        n1, n2 = (rows == 1).sum(1), (rows == 2).sum(1)
        assert bool(((n1 + n2) >= 1).all())
        exact = (10 * n1) % (n1 + n2) == 0
        assert bool(exact.any())
        assert bool((O.get_labels("SRFU_R", rows)[exact] == (10 * n1 // (n1 + n2))[exact]).all())
