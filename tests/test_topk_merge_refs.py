"""CPU: the reference and the cases of tests/topk_merge_refs.py, before the GPU files rely on them.

merge_runs_ref against a plain Python sort on every case and against data_path_refs.merge_ref on that file's own cases; the
generator's runs are sorted by the order law (and the unsorted family is not, in exactly one run of one user); the special
cases hold what they name; the sharded cases are admissible on the fp64 reference alone (the share of slots left to near ties
stays under rank_refs.SKIP_CAP).  No GPU anywhere."""
import numpy as np
import pytest

from tests import data_path_refs as D
from tests import rank_refs as R
from tests import topk_allow_refs as A
from tests import topk_merge_refs as M


def _bits_equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def _check(case):
    want = M.merge_runs_ref(case.idx, case.val, case.k)
    assert _bits_equal(want, M.merge_runs_sorted(case.idx, case.val, case.k)), case.name
    S, B, n = case.idx.shape
    live = (case.idx >= 0).sum(axis=(0, 2))
    for b in range(B):
        kk = min(case.k, int(live[b]))
        assert (want[0][b, kk:] == -1).all() and np.isneginf(want[1][b, kk:]).all() and (want[0][b, :kk] >= 0).all(), case.name
    assert not (want[1].view(np.int32) == np.float32(-0.0).view(np.int32)).any(), case.name           # -0 is written as +0
    return want


@pytest.mark.parametrize("S, n", M.GRID)
def test_grid_cases_are_sorted_runs_and_the_reference_is_a_plain_sort(S, n):
    cases = M.grid_cases(S, n)
    assert {c.idx.shape[1] for c in cases} == set(M.BATCHES)
    for c in cases:
        assert c.idx.shape == c.val.shape == (S, c.idx.shape[1], n) and not c.path.any(), c.name
        assert 1 <= c.k <= M.K_MAX
        _check(c)
    ks = {c.k for c in cases}
    assert {1, min(n, M.K_MAX), min(M.K_MAX, S * n)} <= ks
    assert M.lds_bytes(S, n) == 8 * M.slots(S, n) > 0


def test_the_grid_reaches_the_cap_and_some_k_exceeds_its_candidates():
    assert (16, 1024) in M.GRID and M.slots(16, 1024) == M.CAP and len(M.GRID) == len(M.N_LISTS) * len(M.LIST_LENS)
    assert any(c.k > c.idx.shape[0] * c.idx.shape[2] for S, n in M.GRID if S * n < 200 for c in M.grid_cases(S, n))
    assert M.slots(3, 65) == 4 * 128 and M.slots(1, 1) == 1 and M.pow2ceil(1024) == 1024 and M.pow2ceil(1025) == 2048
    assert M.lds_bytes(17, 1024) == 0 and M.lds_bytes(0, 5) == 0 and M.lds_bytes(5, 0) == 0 and M.lds_bytes(1, M.CAP + 1) == 0


def test_special_cases_hold_what_they_name():
    cases = {c.name: c for c in M.special_cases()}
    for c in cases.values():
        assert not c.path.any(), c.name                     # all of them are sorted runs
        _check(c)
    c = cases["short_runs_k1024"]
    assert ((c.idx >= 0).sum(2)[[0, 5]] == np.array([[325] * 3, [0] * 3])).all() and np.isposinf(c.val[0, 0, 325:]).all()
    assert (M.merge_runs_ref(cases["all_empty"].idx, cases["all_empty"].val, 65)[0] == -1).all()
    oi, _ = M.merge_runs_ref(cases["one_user_all_empty"].idx, cases["one_user_all_empty"].val, 100)
    assert (oi[1] == -1).all() and (oi[0, :100] >= 0).all()
    oi, _ = _check(cases["all_tied_interleaved"])
    assert (oi == np.arange(1, 201)).all()
    oi, ov = _check(cases["signed_zeros"])
    assert oi.tolist() == [[3, 4, 9, 20, 30, 40]] and (ov.view(np.int32)[0, :4] == 0).all()
    oi, ov = _check(cases["infinities_denormals"])
    assert oi.tolist() == [[1, 6, 7, 2, 3, 8, 4, 5, 9, -1, -1, -1]]
    assert np.isposinf(ov[0, :2]).all() and np.isneginf(ov[0, 7:]).all() and ov[0, 4] == np.float32(1e-45) > 0 > ov[0, 6]
    oi, _ = _check(cases["largest_ids"])
    assert oi.tolist() == [[0, M.ID_MAX - 2, M.ID_MAX - 1, M.ID_MAX]]
    assert 8 * 4096 < 48 * 1024 < 8 * 8192 and {"lds_P4096", "lds_P8192"} <= set(cases)
    assert max(int(c.idx.max()) for S, n in ((8, 64),) for c in M.grid_cases(S, n)) == M.ID_MAX


def test_unsorted_cases_break_one_run_of_one_user():
    cases = M.unsorted_cases()
    assert len(cases) == 10 and {c.idx.shape[0] * c.idx.shape[2] for c in cases} >= {16 * 1024, 128}
    for c in cases:
        assert c.path.tolist() == [0, 1, 0], c.name
        S, B, n = c.idx.shape
        broken = [(s, b) for s in range(S) for b in range(B) if not M.is_sorted_run(c.idx[s, b], c.val[s, b])]
        assert len(broken) == 1 and broken[0][1] == 1, c.name
        _check(c)
    assert any("pair0" in c.name for c in cases) and any(c.name.endswith(f"pair{c.idx.shape[2] - 2}") for c in cases)


def test_the_sortedness_test_is_the_order_law():
    f = lambda i, v: M.is_sorted_run(np.array(i, np.int64), np.array(v, np.float32))
    assert f([1, 2, 3], [3, 2, 1]) and f([1, 2], [1, 1]) and f([2, 2], [1, 1]) and not f([2, 1], [1, 1]) and not f([1, 2], [1, 2])
    assert f([5, 7], [-0.0, 0.0]) and f([5, 7], [0.0, -0.0]) and not f([7, 5], [0.0, -0.0])
    assert f([1, -1, -1], [1, 9, 9]) and not f([1, -1, 2], [3, 9, 1]) and f([-1, -1], [0, 0]) and not f([-1, 4], [0, 0])
    assert f([1, 2], [-np.inf, -np.inf]) and f([1, 2, -1], [np.inf, -np.inf, 0])


def test_against_the_reference_of_the_narrow_merge_on_its_own_cases():
    """data_path_refs.merge_ref: (B, n_cand) unsorted candidates, k <= 64 - one list per user here"""
    n = 0
    for c in D.merge_cases():
        if c.idx.shape[1] > M.CAP:
            continue
        ids, pos = D.merge_ref(c.idx, c.val, c.k)
        oi, ov = M.merge_runs_ref(c.idx[None], c.val[None], c.k)
        assert np.array_equal(ids, oi), c.name
        for b in range(ids.shape[0]):
            live = pos[b] >= 0
            want = c.val[b, pos[b][live]] + np.float32(0.0)
            assert np.array_equal(ov[b, live].view(np.int32), want.view(np.int32)) and np.isneginf(ov[b, ~live]).all(), c.name
        n += 1
    assert n == len(D.merge_cases()) == 72


def test_one_case_per_refusal():
    names = [r[0] for r in M.REFUSALS]
    assert len(set(names)) == len(names) == 15
    assert sum(code == M.E_UNSUPPORTED for *_, code in M.REFUSALS) == 3
    for _, over, code in M.REFUSALS:
        if code == M.E_UNSUPPORTED:
            assert M.slots(over["n_lists"], over["list_len"]) > M.CAP


# ---- the sharded cases ----------------------------------------------------------------------------------------------------------
def _excl_rows(ref, B, n_shards, kind, with_sets):
    full = (0, R.N_ITEMS + 1)
    x = R.exclusion_rows(ref, *full, R.N_ITEMS, 11) if with_sets else None
    if kind is None:
        return x
    if kind == "groups":
        return A.union_rows(M.shard_group_masks(n_shards), M.shard_groups(B), x)
    return A.union_rows(M.shard_filter_mask(kind, n_shards), [0] * B, x)


def test_the_sharded_cases_are_admissible_on_the_reference_alone():
    calls = M.sharded_calls()
    assert {c[3] for c in calls} == {1, 3, 8} and {c[4] for c in calls} == {10, 65, 100, 1024}
    assert {c[5] for c in calls} == {None, "random_0.5", "none", "straddle", "groups"} and any(c[1] for c in calls)
    refs = {}
    for d, f, route, S, k, kind, sets in calls:
        key = (d, f, route == "bf16", S)
        if key not in refs:
            case = M.sharded_case(d, S, f)
            refs[key] = case.ref(R.bf16_round(case.table) if route == "bf16" else None)
        ref = refs[key]
        rows = _excl_rows(ref, ref.s.shape[0], S, kind, sets)
        assert R.skip_share(ref, k, 0, R.N_ITEMS + 1, True, rows) < R.SKIP_CAP, (d, f, route, S, k, kind, sets)


def test_the_shard_cuts_carry_a_tied_pair_and_the_straddling_block_crosses_one():
    for S in (3, 8):
        cuts = R.shard_cuts(S)
        case = M.sharded_case(50, S)
        for cut in cuts:
            assert (case.table[cut - 1] == case.table[cut]).all()
        m = M.shard_filter_mask("straddle", S)
        assert m[cuts[0] - 1] and m[cuts[0]] and int(m.sum()) == 300
        assert -(-(R.N_ITEMS + 1) // S) < 1024 or S < 3          # at 3 and 8 shards every k = 1024 list has trailing empties
    assert M.shard_group_masks(8).shape == (2, R.N_ITEMS + 1) and set(M.shard_groups(17).tolist()) == {0, 1}
