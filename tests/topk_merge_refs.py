"""Cases and the numpy reference of srfrd_topk_merge_runs (include/srfrd_hip_merge.h), and the sharded cases of the wide and the
filtered ShardedRanker routes.  No GPU, no srfrd_amd import at module level: tests/test_topk_merge_refs.py checks the
reference and the cases on the CPU, tests/test_gpu_topk_merge.py and tests/test_gpu_sharded_wide.py run them.

A case is a stack of lists: idx int64 / val fp32 (n_lists, B, list_len), k, and the path every user must report (0: its lists
were sorted runs and were merged, 1: one of them was not and everything was sorted)."""
import itertools
from collections import namedtuple

import numpy as np

from tests import rank_refs as R

CAP = 16_384                                    # keys of one launch: pow2ceil(n_lists) * pow2ceil(list_len)
K_MAX = 1024                                    # SRFRD_TOPK_WIDE_MAX
N_LISTS = (1, 2, 3, 8, 16)
LIST_LENS = (1, 63, 64, 65, 100, 128, 1024)
BATCHES = (1, 3)
ID_MAX = 2 ** 31 - 2
E_ARG, E_UNSUPPORTED = -1, -2

MergeRunsCase = namedtuple("MergeRunsCase", "name idx val k path")


def pow2ceil(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def slots(n_lists, list_len):
    return pow2ceil(n_lists) * pow2ceil(list_len)


def lds_bytes(n_lists, list_len):
    """srfrd_topk_merge_runs_lds_bytes restated"""
    if n_lists < 1 or list_len < 1 or slots(n_lists, list_len) > CAP:
        return 0
    return 8 * slots(n_lists, list_len)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def merge_runs_ref(idx, val, k):
    """idx / val (n_lists, B, list_len) -> (ids (B, k) int64, values (B, k) fp32): per user the candidates with idx >= 0, -0 as
    +0, by value descending and id ascending, the first k; -1 / -inf behind them.  The order of the input is not used."""
    idx, val = np.asarray(idx), np.asarray(val, np.float32)
    S, B, n = idx.shape
    oi, ov = np.full((B, k), -1, np.int64), np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        i, v = idx[:, b].reshape(-1), val[:, b].reshape(-1)
        live = i >= 0
        i, v = i[live], v[live] + np.float32(0.0)
        assert not np.isnan(v).any(), "merge_runs_ref is not defined for NaN"
        order = np.lexsort((i, -v.astype(np.float64)))[:k]
        oi[b, :order.size], ov[b, :order.size] = i[order], v[order]
    return oi, ov


def merge_runs_sorted(idx, val, k):
    """the same by a plain Python sort of (value negated, id) pairs"""
    idx, val = np.asarray(idx), np.asarray(val, np.float32)
    S, B, n = idx.shape
    oi, ov = np.full((B, k), -1, np.int64), np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        pairs = sorted((-(float(v) + 0.0), int(i)) for i, v in zip(idx[:, b].reshape(-1).tolist(), val[:, b].reshape(-1).tolist()) if i >= 0)
        for j, (nv, i) in enumerate(pairs[:k]):
            oi[b, j], ov[b, j] = i, np.float32(-nv) + np.float32(0.0)
    return oi, ov


def is_sorted_run(idx, val):
    """one list by the order law, empty slots last: what the kernel tests while it loads"""
    idx, val = np.asarray(idx), np.asarray(val, np.float32) + np.float32(0.0)
    live = idx >= 0
    m = int(live.sum())
    if not live[:m].all():
        return False
    v, i = val[:m].astype(np.float64), idx[:m]
    return bool(((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (i[:-1] <= i[1:]))).all())


def path_of(idx, val):
    S, B, _ = idx.shape
    return np.array([int(not all(is_sorted_run(idx[s, b], val[s, b]) for s in range(S))) for b in range(B)], np.int32)


# ---- sorted runs --------------------------------------------------------------------------------------------------------------------
def sort_run(idx, val):
    """a list by the order law, its empty slots last (their values kept: the kernel must not read them)"""
    key = np.where(idx >= 0, -(val.astype(np.float64) + 0.0), np.inf)
    order = np.lexsort((np.where(idx >= 0, idx, ID_MAX + 1), key))
    return idx[order], val[order]


def random_runs(rng, S, B, n, live=None):
    """(S, B, n) sorted runs: values rounded to a tenth (ties within and across runs), ids disjoint across a user's runs and up
    to ID_MAX; ``live(s, b)`` slots of a run are filled (default: all), the rest are -1 with +inf as their value"""
    idx, val = np.empty((S, B, n), np.int64), np.empty((S, B, n), np.float32)
    step = ID_MAX // (S * n)
    for b in range(B):
        ids = rng.permutation(S * n).astype(np.int64) * step
        ids[np.argmax(ids)] = ID_MAX
        ids = ids.reshape(S, n)
        for s in range(S):
            v = np.round(rng.randn(n), 1).astype(np.float32)
            i = ids[s].copy()
            m = n if live is None else live(s, b)
            i[m:], v[m:] = -1, np.inf
            idx[s, b], val[s, b] = sort_run(i, v)
    return idx, val


def _case(name, idx, val, k):
    idx, val = np.ascontiguousarray(idx, np.int64), np.ascontiguousarray(val, np.float32)
    path = path_of(idx, val)
    for a in (idx, val, path):
        a.setflags(write=False)
    return MergeRunsCase(name, idx, val, int(k), path)


def grid_ks(S, n):
    total = S * n
    ks = {1, min(n, K_MAX), min(K_MAX, total)}
    if total + 3 <= 200:
        ks.add(total + 3)                          # more slots than candidates
    return sorted(ks)


def grid_cases(S, n):
    """every B and k of one (n_lists, list_len): the k variants share the lists"""
    out = []
    for B in BATCHES:
        rng = np.random.RandomState(S * 100_000 + n * 10 + B)
        idx, val = random_runs(rng, S, B, n)
        out += [_case(f"S{S}_n{n}_B{B}_k{k}", idx, val, k) for k in grid_ks(S, n)]
    return out


GRID = [(S, n) for S, n in itertools.product(N_LISTS, LIST_LENS) if slots(S, n) <= CAP]


def swap_pair(case, s, b, j, name):
    """``case`` with slots j and j + 1 of list s of user b exchanged (they must differ by the order law)"""
    idx, val = case.idx.copy(), case.val.copy()
    assert idx[s, b, j] >= 0 and idx[s, b, j + 1] >= 0
    assert (float(val[s, b, j]) + 0.0, -int(idx[s, b, j])) != (float(val[s, b, j + 1]) + 0.0, -int(idx[s, b, j + 1]))
    idx[s, b, [j, j + 1]], val[s, b, [j, j + 1]] = idx[s, b, [j + 1, j]], val[s, b, [j + 1, j]]
    return _case(name, idx, val, case.k)


def special_cases():
    out = []
    rng = np.random.RandomState(77)
    # short runs with trailing empties (325 of 1024, the sharded k = 1024 shape), one run wholly empty, all empty
    idx, val = random_runs(rng, 8, 3, 1024, live=lambda s, b: 325 if s != 5 else 0)
    out += [_case("short_runs_k1024", idx, val, 1024), _case("short_runs_k100", idx, val, 100)]
    idx, val = random_runs(rng, 3, 3, 100, live=lambda s, b: (0, 1, 99)[s] if b != 1 else 0)
    out.append(_case("one_user_all_empty", idx, val, 100))
    idx, val = random_runs(rng, 2, 1, 65, live=lambda s, b: 0)
    out.append(_case("all_empty", idx, val, 65))
    # one value everywhere, the ids dealt round the runs: the output is the ids ascending
    S, n = 8, 128
    idx = (np.arange(n)[None, None, :] * S + np.arange(S)[:, None, None] + 1).repeat(3, 1).astype(np.int64)
    out.append(_case("all_tied_interleaved", idx, np.full((S, 3, n), 1.5, np.float32), 200))
    # -0 in one run against +0 in another, and both inside one run: equal values, ordered by id, written as +0
    idx = np.array([[[9, 20, 30]], [[3, 4, 40]]], np.int64)
    val = np.array([[[-0.0, 0.0, -1.0]], [[0.0, -0.0, -2.0]]], np.float32)
    out.append(_case("signed_zeros", idx, val, 6))
    # +inf, -inf with a valid id (a candidate, behind every finite value), denormals on both sides of zero
    tiny = np.float32(1e-45)
    idx = np.array([[[1, 2, 3, 4, 5, -1]], [[6, 7, 8, 9, -1, -1]]], np.int64)
    val = np.array([[[np.inf, 2 * tiny, tiny, -tiny, -np.inf, 7.0]], [[np.inf, 1.0, 0.0, -np.inf, np.inf, np.inf]]], np.float32)
    out += [_case("infinities_denormals", idx, val, 12), _case("infinities_denormals_k3", idx, val, 3)]
    # the largest ids
    idx = np.array([[[ID_MAX - 1, ID_MAX]], [[0, ID_MAX - 2]]], np.int64)
    out.append(_case("largest_ids", idx, np.ones((2, 1, 2), np.float32), 4))
    # both sides of the 48 KiB dynamic-LDS opt-in: P = 4096 (32 KiB) and P = 8192 (64 KiB); P = 16 384 is in the grid (16 x 1024)
    for S, n in ((4, 1024), (8, 1000)):
        idx, val = random_runs(rng, S, 3, n)
        out.append(_case(f"lds_P{slots(S, n)}", idx, val, 1024))
    return out


def unsorted_cases():
    """one adjacent pair exchanged inside one run of user 1 of three, at the run's first and its last pair: that user takes the
    full sort, the other two still merge"""
    out = []
    for S, n, s in ((8, 1024, 5), (3, 100, 0), (2, 65, 1), (1, 128, 0), (16, 1024, 15)):
        rng = np.random.RandomState(S * 31 + n)
        idx = np.empty((S, 3, n), np.int64)
        for b in range(3):
            idx[:, b] = (rng.permutation(S * n).astype(np.int64) + 1).reshape(S, n)
        val = np.sort(rng.randn(S, 3, n).astype(np.float32), axis=2)[:, :, ::-1]          # distinct values: every pair is strict
        base = _case(f"sorted_S{S}_n{n}", idx, val, min(K_MAX, n))
        assert not base.path.any()
        for j in (0, n - 2):
            c = swap_pair(base, s, 1, j, f"unsorted_S{S}_n{n}_run{s}_pair{j}")
            assert c.path.tolist() == [0, 1, 0]
            out.append(c)
    return out


# (n_lists, list_len, keyword overrides of the call, the code): one per refusal of the header
REFUSALS = (
    ("cand_idx", dict(cand_idx=None), E_ARG), ("cand_val", dict(cand_val=None), E_ARG), ("topk_idx", dict(topk_idx=None), E_ARG),
    ("topk_val", dict(topk_val=None), E_ARG), ("B0", dict(B=0), E_ARG), ("n_lists0", dict(n_lists=0), E_ARG),
    ("list_len0", dict(list_len=0), E_ARG), ("k0", dict(k=0), E_ARG), ("k1025", dict(k=K_MAX + 1), E_ARG),
    ("lists_overlap", dict(n_lists=2, list_len=100, list_stride=99), E_ARG), ("user_stride0", dict(user_stride=0), E_ARG),
    ("user_stride_negative", dict(user_stride=-100), E_ARG),
    ("17x1024", dict(n_lists=17, list_len=1024, list_stride=1 << 20), E_UNSUPPORTED),
    ("9x1025", dict(n_lists=9, list_len=1025, list_stride=1 << 20), E_UNSUPPORTED),
    ("1x16385", dict(n_lists=1, list_len=CAP + 1), E_UNSUPPORTED),
)


# ---- the sharded cases ------------------------------------------------------------------------------------------------------------
SHARD_ROUTES = list(R.SHARD_CASES) + [(50, "fp32_forced")]     # (d_item, route): the bf16 stream from both tables, the fp32 stream
SHARD_COUNTS = (1, 3, 8)
SHARD_KS = (65, 100, 1024)
SHARD_FILTERS = ("random_0.5", "none", "straddle")


def sharded_case(d, n_shards, d_fake=0):
    """rank_refs.sharded_case - 2601 rows, a bit-identical pair across every shard cut, leading every list - with SRFRN's side
    term when d_fake > 0"""
    if not d_fake:
        return R.sharded_case(d, n_shards)
    c = R.base_case(d, d_fake, n_shards, positive=True)
    for j, cut in enumerate(R.shard_cuts(n_shards)):
        c.table[[cut - 1, cut]] = 40.0 - j
    return c


def shard_filter_mask(kind, n_shards, seed=0):
    """bool (N_ITEMS + 1,): topk_allow_refs.filter_mask's kinds, and "straddle": one allowed block of 300 ids over a shard cut"""
    from tests import topk_allow_refs as A
    if kind != "straddle":
        return A.filter_mask(kind, R.N_ITEMS, seed)
    cuts = R.shard_cuts(n_shards) or [R.N_ITEMS // 2]
    m = np.zeros(R.N_ITEMS + 1, bool)
    m[cuts[0] - 150:cuts[0] + 150] = True
    return m


def shard_group_masks(n_shards):
    """two rows: density 0.5, and the block over the first cut"""
    return np.stack([shard_filter_mask("random_0.5", n_shards, 3), shard_filter_mask("straddle", n_shards)])


def shard_groups(B):
    return np.arange(B) % 2


def sharded_calls():
    """every (d, d_fake, route, n_shards, k, filter kind or None, exclusion sets) the GPU file ranks: its admissibility is
    asserted on the reference alone (tests/test_topk_merge_refs.py)"""
    out = []
    for (d, route), S in itertools.product(SHARD_ROUTES, SHARD_COUNTS):
        for k in SHARD_KS:
            out += [(d, 0, route, S, k, None, False), (d, 0, route, S, k, None, True)]
        for kind in SHARD_FILTERS:
            out += [(d, 0, route, S, 100, kind, False), (d, 0, route, S, 10, kind, False)]
        out += [(d, 0, route, S, 100, "random_0.5", True), (d, 0, route, S, 100, "groups", False)]
    for S in SHARD_COUNTS:
        out += [(45, 5, "fp32", S, 100, None, False), (45, 5, "bf16", S, 100, "random_0.5", False)]
    return out
