"""Cases and plain references for the kernels that feed a run its batches and report its metric: srfrd_sample_batch,
srfrd_eval_rank, srfrd_check_ids, srfrd_topk_merge, srfrd_user_labels.  numpy and Python only: nothing here touches the
library or a device (tests/test_data_path_refs.py holds this file to independent statements on the CPU,
tests/test_gpu_data_path.py holds the kernels to it).

The sampler's reference is ``oracle.srfrd_oracle.sample_batch_ref``; this file only builds its inputs and caches its outputs.
``merge_ref`` is defined for values without NaN: what srfrd_topk_merge does with a NaN score stays undefined, and no case
holds one."""
import functools
import itertools
from collections import namedtuple

import numpy as np

from tests.token_neg_refs import csr  # noqa: F401  (histories -> CSR, for the callers of sampler_inputs)

# ------------------------------------------------------------------------------------------------------------------------
# srfrd_sample_batch
# ------------------------------------------------------------------------------------------------------------------------
SamplerCase = namedtuple("SamplerCase", "name hist revs usernum itemnum B L seed batch")
AROUND_LS = (1, 12, 63, 64, 65, 200)
SEED_BATCH = ((5, 0), (5, 1), (0xFFFFFFFF, 2 ** 32 - 3), (0, 2 ** 31))
UNIFORM_SEED = 20241020
CHI2_999 = {19: 43.8202, 46: 81.4003}                   # 99.9 % quantiles of chi-square (19 and 46 degrees of freedom)


def _reviews(rng, hist):
    return [rng.randint(1, 3, len(h)).tolist() for h in hist]


@functools.lru_cache(maxsize=None)
def _around_hist(L):
    """user 0 empty, then users of n in {0, 1, 2, 3, L, L + 1, L + 2, 2 L + 7} items out of 500: min(n - 1, L) covers 1, 2,
    L - 1, L, and L with a longer history behind it.  Every list of three or more items repeats its first item at the end."""
    rng = np.random.RandomState(1000 + L)
    hist = [[]]
    for n in (0, 1, 2, 3, L, L + 1, L + 2, 2 * L + 7):
        h = rng.randint(1, 501, n).tolist()
        if n >= 3:
            h[-1] = h[0]
        hist.append(h)
    return hist, _reviews(rng, hist)


def around_L(L):
    """the sampler cases at sequence length L: B in (1, 5), and 37 (ten workgroups, the last with one wave) at L = 65"""
    hist, revs = _around_hist(L)
    return [SamplerCase(f"around_L{L}_B{B}_s{seed:x}_b{batch:x}", hist, revs, len(hist) - 1, 500, B, L, seed, batch)
            for B in ((1, 5, 37) if L == 65 else (1, 5)) for seed, batch in SEED_BATCH]


def tiny_catalog():
    """five items.  User 1 holds all five, so each of its negatives is the 256th candidate - a history item; user 2 holds
    four, so each of its negatives is item 5"""
    hist = [[], [3, 1, 4, 1, 5, 2, 3], [2, 4, 1, 3, 4, 2]]
    revs = [[], [1, 2, 2, 1, 2, 1, 1], [2, 2, 1, 2, 1, 1]]
    return SamplerCase("tiny_catalog", hist, revs, 2, 5, 6, 4, 7, 3)


TINY_FREE_ITEM = 5


def one_eligible():
    """8192 users of one item each, except user 4097 ([1, 2, 3]): most rows use up their 4096 user draws"""
    hist = [[]] + [[1 + u % 10] for u in range(1, 8193)]
    hist[4097] = [1, 2, 3]
    revs = [[]] + [[1 + u % 2] for u in range(1, 8193)]
    revs[4097] = [2, 1, 2]
    return SamplerCase("one_eligible", hist, revs, 8192, 10, 8, 3, 11, 0)


ONE_ELIGIBLE_USERS = [4097, 3202, 2140, 2379, 4097, 1495, 7650, 6278]


def uniformity():
    """40 users, the odd ones with three distinct items, the even ones with one; 50 items; 4096 rows of one position"""
    rng = np.random.RandomState(77)
    hist = [[]] + [(rng.permutation(50)[:3] + 1).tolist() if u % 2 else [int(rng.randint(1, 51))] for u in range(1, 41)]
    return SamplerCase("uniformity", hist, _reviews(rng, hist), 40, 50, 4096, 1, UNIFORM_SEED, 0)


def sampler_dicts(case):
    """the histories as the oracle takes them: an entry for every user 1..usernum"""
    return ({u: case.hist[u] for u in range(1, case.usernum + 1)}, {u: case.revs[u] for u in range(1, case.usernum + 1)})


_SAMPLER_REFS = {}


def sampler_ref(case, batch=None):
    """(user (B,), packed (6, B, L)) int64 of the oracle, computed once per (case, batch index) and returned read-only"""
    from oracle import srfrd_oracle as O
    batch = case.batch if batch is None else batch
    key = (case.name, batch)
    if key not in _SAMPLER_REFS:
        ti, tr = sampler_dicts(case)
        user, packed = O.sample_batch_ref(ti, tr, case.usernum, case.itemnum, case.B, case.L, case.seed, batch)
        if case.name == "one_eligible":
            found = [int(u) == 4097 for u in user]
            assert any(found) and not all(found), "one_eligible must hold a row that finds the user and one that does not"
        user.setflags(write=False)
        packed.setflags(write=False)
        _SAMPLER_REFS[key] = (user, packed)
    return _SAMPLER_REFS[key]


def uniformity_stats(case, user, packed):
    """chi-square of the rows' users over the 20 eligible users (19 degrees of freedom) and of the negatives over the 47
    items outside a three-item history, each negative named by its place among its own user's 47 free items and the users
    pooled (46 degrees of freedom)"""
    user = np.asarray(user)
    neg = np.asarray(packed)[4, :, 0]
    eligible = [u for u in range(1, case.usernum + 1) if len(case.hist[u]) > 1]
    assert len(eligible) == 20 and set(user.tolist()) <= set(eligible)
    n = user.size
    cu = np.array([(user == u).sum() for u in eligible], np.float64)
    chi_user = float(((cu - n / 20) ** 2 / (n / 20)).sum())
    place = np.zeros(47, np.float64)
    for u in eligible:
        free = [i for i in range(1, case.itemnum + 1) if i not in case.hist[u]]
        assert len(free) == 47
        where = {item: p for p, item in enumerate(free)}
        for item in neg[user == u].tolist():
            place[where[item]] += 1                              # (KeyError: a negative inside the history, or 0)
    chi_neg = float(((place - n / 47) ** 2 / (n / 47)).sum())
    return chi_user, chi_neg


# ------------------------------------------------------------------------------------------------------------------------
# srfrd_eval_rank
# ------------------------------------------------------------------------------------------------------------------------
def rank_ref(logits):
    """float32 (B, n_cand) -> list of B ints: the number of j >= 1 with x_j > x_0 in IEEE arithmetic on the float32 values
    (a denormal is greater than 0, -0 is not less than +0, NaN compares false); n_cand - 1 when x_0 is NaN"""
    x = np.asarray(logits)
    assert x.dtype == np.float32 and x.ndim == 2
    out = []
    for row in x:
        x0 = row[0]
        if x0 != x0:
            out.append(len(row) - 1)
        else:
            out.append(sum(1 for v in row[1:] if v > x0))
    return out


RankCase = namedtuple("RankCase", "name logits ranks")
NAN, INF, DEN = float("nan"), float("inf"), 1e-40        # (1e-40 is a float32 denormal: 2^-126 is 1.18e-38)


def _f32(rows):
    return np.array(rows, dtype=np.float32)


def _spread(n_cand, x0, above, seed, equal=0, hi=None, lo=None, nan=0):
    """one row of n_cand values: x0 first, then `above` values greater than x0, `equal` copies of it, `nan` NaNs and the rest
    smaller, at shuffled places.  hi / lo: the value used above / below (default: x0 + 1, + 2, ... and x0 - 1, - 2, ...)"""
    rest = n_cand - 1 - above - equal - nan
    assert rest >= 0
    vals = ([x0 + 1 + i for i in range(above)] if hi is None else [hi] * above) + [x0] * equal + [NAN] * nan
    vals += [x0 - 1 - i for i in range(rest)] if lo is None else [lo] * rest
    order = np.random.RandomState(seed).permutation(n_cand - 1)
    return [x0] + [vals[i] for i in order]


@functools.lru_cache(maxsize=None)
def rank_cases():
    c = []
    # n_cand 1 and 2: nothing to count, and the three orders of two values
    c.append(RankCase("n1", _f32([[3.0]]), [0]))
    c.append(RankCase("n1_nan_B3", _f32([[NAN], [0.0], [-INF]]), [0, 0, 0]))
    c.append(RankCase("n2", _f32([[0.0, 1.0], [1.0, 0.0], [1.0, 1.0]]), [1, 0, 0]))
    # all-equal rows around the wave width
    for n in (63, 64, 65):
        c.append(RankCase(f"all_equal_n{n}", _f32([[2.5] * n, [0.0] * n, [-1e30] * n, [INF] * n]), [0, 0, 0, 0]))
    # the last candidate alone is greater (lane 62 / 63 of the first round, lane 0 and 63 of the second)
    for n in (2, 63, 64, 65, 101, 129):
        c.append(RankCase(f"last_only_n{n}", _f32([[1.0] + [0.0] * (n - 2) + [2.0]]), [1]))
    c.append(RankCase("first_of_round2_n129", _f32([[1.0] + [0.0] * 64 + [2.0] + [0.0] * 63,
                                                    [1.0] + [0.0] * 63 + [2.0] + [0.0] * 64,
                                                    [1.0] + [2.0] * 128, [1.0] + [2.0] * 64 + [0.0] * 64,
                                                    [1.0] + [0.0] * 64 + [2.0] * 64]), [1, 1, 128, 64, 64]))
    # infinities
    c.append(RankCase("target_pinf", _f32([[INF, 1.0, INF, -INF, 3e38], [INF, INF, INF, INF, INF],
                                           [INF, -1.0, 0.0, 1.0, 2.0]]), [0, 0, 0]))
    c.append(RankCase("target_ninf", _f32([[-INF, 1.0, INF, -INF, -3e38], [-INF, -INF, -INF, -INF, -INF],
                                           [-INF, -1.0, 0.0, 1.0, 2.0], [-INF, -INF, -INF, -INF, -3e38]]), [3, 0, 4, 1]))
    c.append(RankCase("competitors_inf", _f32([_spread(65, 0.5, 7, 1, hi=INF, lo=-INF),
                                               _spread(65, -2.0, 64, 2, hi=INF), _spread(65, 3e38, 3, 3, hi=INF, lo=-INF, equal=5),
                                               _spread(65, 0.0, 0, 4, lo=-INF)]), [7, 64, 3, 0]))
    # signed zeros and denormals: no flush to zero in the compare
    c.append(RankCase("zeros", _f32([[0.0] + [-0.0] * 63, [-0.0] + [0.0] * 63, [0.0, -0.0, 0.0, 1.0] + [-1.0] * 60]),
                      [0, 0, 1]))
    c.append(RankCase("denormals", _f32([[0.0] + [DEN] * 100, [DEN] + [0.0] * 100, [-DEN] + [-0.0] * 100,
                                         [DEN] + [2e-40] * 50 + [0.5e-40] * 50, [-0.0] + [-DEN] * 99 + [1.4e-45]]),
                      [100, 0, 100, 50, 1]))
    # the HR@10 edge: ranks 8 .. 11 and the last place, 101 candidates
    c.append(RankCase("ranks_9_10", _f32([_spread(101, 0.25, g, 10 + g, equal=3) for g in (8, 9, 10, 11, 100 - 3)]),
                      [8, 9, 10, 11, 97]))
    # NaN: the target (ranks last), the competitors (not counted), the whole row
    for n in (2, 63, 64, 65, 101, 129):
        c.append(RankCase(f"nan_target_n{n}", _f32([[NAN] + [float(j) for j in range(n - 1)]]), [n - 1]))
    c.append(RankCase("nan_competitors", _f32([_spread(101, 1.0, 4, 21, nan=30), _spread(101, 1.0, 0, 22, nan=100),
                                               _spread(101, -INF, 0, 23, nan=50, lo=-INF), _spread(101, INF, 0, 24, nan=9)]),
                      [4, 0, 0, 0]))
    c.append(RankCase("nan_all_n101", _f32([[NAN] * 101, _spread(101, 0.0, 9, 25), [NAN] + [-INF] * 100]), [100, 9, 100]))
    # every count 0 .. 100 and back, 300 rows of 101 (75 workgroups), every third row with ties of the target
    c.append(RankCase("B300_n101", _f32([_spread(101, float(r % 7) - 3.0, r % 101 if r % 3 else min(r % 101, 95), 100 + r,
                                                  equal=0 if r % 3 else 5) for r in range(300)]),
                      [r % 101 if r % 3 else min(r % 101, 95) for r in range(300)]))
    for n in (63, 64, 65, 129):
        c.append(RankCase(f"B5_n{n}", _f32([_spread(n, 0.0, g, n + g) for g in (0, 1, n // 2, n - 2, n - 1)]),
                          [0, 1, n // 2, n - 2, n - 1]))
    for case in c:
        assert case.logits.ndim == 2 and len(case.ranks) == case.logits.shape[0], case.name
        case.logits.setflags(write=False)
    return tuple(c)


# ------------------------------------------------------------------------------------------------------------------------
# srfrd_topk_merge
# ------------------------------------------------------------------------------------------------------------------------
def merge_ref(idx, val, k):
    """idx int64 / val float32 (B, n_cand) -> (ids (B, k) int64, pos (B, k) int64): per row the pairs with idx >= 0 sorted by
    (value descending, id ascending), +0 and -0 equal, the first k; behind them id -1 and position -1 (the value there is
    -inf).  pos names the input slot a result came from, so its value is compared by bits."""
    idx, val = np.asarray(idx), np.asarray(val)
    B, n = idx.shape
    ids = np.full((B, k), -1, np.int64)
    pos = np.full((B, k), -1, np.int64)
    for b in range(B):
        live = [j for j in range(n) if idx[b, j] >= 0]
        assert not any(val[b, j] != val[b, j] for j in live), "merge_ref is not defined for NaN"
        live.sort(key=lambda j: (-float(val[b, j]), int(idx[b, j])))
        for r, j in enumerate(live[:k]):
            ids[b, r], pos[b, r] = idx[b, j], j
    return ids, pos


MergeCase = namedtuple("MergeCase", "name idx val k")
MERGE_N = (1, 63, 64, 65, 160, 1536, 1537, 4096)        # 1536 / 1537: the two sides of the 48 KiB dynamic-LDS opt-in
MERGE_B = (1, 4, 5)
MERGE_K = (1, 10, 64)
ID_MAX = 2 ** 31 - 2


def _merge_row(rng, n, k, sort):
    """sort: "regular" (ties, +-inf, a tenth of the slots empty and holding +inf), "empty", "few" (k - 1 live slots, at most
    n), "zero" (a +0 / -0 pair above everything else)"""
    step = ID_MAX // n
    ids = rng.permutation(n).astype(np.int64) * step
    ids[np.argmax(ids)] = ID_MAX
    val = np.round(rng.randn(n), 1).astype(np.float32)
    if sort == "empty":
        ids[:] = -1
        val[::2] = np.inf
    elif sort == "few":
        dead = rng.permutation(n)[min(n, k - 1):]
        ids[dead] = -1
        val[dead] = np.inf
    elif sort == "zero":
        val = (-np.abs(val) - np.float32(0.1)).astype(np.float32)
        if n >= 2:
            a, b = rng.permutation(n)[:2]
            val[a], val[b] = np.float32(0.0), np.float32(-0.0)
    else:
        spots = rng.permutation(n)
        val[spots[:max(1, n // 16)]] = np.inf
        val[spots[n // 16 + 1:n // 16 + 1 + n // 16]] = -np.inf
        dead = spots[-(n // 10):] if n >= 10 else spots[:0]
        ids[dead] = -1
        val[dead] = np.inf                                       # (an empty slot's value is never read as a score)
    return ids, val


@functools.lru_cache(maxsize=None)
def merge_cases():
    """the product of MERGE_N, MERGE_B, MERGE_K: 72 cases.  B = 1: a regular row, or the zero row at k = 10; B = 4: regular,
    empty, few, zero; B = 5: one more regular row, in a second workgroup"""
    out = []
    for n, B, k in itertools.product(MERGE_N, MERGE_B, MERGE_K):
        rng = np.random.RandomState(n * 1000 + B * 100 + k)
        sorts = (["zero" if k == 10 else "regular"] if B == 1 else ["regular", "empty", "few", "zero", "regular"][:B])
        rows = [_merge_row(rng, n, k, s) for s in sorts]
        idx, val = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        idx.setflags(write=False)
        val.setflags(write=False)
        out.append(MergeCase(f"n{n}_B{B}_k{k}", idx, val, k))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------------
# srfrd_check_ids
# ------------------------------------------------------------------------------------------------------------------------
# planes 0..2: item_a, item_b, item_c; 3..5: fake_a, fake_b, fake_c.  bad: ((plane, position, value), ...); others: "null"
# (the planes without a bad value are NULL) or "clean" (all six are passed); preset: the word before the call.
CheckCase = namedtuple("CheckCase", "name n n_items fake_hi bad others preset expected")
CHECK_N = (1, 63, 64, 65, 257, 131072, 131073, 262149)  # the grid-stride loop starts above 512 x 256 = 131 072
CHECK_FAKE_HI = 2


def item_bad_values(n_items):
    return (-1, n_items + 1, 2 ** 32, 2 ** 32 + n_items, 2 ** 63 - 1, -2 ** 63)


FAKE_BAD_VALUES = (-1, 3, 2 ** 32 + 1)


def check_positions(n):
    return sorted({0, n - 1} | ({131072} if n > 131072 else set()))


def _check_name(n, n_items, bad, others, preset):
    return f"n{n}_I{n_items}_{others}_w{preset}_" + "_".join(f"p{p}at{q}v{v}" for p, q, v in bad)


def _single(n, n_items, plane, pos, value, others, preset=0):
    bad = ((plane, pos, value),)
    return CheckCase(_check_name(n, n_items, bad, others, preset), n, n_items, CHECK_FAKE_HI, bad, others, preset,
                     preset | (1 if plane < 3 else 2))


@functools.lru_cache(maxsize=None)
def check_cases():
    """a seeded sample of {n} x {position} x {plane} x {bad value} x {n_items} x {others NULL / clean}, every large n with a
    bad id in its last element and at index 131 072, plus the cases without a single bad value: about 150 launches"""
    product = []
    for n in CHECK_N:
        for pos, plane, others in itertools.product(check_positions(n), range(6), ("null", "clean")):
            if plane < 3:
                product += [_single(n, I, plane, pos, v, others) for I in (1, 60) for v in item_bad_values(I)]
            else:
                product += [_single(n, 60, plane, pos, v, others) for v in FAKE_BAD_VALUES]
    rng = np.random.RandomState(4)
    picked = {product[i].name: product[i] for i in rng.choice(len(product), 100, replace=False)}
    for n in (131072, 131073, 262149):                               # every large n, every plane: last element and index 131 072
        for pos, plane in itertools.product(check_positions(n)[1:], range(6)):
            value = (item_bad_values(60) if plane < 3 else FAKE_BAD_VALUES)[(plane + pos) % 3]
            case = _single(n, 60, plane, pos, value, ("null", "clean")[(plane + pos) % 2])
            picked.setdefault(case.name, case)
    out = list(picked.values())
    for n in (1, 65, 131073):
        last = n - 1
        # one plane of each sort bad -> 3; a word that is already set keeps its bits; a clean call leaves the word alone
        both = ((1, last, 61), (4, 0, 3))
        out.append(CheckCase(_check_name(n, 60, both, "clean", 0), n, 60, CHECK_FAKE_HI, both, "clean", 0, 3))
        out.append(_single(n, 60, 2, last, 2 ** 32, "null", preset=4))
        out.append(_single(n, 60, 5, last, -1, "clean", preset=4))
        for preset in (0, 4, 7):
            out.append(CheckCase(_check_name(n, 60, (), "clean", preset), n, 60, CHECK_FAKE_HI, (), "clean", preset, preset))
        # the boundary values 0, n_items and fake_hi do not flag (as bad-value triples that are in fact valid)
        edge = ((0, 0, 0), (1, last, 60), (2, last, 0), (3, 0, 0), (4, last, 2), (5, 0, 2))
        out.append(CheckCase(_check_name(n, 60, edge, "clean", 0) + "_valid", n, 60, CHECK_FAKE_HI, edge, "clean", 0, 0))
        edge1 = ((0, last, 1),)
        out.append(CheckCase(_check_name(n, 1, edge1, "null", 0) + "_valid", n, 1, CHECK_FAKE_HI, edge1, "null", 0, 0))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def check_planes(n, seed=0):
    """six clean int64 planes of n ids: item ids in [0, 1] (valid for every n_items used), fake ids in [0, 2]"""
    rng = np.random.RandomState(seed + n % 1000)
    return [rng.randint(0, 2 if p < 3 else 3, n).astype(np.int64) for p in range(6)]


# ------------------------------------------------------------------------------------------------------------------------
# srfrd_user_labels
# ------------------------------------------------------------------------------------------------------------------------
LABEL_LS = (1, 63, 64, 65, 200)


def _decile_rows(L):
    """fake/real windows whose fake ratio sits exactly on a decile boundary (n1 / tot = k / 10), plus their neighbours:
    the cases where a division lowered to x * rcp(y) lands one ulp under the integer and the floor drops by one."""
    import torch
    rows = []
    for tot in range(1, L + 1):
        for n1 in range(0, tot + 1):
            if (10 * n1) % tot == 0 or (10 * n1 + 10) % tot == 0:
                rows.append([0] * (L - tot) + [1] * n1 + [2] * (tot - n1))
    return torch.tensor(rows, dtype=torch.int64)
