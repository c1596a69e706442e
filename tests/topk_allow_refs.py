"""What the item-filter tests share (tests/test_topk_allow_abi.py, test_topk_allow_refs.py, test_gpu_topk_allow.py): the shapes the
GPU file runs, the filters, a numpy restatement of the packing, the filtered plan asked on the host, and a Runner that calls
srfrd::logits_topk_allow / srfrd::target_rank_allow.  The fp64 reference, the value bound, the order law and the input
generators are tests/rank_refs.py's, unchanged: a filter folds into its ``excl_rows`` argument (``union_rows``)."""
import numpy as np
import torch

from tests import rank_refs as R

N_ITEMS, B = R.N_ITEMS, R.B_WIDTHS                # 2601 rows (no maxima: at most the capacity), 17 users
SWEEP_KS = (1, 10, 100, 1024)
SWEEP_CASES = [(d, 0) for d in R.REQUIRED_WIDTHS] + list(R.FAKE_CASES)
BIG_ITEMS = 20_000                                # 20 001 rows, just over the capacity: 79 chunks of 256 rows, the threshold path
BIG_KS = (10, 100, 1024)
BLOCK = (700, 18_700)                             # a contiguous allowed block of 18 000 ids: more than the capacity
SMALL_BLOCK = (9_000, 9_300)                      # 300 ids, fewer than k = 1024
FILTERS = ("random_0.5", "random_0.05", "block", "block300", "all", "none")
EDGES = (31, 32, 33, 63, 64)                      # a filter's edge on each side of a 32-bit word boundary
RANGE_WIDTHS = [(50, "fp32"), (64, "fp32"), (50, "bf16")]
PACK_ROWS = (1, 31, 32, 33, 2601, 20_001)
PLAN_KS = (1, 64, 65, 256, 257, 512, 1024)
FINE, ALL = 0, 2                                  # SRFRD_WIDE_FINE / SRFRD_WIDE_ALL
CAPACITY = 16_384
FALLBACK_CASES = [(8, "fp32"), (50, "bf16"), (60, "fp32")]
MODEL_CASE = (3000, 9, 100)


# ---- filters ----------------------------------------------------------------------------------------------------------------------
def filter_mask(kind, n_items, seed=0):
    """bool (n_items + 1,) numpy"""
    n = n_items + 1
    g = np.random.RandomState(1000 + seed)
    if kind.startswith("random_"):
        return g.random_sample(n) < float(kind.split("_")[1])
    m = np.zeros(n, bool)
    if kind == "block":
        m[BLOCK[0]:BLOCK[1]] = True
    elif kind == "block300":
        m[SMALL_BLOCK[0]:SMALL_BLOCK[1]] = True
    elif kind == "all":
        m[:] = True
    elif kind != "none":
        raise ValueError(kind)
    return m


def edge_mask(edge, n_items, seed=0):
    """nothing below `edge`, the four ids from it on allowed, density 0.5 behind them"""
    m = filter_mask("random_0.5", n_items, seed + edge)
    m[:edge] = False
    m[edge:edge + 4] = True
    return m


def group_masks(n_items, seed=0):
    """three rows: density 0.5, density 0.1, a block"""
    m = np.stack([filter_mask("random_0.5", n_items, seed), filter_mask("random_0.1", n_items, seed + 1), np.zeros(n_items + 1, bool)])
    m[2, n_items // 4: n_items // 2] = True
    return m


def words_of(n_rows):
    return 0 if n_rows <= 0 else (n_rows + 31) // 32 + 1


def pack_ref(mask):
    """the packing restated in numpy: (G, n_rows) bool -> (G, W) uint32, bit i & 31 of word i >> 5, zero last word and tail"""
    mask = np.atleast_2d(np.asarray(mask)) != 0
    G, n = mask.shape
    W = words_of(n)
    bits = np.zeros((G, W * 32), np.uint64)
    bits[:, :n] = mask
    w = (bits.reshape(G, W, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return w.astype(np.uint32)


def union_rows(mask, group, excl_rows=None):
    """the reference's ``excl_rows`` of a filtered call: per user the ids its group's row disallows, united with its exclusion row"""
    mask = np.atleast_2d(mask)
    off = [np.nonzero(~mask[g])[0].astype(np.int64) for g in range(mask.shape[0])]
    out = []
    for b, g in enumerate(group):
        out.append(off[g] if excl_rows is None else np.concatenate([off[g], np.asarray(excl_rows[b], np.int64).reshape(-1)]))
    return out


# ---- the plan, asked on the host ----------------------------------------------------------------------------------------------
def switches(route):
    from srfrd_amd import _lib
    return _lib.SW_TOPK_FP32 if route == "fp32_forced" else 0


def plan(d_item, d_fake, n_items, route, B, k, lo, hi, excl, n_cu=256):
    from srfrd_amd import _lib
    return _lib.topk_allow_plan(R.plan_layout(d_item, d_fake, n_items, route == "bf16"), B, k, lo, hi, excl, switches(route), n_cu)


def rows_per_group(p, n_rows):
    """rows of the largest group of a plan (0: no groups): the 256-row chunks of the range over the groups per user"""
    _, (path, cap, groups) = p
    if path == ALL:
        return 0
    chunks = -(-n_rows // 256)
    assert groups % chunks == 0, (groups, chunks)
    return 256 // (groups // chunks)


def check_plan(p, path=None, excl=None):
    """the kernels a path launches, in order -> the plan's (path, capacity, groups)"""
    assert not isinstance(p, int), p
    launches, (got, cap, groups) = p
    names = [n.split("<")[0].replace("srfrd::", "") for n, *_ in launches]
    if excl is not None:
        assert (names[0] == "excl_prep_kernel") == excl, names
    if names[0] == "excl_prep_kernel":
        names = names[1:]
    assert got in (FINE, ALL), got
    if got == FINE:
        assert names[0] in ("allow_max16_kernel", "allow_max_kernel"), names
        names = names[1:]
    assert names[0] == "wide_tau_kernel" and names[1] in ("allow_collect16_kernel", "allow_collect_kernel"), names
    assert names[2:] == ["wide_select_kernel", "allow_fallback_kernel"], names
    assert path is None or got == path, (got, "wanted", path)
    return got, cap, groups


def allow_calls():
    """(d_item, d_fake, n_items, route, B, k, lo, hi, excl) of every top-k call shape tests/test_gpu_topk_allow.py makes"""
    out = []
    for d, f in SWEEP_CASES:
        for route in R.ROUTES:
            for k in SWEEP_KS:
                out.append((d, f, N_ITEMS, route, B, k, 0, N_ITEMS + 1, False))
    for d, route in R.SHAPE_WIDTHS:
        for k in BIG_KS:
            out.append((d, 0, BIG_ITEMS, route, B, k, 0, BIG_ITEMS + 1, False))
    for d, route in RANGE_WIDTHS:
        for lo, hi in R.ranges():
            out.append((d, 0, N_ITEMS, route, B, 100, lo, hi, False))
        for n in (N_ITEMS, BIG_ITEMS):
            for excl in (False, True):
                out.append((d, 0, n, route, B, 100, 0, n + 1, excl))
        out.append((d, 0, N_ITEMS, route, B, 1024, 300, 1300, False))
    for d, f in R.FAKE_CASES:
        for route in ("fp32", "bf16"):
            for n in (N_ITEMS, BIG_ITEMS):
                out.append((d, f, n, route, B, 100, 0, n + 1, True))
    for d, route in FALLBACK_CASES:
        for k in (100, 1024):
            for b in (3, 2):
                out.append((d, 0, BIG_ITEMS, route, b, k, 0, BIG_ITEMS + 1, False))
    n, b, k = MODEL_CASE
    out.append((50, 0, n, "fp32", b, k, 0, n + 1, True))
    return out


# ---- the GPU side ---------------------------------------------------------------------------------------------------------------
class Filter:
    """a mask (G, n_items + 1) packed on the GPU by srfrd_amd.ItemFilter, with its numpy rows"""

    def __init__(self, mask, n_items):
        import srfrd_amd
        self.mask, self.n_items = np.atleast_2d(np.asarray(mask, bool)), n_items
        self.f = srfrd_amd.ItemFilter(torch.from_numpy(self.mask), n_items, "cuda")

    def row(self, g):
        """the single-group filter of row g"""
        return Filter(self.mask[g], self.n_items)


class Runner(R.Runner):
    """rank_refs.Runner whose topk / rank are the filtered ops; wide() is the unfiltered wide op on the same operands"""

    def group_dev(self, group):
        return None if group is None else torch.as_tensor(np.asarray(group), dtype=torch.int64).cuda()

    def topk_dev(self, filt, k, lo, hi, exclude_pad=True, excl_rows=None, group=None, hidden=None):
        x = (None, None, 0) if excl_rows is None else self._excl(excl_rows)
        return torch.ops.srfrd.logits_topk_allow(self.hidden if hidden is None else hidden, self.ulab, self.key, lo, hi, k,
                                                 bool(exclude_pad), *x, filt.f.words, self.group_dev(group))

    def topk(self, filt, k, lo, hi, exclude_pad=True, excl_rows=None, group=None):
        idx, val = self.topk_dev(filt, k, lo, hi, exclude_pad, excl_rows, group)
        return idx.cpu().numpy(), val.cpu().numpy()

    def rank(self, filt, targets, lo, hi, exclude_pad=True, excl_rows=None, group=None):
        x = (None, None, 0) if excl_rows is None else self._excl(excl_rows)
        t = torch.as_tensor(np.asarray(targets), dtype=torch.int64).cuda()
        return torch.ops.srfrd.target_rank_allow(self.hidden, self.ulab, t, self.key, lo, hi, bool(exclude_pad), *x, filt.f.words,
                                                 self.group_dev(group)).cpu().numpy()

    def wide(self, k, lo, hi, exclude_pad=True, excl_rows=None):
        x = (None, None, 0) if excl_rows is None else self._excl(excl_rows)
        idx, val = torch.ops.srfrd.logits_topk_wide(self.hidden, self.ulab, self.key, lo, hi, k, bool(exclude_pad), *x)
        return idx.cpu().numpy(), val.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def first_allowed(whole, mask_rows, k):
    """the first k entries of each user's whole ranking (idx, val) whose id its mask row allows, -1 / -inf behind them"""
    idx, val = whole
    oi, ov = np.full((idx.shape[0], k), -1, np.int64), np.full((idx.shape[0], k), -np.inf, np.float32)
    for b in range(idx.shape[0]):
        keep = (idx[b] >= 0) & mask_rows[b][np.maximum(idx[b], 0)]
        n = min(k, int(keep.sum()))
        oi[b, :n], ov[b, :n] = idx[b][keep][:n], val[b][keep][:n]
    return oi, ov


def zero_user_case(d_item, n_items, B=3, user=1):
    c = R.base_case(d_item, 0, 12, n_items=n_items, B=B)
    c.hidden[user, -1] = 0.0
    return c


def without_user(case, user):
    keep = [b for b in range(case.B) if b != user]
    return R.Case(case.table, case.hidden[keep].clone(), case.fake_embed, None if case.labels is None else case.labels[keep])


def fallback_mask(n_items):
    """everything but every seventh id: 17 143 allowed ids of 20 001, more than the capacity"""
    m = np.ones(n_items + 1, bool)
    m[::7] = False
    return m
