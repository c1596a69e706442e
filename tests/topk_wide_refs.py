"""What the wide top-k tests share (tests/test_topk_wide_abi.py, test_topk_wide_refs.py, test_gpu_topk_wide.py): the shapes the
GPU file runs, the wide plan asked on the host for each of them, and a Runner that calls srfrd::logits_topk_wide.  The fp64
reference, the value bound, the order law and the input generators are tests/rank_refs.py's, unchanged: a wide list is held to
the bar the k <= 64 lists are held to."""
import numpy as np
import torch

from tests import rank_refs as R

N_ITEMS, B_WIDTHS = R.N_ITEMS, R.B_WIDTHS        # 2601 rows, 17 users
KS = (65, 100, 1024)                             # one past the narrow op's limit; a re-ranker's pull; the limit
CASES = [(d, 0) for d in R.REQUIRED_WIDTHS] + list(R.FAKE_CASES)
TAIL_BATCHES = (1, 15, 16, 17, 33, 257)
RANGE_WIDTHS = [(50, "fp32"), (64, "fp32"), (50, "bf16")]
FINE, CHUNK, ALL = 0, 1, 2                       # SRFRD_WIDE_*
PATH_NAMES = {FINE: "fine", CHUNK: "chunk", ALL: "all"}
# (d_item, route, B, k) of the chunk-maxima cases; the catalog size comes from the plan (first_rows)
CHUNK_CASES = [(50, "fp32", B_WIDTHS, 65), (8, "fp32", 3, 1024), (50, "bf16", 2, 1024)]
FALLBACK_CASES = [(8, "fp32"), (50, "bf16"), (60, "fp32")]     # (d_item, route) over capacity + 1 rows, B = 3 (and 2)
BESIDE_CASES = [(50, "fp32"), (50, "bf16"), (64, "fp32"), (50, "fp32_forced")]
MODEL_CASE = (3000, 9, 100)                      # (n_items, B, k) of the model.topk test (SASRec, hidden 50, exclude="input")
ONE_CHUNK_ITEMS = R.ONE_CHUNK_ITEMS              # 17 items: sixteen rankable ones under exclude_pad
ADMISSIBLE_WIDTHS = (1, 2, 3, 8, 50, 64)


def switches(route):
    from srfrd_amd import _lib
    return _lib.SW_TOPK_FP32 if route == "fp32_forced" else 0


def plan(d_item, d_fake, n_items, route, B, k, lo, hi, excl, n_cu=256):
    """-> ([(kernel, workgroups, threads, dynamic LDS)], (path, capacity, groups)) or a negative code"""
    from srfrd_amd import _lib
    return _lib.topk_wide_plan(R.plan_layout(d_item, d_fake, n_items, route == "bf16"), B, k, lo, hi, excl, switches(route), n_cu)


def capacity():
    return plan(8, 0, 100, "fp32", 1, 100, 0, 101, False)[1][1]


def first_rows(d_item, route, B, k, path, n_cu=256, limit=1 << 22):
    """the smallest item range (256 c + 1 rows: one row into a new chunk) whose plan takes `path`"""
    lo, hi = 1, limit // 256
    ok = lambda c: plan(d_item, 0, 256 * c, route, B, k, 0, 256 * c + 1, False, n_cu)[1][0] == path
    assert ok(hi), (d_item, route, B, k, path)
    while lo < hi:                                # (a path's catalogs are an interval: more rows, coarser groups)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid) else (mid + 1, hi)
    return 256 * lo + 1


def check_plan(p, path=None):
    """the kernels a path launches, in order -> the plan's (path, capacity, groups)"""
    assert not isinstance(p, int), p
    launches, (got, cap, groups) = p
    names = [n.split("<")[0].replace("srfrd::", "") for n, *_ in launches]
    if names[0] == "excl_prep_kernel":
        names = names[1:]
    first = {FINE: ("wide_max16_kernel", "wide_max_kernel"), CHUNK: ("topk_max16_kernel", "topk_max_kernel"), ALL: ()}[got]
    if first:
        assert names[0] in first, (names, got)
        names = names[1:]
    assert names[0] == "wide_tau_kernel" and names[1] in ("wide_collect16_kernel", "wide_collect_kernel"), names
    assert names[2:] == ["wide_select_kernel", "wide_fallback_kernel"], names
    assert path is None or got == path, (PATH_NAMES[got], "wanted", PATH_NAMES[path])
    return got, cap, groups


def wide_calls(n_cu=256):
    """(d_item, d_fake, n_items, route, B, k, lo, hi, excl) of every call shape tests/test_gpu_topk_wide.py makes"""
    out = []
    for d, f in CASES:
        for route in R.ROUTES:
            for k in KS:
                for excl in (False, True):
                    out.append((d, f, N_ITEMS, route, B_WIDTHS, k, 0, N_ITEMS + 1, excl))
            for lo, hi in R.LEAK_RANGES:
                out.append((d, f, N_ITEMS, route, B_WIDTHS, 100, lo, hi, False))
    for d, route, B, k in CHUNK_CASES:
        rows = first_rows(d, route, B, k, CHUNK, n_cu)
        out.append((d, 0, rows - 1, route, B, k, 0, rows, False))
    for d, route in RANGE_WIDTHS:
        for k in (100, 1024):
            out.append((d, 0, ONE_CHUNK_ITEMS, route, B_WIDTHS, k, 0, ONE_CHUNK_ITEMS + 1, False))
        for lo, hi in R.ranges():
            out.append((d, 0, N_ITEMS, route, B_WIDTHS, 100, lo, hi, False))
        out.append((d, 0, N_ITEMS, route, B_WIDTHS, 100, 257, 557, True))
        for B in TAIL_BATCHES:
            for excl in (False, True):
                out.append((d, 0, N_ITEMS, route, B, 100, 0, N_ITEMS + 1, excl))
    cap = capacity()
    for d, route in FALLBACK_CASES:                  # identical rows and the zero user (B = 3), and the batch without it (B = 2)
        for k in (100, 1024):
            for B, lo in ((3, 0), (3, 5), (2, 0)):
                out.append((d, 0, cap, route, B, k, lo, cap + 1, False))
    for d, route in BESIDE_CASES:
        for k in (64, 100):
            out.append((d, 0, N_ITEMS, route, B_WIDTHS, k, 0, N_ITEMS + 1, False))
    n, B, k = MODEL_CASE
    out.append((50, 0, n, "fp32", B, k, 0, n + 1, True))
    return out


class Runner(R.Runner):
    """rank_refs.Runner whose topk is the wide op; narrow() is the k <= 64 op on the same operands"""

    def topk(self, k, lo, hi, exclude_pad=True, excl_rows=None):
        idx, val = self.topk_dev(k, lo, hi, exclude_pad, excl_rows)
        return idx.cpu().numpy(), val.cpu().numpy()

    def topk_dev(self, k, lo, hi, exclude_pad=True, excl_rows=None, hidden=None):
        x = (None, None, 0) if excl_rows is None else self._excl(excl_rows)
        return torch.ops.srfrd.logits_topk_wide(self.hidden if hidden is None else hidden, self.ulab, self.key, lo, hi, k,
                                                bool(exclude_pad), *x)

    def narrow(self, k, lo, hi, exclude_pad=True, excl_rows=None):
        return R.Runner.topk(self, k, lo, hi, exclude_pad, excl_rows)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def identical_rows_case(d_item, rows, B=3):
    """every row of the table the same (item 0 included): every score of a user ties, the list is the first k rankable ids"""
    c = R.base_case(d_item, 0, 11, n_items=rows - 1, B=B)
    c.table[:] = c.table[1].clone()
    return c


def zero_user_case(d_item, rows, B=3, user=1):
    """an ordinary catalog and batch in which one user's last hidden state is all zeros: its scores are 0 everywhere"""
    c = R.base_case(d_item, 0, 12, n_items=rows - 1, B=B)
    c.hidden[user, -1] = 0.0
    return c


def without_user(case, user):
    keep = [b for b in range(case.B) if b != user]
    return R.Case(case.table, case.hidden[keep].clone(), case.fake_embed, None if case.labels is None else case.labels[keep])
