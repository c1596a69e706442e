"""Helpers of tests/test_token_trainer_abi.py (CPU) and tests/test_gpu_token_reduce.py / test_gpu_token_trainer.py (gpu): the
shapes srfrd_table_reduce_mixed is run at, an fp64 numpy reference of it, and an index audit that restates the kernel's
addressing for one call and asserts every index in range.  Nothing here touches a GPU."""
import numpy as np

SEG = 256                      # SRFRD_TNEG_SPLIT_ROWS
U24 = 2.0 ** -24


def ws_floats(n, d_item):
    """2 ceil(n / SEG) d_item rounded up to 64: srfrd_table_reduce_mixed_workspace_floats"""
    return (((n + SEG - 1) // SEG) * 2 * d_item + 63) // 64 * 64


class Case:
    """one call: a list of n entries, the first n_rows of them full rows, the rest rank-1 rows of rows_per_token per token"""

    def __init__(self, name, n, n_rows, hist, d_item=50, extra=0, rpt=2):
        self.name, self.n, self.n_rows, self.hist = name, n, n_rows, hist
        self.d_item, self.d_out, self.rpt = d_item, d_item + extra, rpt
        self.T = -(-(n - n_rows) // rpt)                       # hidden rows
        assert 0 <= n_rows <= n

    def __repr__(self):
        return self.name

    def keys(self):
        """-> (unsorted int64 keys (n,), n_items)"""
        n, nr = self.n, self.n_rows
        rs = np.random.RandomState(n * 7 + nr)
        if self.hist == "one":                                  # one item: a run through every segment
            return np.full(n, 3, np.int64), 5
        if self.hist == "zero":                                 # all pad: nothing is written
            return np.zeros(n, np.int64), 5
        if self.hist == "catalog8":                             # 8 items and the pad key
            return rs.randint(0, 9, n).astype(np.int64), 8
        if self.hist == "distinct":
            return (rs.permutation(n) + 1).astype(np.int64), n
        if self.hist == "boundary":                             # item 1's run is sorted positions [0, 256): ends on the cut
            assert n > SEG
            k = np.concatenate([np.ones(SEG, np.int64), 2 + rs.randint(0, 3, n - SEG)])
            return k[rs.permutation(n)], 4
        if self.hist == "straddle":
            # item 1 fills sorted positions [0, 256 - a), item 5's a full rows end the first segment and its b rank-1 rows
            # start the second; item 9 takes the rest
            a, b = min(3, nr), 5
            assert nr >= 1 and n - nr >= b + (SEG - a) and n > SEG + b
            k = np.full(n, 9, np.int64)
            k[:a] = 5                                           # full rows of item 5
            k[nr:nr + b] = 5                                    # rank-1 rows of item 5
            k[nr + b:nr + b + SEG - a] = 1                      # item 1: rank-1 rows only
            return k, 9
        raise KeyError(self.hist)

    def inputs(self):
        """-> dict of the call's fp32 / int64 host arrays"""
        keys, n_items = self.keys()
        rs = np.random.RandomState(self.n + 13 * self.d_item)
        nc = self.n - self.n_rows
        return dict(keys=keys, n_items=n_items,
                    rows=rs.randn(self.n_rows, self.d_item).astype(np.float32),
                    coef=rs.randn(nc).astype(np.float32),
                    hidden=rs.randn(max(self.T, 1), self.d_out).astype(np.float32))


def _cases():
    out = []
    widths = [(1, 0), (50, 0), (64, 0), (1, 5), (50, 5), (64, 5)]       # d_item, d_out - d_item
    rpts = [1, 2, 17]
    hists = ["catalog8", "distinct", "one", "zero"]
    i = 0
    # every (n, n_rows) pair that fits, the widths, rows_per_token and the key histograms cycling through them
    for n in (1, 255, 256, 257, 769, 2100):
        for n_rows in (0, 1, 37, 300):
            for only_full in (False, True):
                nn = n_rows if only_full else n
                if n_rows > nn or nn < 1 or (only_full and n_rows == 0):
                    continue
                if only_full and n != 2100:                     # (n == n_rows: one case per n_rows, not one per n)
                    continue
                d, x = widths[i % 6]
                out.append(Case(f"n{nn}_r{n_rows}_d{d}+{x}_t{rpts[i % 3]}_{hists[i % 4]}", nn, n_rows, hists[i % 4], d, x, rpts[i % 3]))
                i += 1
    # every histogram at every width, on a list of more than three segments with both kinds of rows
    for d, x in widths:
        for h in hists + ["boundary", "straddle"]:
            out.append(Case(f"n769_r37_d{d}+{x}_t2_{h}", 769, 37, h, d, x, 2))
    for rpt in rpts:                                            # the special cuts at every rows_per_token, and with n_rows = 300 > SEG
        out.append(Case(f"n2100_r300_d50+5_t{rpt}_straddle", 2100, 300, "straddle", 50, 5, rpt))
        out.append(Case(f"n2100_r300_d50+0_t{rpt}_boundary", 2100, 300, "boundary", 50, 0, rpt))
        out.append(Case(f"n2100_r0_d64+5_t{rpt}_one", 2100, 0, "one", 64, 5, rpt))
    out.append(Case("n2100_r2100_d50+0_t1_one", 2100, 2100, "one", 50, 0, 1))          # full rows only, a run of nine segments
    seen = set()
    return [c for c in out if not (c.name in seen or seen.add(c.name))]


REDUCE_CASES = _cases()


def terms_of(keys, rows, coef, hidden, rpt, d_item):
    """(n, d_item) fp64: the row every list entry stands for, from the fp32 inputs"""
    n_rows, nc = rows.shape[0], coef.shape[0]
    tok = np.arange(nc) // rpt
    r1 = coef.astype(np.float64)[:, None] * hidden.astype(np.float64)[tok, :d_item] if nc else np.zeros((0, d_item))
    return np.concatenate([rows.astype(np.float64).reshape(n_rows, d_item), r1], 0)


def mixed_reduce_ref(keys, rows, coef, hidden, rpt, d_item, n_items):
    """fp64 reference: per item the sum of its entries in list order (a stable sort of the keys), keys <= 0 skipped ->
    (G (n_items + 1, d_item), m (n_items + 1,) the number of terms of a row, S (n_items + 1, d_item) = sum |term|)"""
    terms = terms_of(keys, rows, coef, hidden, rpt, d_item)
    order = np.argsort(keys, kind="stable")
    G = np.zeros((n_items + 1, d_item))
    S = np.zeros((n_items + 1, d_item))
    m = np.zeros(n_items + 1, np.int64)
    for e in order:                                             # (sorted order: an item's entries in list order)
        k = keys[e]
        if k > 0:
            G[k] += terms[e]
            S[k] += np.abs(terms[e])
            m[k] += 1
    return G, m, S


def audit_indices(keys, n_rows, rpt, T, n_items, d_item, ws):
    """Restates rank1_segment_kernel<mixed> / rank1_merge_kernel's addressing for one call - sorted position -> list entry ->
    full row or (coefficient, token); key -> table row; segment -> partial slots - and asserts every index in range.
    ``T``: rows of `hidden`; ``ws``: floats of the workspace.  -> (segments, partial slots a run-crossing segment uses)"""
    n = keys.shape[0]
    assert 0 < n < 2 ** 31 and 0 <= n_rows <= n and rpt >= 1
    order = np.argsort(keys, kind="stable")
    skeys = keys[order]
    assert np.all((order >= 0) & (order < n)), "order[i] < n"
    full = order < n_rows
    r = order[~full] - n_rows
    assert np.all((r >= 0) & (r < n - n_rows)), "coefficient index"
    assert np.all(r // rpt < T), "tok < T"
    assert np.all(order[full] < n_rows), "full row index"
    assert np.all(np.abs(order) < 2 ** 31), "the lane's source fits an int"
    assert np.all((skeys >= 0) & (skeys <= n_items)), "0 <= key <= n_items"
    segs = (n + SEG - 1) // SEG
    slots = ws // d_item
    used = 0
    for w in range(segs):
        s0, s1 = w * SEG, min(w * SEG + SEG, n)
        assert s1 - 1 < n                                        # (the entry an idle lane takes its source from)
        if skeys[s1 - 1] <= 0:
            continue
        cont = s0 > 0 and skeys[s0 - 1] == skeys[s0]
        goes_on = s1 < n and skeys[s1] == skeys[s1 - 1]
        for on, slot in ((cont, 2 * w), (goes_on, 2 * w + 1)):
            if on:
                assert slot < slots, "partial slot < ws_floats / d_item"
                used += 1
        if goes_on:                                              # the merge walks the segments the run passes through
            v = w + 1
            while True:
                assert 2 * v < slots
                e = (v + 1) * SEG
                if e >= n or skeys[e] != skeys[s1 - 1]:
                    break
                v += 1
    return segs, used


def step_keys(input_ids, targets, negatives, n_items, remove_hits):
    """the key list of FusedTrainer's token-negatives step: [clamped input ids (T) | per position (target, K negatives)],
    as srfrd_tneg_bwd writes the second part: 0 at ignored positions and for slots that take no part"""
    B, L, K = negatives.shape
    y = np.clip(targets.reshape(-1), 0, n_items)
    ng = np.clip(negatives.reshape(B * L, K), 0, n_items).copy()
    if remove_hits:
        ng[ng == y[:, None]] = 0
    ng[y == 0] = 0
    head = np.concatenate([y[:, None], ng], 1).reshape(-1)
    return np.concatenate([np.clip(input_ids.reshape(-1), 0, n_items), head]).astype(np.int64)


# (B, L, K, n_items) of every FusedTrainer(loss="token_softmax" | "gbce") that tests/test_gpu_token_trainer.py builds
TRAINER_SHAPES = [(16, 20, 1, 300), (16, 20, 5, 300), (16, 20, 65, 300), (16, 50, 1, 300), (16, 50, 5, 300), (16, 50, 65, 300),
                  (8, 20, 24, 300), (8, 20, 1, 300), (8, 20, 7, 300), (16, 20, 65, 8), (512, 50, 64, 50_000), (16, 50, 3, 400)]
