"""What the full-catalog ranking tests share (tests/test_gpu_rank_widths.py, test_gpu_rank_shapes.py, test_rank_width_cover.py,
and the predict check of test_gpu_rank_exclude.py): the fp64 host reference of the scores, the value bound derived from it, the
stable order and the target rank as include/srfrd_hip.h defines them, the comparison of a kernel's list with that reference,
and the generators of the inputs.  Plain torch / numpy on the CPU; only Runner touches the GPU.

Value bound.  For one set of operands E32 = max over (b, i) of |s32 - s64| / A, where s32 is a plain fp32 matmul of the same
operands on the CPU, s64 the fp64 one and A(b, i) = sum_k |h_k| |e_k| (+ the side term's absolute sum): the error of an
ordinary fp32 evaluation, not of the kernels.  A kernel value passes when |val - s64| <= 4 max(E32, 2^-23) A.  The factor 4: the
six-product path accumulates six times the terms in another order and rounding error grows like the square root of the term
count (sqrt 6 = 2.45); the rest is room for a maximum over a finite sample.  The floor 2^-23 A covers widths 1..3, where a
plain dot product is exact but the split sum and the side-term add still round."""
import numpy as np
import torch

from tests.loss_refs import FAKE_CASES, head_model, head_table

# ------------------------------------------------------------------------------------------------ what the tests run
WIDTHS = list(range(1, 65))
# both sides of every seam of rank_plan and the stream kernels: the 4-wide k-padding of the fp32 stream, the 8-wide lane
# groups and the 32-deep k-steps of the bf16 stream, the fp32 table's route change at 52 / 53, the bf16 shadow's at 51 / 53 / 64
REQUIRED_WIDTHS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 47, 48, 49, 50, 51, 52, 53, 54, 63, 64)
ROUTES = ("fp32", "fp32_forced", "bf16")          # fp32 table; fp32 table under SRFRD_TOPK_FP32=1; bf16 shadow
WIDTH_CASES = [(d, 0) for d in WIDTHS] + list(FAKE_CASES)        # (d_item, d_fake): d_fake > 0 is SRFRN
N_ITEMS, B_WIDTHS, L_HID = 2600, 17, 2            # rows 0..2600: eleven 256-row chunks, the last of 41 rows, above kCandMax
KS = (1, 10, 64)                                  # 64 > 11 chunks: tau = -inf and 2601 > 2048 candidates, the exhaustive path
RANGE_LO = (0, 1, 2, 3, 255, 256, 257)
SKIP_CAP = 0.10                                   # share of (user, slot) pairs / of targets a case may leave to near ties
TIE_IDS_A, TIE_IDS_B = (255, 256, 257), (511, 512, 513)
TIE_SINGLES = (1000, 1001, 1002)
TIE_EDGE = (700, 2000)                            # slots 10 / 11 at k = 10
SHAPE_WIDTHS = [(32, "fp32"), (50, "fp32"), (64, "fp32"), (50, "bf16"), (51, "bf16"), (64, "bf16")]
SHAPE_BATCHES = (1, 15, 16, 17, 33)
NU2_BATCHES = (257, 300)
EXHAUSTIVE_ROWS = (2049, 12_544)                   # k = 50: at most 49 chunks of 256 rows keep tau at -inf
K50_THRESHOLD_ROWS = 16_384                       # 64 chunks: the same k on the threshold path
K_CAND_MAX = 2048


def ranges():
    return [(lo, hi) for lo in RANGE_LO for hi in (lo + 1, lo + 17, N_ITEMS + 1)]


# ------------------------------------------------------------------------------------------------ scores
def _last(hidden, d):
    return hidden[:, -1, :d]


def scores64(hidden, table, side=None):
    """(B, rows) fp64 numpy: hidden[:, -1, :d_item] @ table.T (+ <hidden[:, -1, d_item:], fake_embed[user_label]> for SRFRN,
    side = (fake_embed, user_label))"""
    d = table.shape[1]
    s = _last(hidden, d).double() @ table.double().T
    if side is not None:
        fe, lab = side
        s = s + (hidden[:, -1, d:].double() * fe.double()[lab]).sum(1, keepdim=True)
    return s.numpy()


def scores32(hidden, table, side=None):
    """the same in plain fp32 on the CPU: what an ordinary evaluation errs by"""
    d = table.shape[1]
    s = _last(hidden, d).float() @ table.float().T
    if side is not None:
        fe, lab = side
        s = s + (hidden[:, -1, d:].float() * fe.float()[lab]).sum(1, keepdim=True)
    return s.double().numpy()


def absdot(hidden, table, side=None):
    """A(b, i) = sum_k |h_k| |e_k| (+ the side term's absolute sum), fp64 numpy"""
    d = table.shape[1]
    a = _last(hidden, d).double().abs() @ table.double().abs().T
    if side is not None:
        fe, lab = side
        a = a + (hidden[:, -1, d:].double().abs() * fe.double().abs()[lab]).sum(1, keepdim=True)
    return a.numpy()


def e32_of(hidden, table, side=None):
    s64, s32, A = scores64(hidden, table, side), scores32(hidden, table, side), absdot(hidden, table, side)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(A > 0, np.abs(s32 - s64) / A, 0.0)
    return float(r.max())


def eps_of(e32):
    """the relative bound of a case: a value passes when |val - s64| <= eps_of(E32) A"""
    return 4.0 * max(e32, 2.0 ** -23)


class Ref:
    """the fp64 reference of one set of operands"""

    def __init__(self, hidden, table, side=None):
        self.s = scores64(hidden, table, side)
        self.A = absdot(hidden, table, side)
        self.e32 = e32_of(hidden, table, side)
        self.unit = max(self.e32, 2.0 ** -23)
        self.eps = eps_of(self.e32)


# ------------------------------------------------------------------------------------------------ order and rank
def masked(scores, lo, hi, exclude_pad, excl_rows=None):
    m = np.full_like(scores, -np.inf)
    m[:, lo:hi] = scores[:, lo:hi]
    if exclude_pad and lo == 0:
        m[:, 0] = -np.inf
    if excl_rows is not None:
        for b, r in enumerate(excl_rows):
            r = np.asarray(r, dtype=np.int64).reshape(-1)
            r = r[(r >= 0) & (r < m.shape[1])]
            m[b, r] = -np.inf
    return m


def topk_ref(scores, k, lo, hi, exclude_pad, excl_rows=None):
    """-> (idx int64 (B, k), val fp64 (B, k)): value descending, id ascending; idx -1 / val -inf where fewer than k remain"""
    m = masked(scores, lo, hi, exclude_pad, excl_rows)
    B, n = m.shape
    idx, val = np.full((B, k), -1, np.int64), np.full((B, k), -np.inf)
    ids = np.arange(n)
    for b in range(B):
        order = np.lexsort((ids, -m[b]))[:k]
        order = order[m[b, order] > -np.inf]
        idx[b, :order.size], val[b, :order.size] = order, m[b, order]
    return idx, val


def rank_ref(scores, targets, lo, hi, exclude_pad, excl_rows=None):
    """rank[b] = #{i in [lo, hi) : i != t_b, i not in excl[b], !(exclude_pad && i == 0), s(b, i) > s(b, t_b)}; targets are
    clamped into the table like every id"""
    m = masked(scores, lo, hi, exclude_pad, excl_rows)
    out = np.zeros(m.shape[0], np.int64)
    for b, t in enumerate(np.clip(np.asarray(targets), 0, m.shape[1] - 1)):
        row = m[b].copy()
        row[t] = -np.inf
        out[b] = int((row > scores[b, t]).sum())
    return out


def check_topk(idx, val, ref, k, lo, hi, exclude_pad, excl_rows=None, tag=""):
    """A kernel's list (numpy idx (B, k), val (B, k)) against the reference.  Asserts: as many filled slots as rankable items
    and -1 / -inf behind them; every id rankable and returned once; every value within eps A of s64 at ITS id; the list's own
    order law (value descending, equal values by ascending id); the reference's order at every adjacent pair whose fp64 gap
    exceeds twice the bound, and the same id set inside every run of closer pairs (a run cut by slot k may take any of the
    run's ids); a run of one fp64 score (bit-identical rows) is no near tie: its ids come in ascending order.
    -> (skipped pairs, filled slots, largest |val - s64| / (max(E32, 2^-23) A))"""
    m = masked(ref.s, lo, hi, exclude_pad, excl_rows)
    B, n = m.shape
    ids = np.arange(n)
    skipped, pairs, worst = 0, 0, 0.0
    for b in range(B):
        order = np.lexsort((ids, -m[b]))
        n_ok = int((m[b] > -np.inf).sum())
        kk = min(k, n_ok)
        pairs += kk                                   # (filled slots only: empty trailing slots do not dilute the cap)
        where = (tag, "user", b, "range", lo, hi, "k", k)
        assert (idx[b, kk:] == -1).all() and np.isneginf(val[b, kk:]).all(), where
        gi, gv = idx[b, :kk], val[b, :kk].astype(np.float64)
        assert ((gi >= 0) & (gi < n)).all(), (where, gi)
        assert (m[b, gi] > -np.inf).all(), (where, "an id outside the rankable set", gi[~(m[b, gi] > -np.inf)])
        assert np.unique(gi).size == kk, (where, "an id twice")
        assert np.isfinite(gv).all(), where
        err, a = np.abs(gv - ref.s[b, gi]), ref.A[b, gi]
        assert (err <= ref.eps * a).all(), (where, "value", float((err / np.maximum(ref.unit * a, 1e-300)).max()), "x unit, allowed 4")
        if kk:
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.where(a > 0, err / (ref.unit * a), 0.0).max()))
        down = gv[:-1] > gv[1:]
        assert (down | ((gv[:-1] == gv[1:]) & (gi[:-1] < gi[1:]))).all(), (where, "own order", gi, gv)
        rs, rt = m[b, order[:n_ok]], ref.eps * ref.A[b, order[:n_ok]]
        cut = (rs[:-1] - rs[1:]) > 2.0 * np.maximum(rt[:-1], rt[1:])          # cut[j]: between reference slots j and j + 1
        j = 0
        while j < kk:
            e = j
            while e < n_ok - 1 and not cut[e]:
                e += 1
            if rs[j] == rs[e]:            # one score, bit for bit in fp64 (identical rows): an exact tie goes by ascending id
                assert (gi[j:min(e + 1, kk)] == order[j:min(e + 1, kk)]).all(), (where, "exact tie", j, e, gi[j:e + 1], order[j:e + 1])
            else:
                if e < kk:
                    assert set(gi[j:e + 1].tolist()) == set(order[j:e + 1].tolist()), (where, "slots", j, e, gi[j:e + 1], order[j:e + 1])
                    skipped += e - j
                else:
                    assert set(gi[j:kk].tolist()) <= set(order[j:e + 1].tolist()), (where, "slots", j, kk, gi[j:kk], order[j:e + 1])
                    skipped += kk - j
                # bit-identical rows inside a run of near ties still go by ascending id among themselves
                got = gi[j:min(e + 1, kk)]
                for v in np.unique(m[b, got]):
                    same = got[m[b, got] == v]
                    assert (same[:-1] < same[1:]).all(), (where, "exact tie inside a near-tie run", same)
            j = e + 1
    return skipped, pairs, worst


def check_same_lists(idx_a, val_a, idx_b, val_b, ref, tag=""):
    """Two lists of one ranking problem that may come from different arithmetics (each already held to the reference by
    check_topk): where a slot holds the same id the two values are within twice the bound of each other (each is within the
    bound of s64); where the ids differ, the two items' fp64 scores are closer than twice the bound (a near tie either
    arithmetic may order).  -> (slots with different ids, values differing in bits)"""
    swaps = bits = 0
    for b in range(idx_a.shape[0]):
        for j in range(idx_a.shape[1]):
            ia, ib = int(idx_a[b, j]), int(idx_b[b, j])
            if ia < 0 or ib < 0:
                assert ia == ib, (tag, b, j, ia, ib)
                continue
            tol = 2.0 * ref.eps * max(ref.A[b, ia], ref.A[b, ib])
            if ia == ib:
                assert abs(float(val_a[b, j]) - float(val_b[b, j])) <= tol, (tag, b, j, val_a[b, j], val_b[b, j])
                bits += int(val_a[b, j] != val_b[b, j])
            else:
                assert abs(ref.s[b, ia] - ref.s[b, ib]) <= tol, (tag, b, j, ia, ib)
                swaps += 1
    return swaps, bits


def check_rank(rank, ref, targets, lo, hi, exclude_pad, excl_rows=None, dups=(), tag=""):
    """A kernel's target ranks against the definition: exact for every target whose score is farther than the bound from every
    other rankable score; otherwise between the counts with the margin taken either way.  `dups`: ids holding bit-identical
    copies of every user's target row - they tie exactly and are never counted.  -> number of targets with a near score"""
    m = masked(ref.s, lo, hi, exclude_pad, excl_rows)
    near = 0
    for b, t in enumerate(np.clip(np.asarray(targets), 0, m.shape[1] - 1)):
        row = m[b].copy()
        row[t] = -np.inf
        if len(dups):
            row[list(dups)] = -np.inf
        st, margin = ref.s[b, t], ref.eps * (ref.A[b] + ref.A[b, t])
        row[row == st] = -np.inf          # the target's fp64 score bit for bit: an identical row, an exact tie, never counted
        fin = row > -np.inf
        lo_cnt, hi_cnt = int((fin & (row > st + margin)).sum()), int((fin & (row > st - margin)).sum())
        assert lo_cnt <= int(rank[b]) <= hi_cnt, (tag, "user", b, "target", int(t), "rank", int(rank[b]), "allowed", lo_cnt, hi_cnt)
        near += lo_cnt != hi_cnt
    return near


# ------------------------------------------------------------------------------------------------ inputs
class Case:
    """operands of one ranking problem on the CPU: table (rows, d_item), hidden (B, L, d_item + d_fake) whose last position is
    ranked (the earlier ones hold 1e3: a kernel reading the wrong position shows), SRFRN's fake_embed (3, d_fake) and labels"""

    def __init__(self, table, hidden, fake_embed=None, labels=None):
        self.table, self.hidden, self.fake_embed, self.labels = table, hidden, fake_embed, labels
        self.d_item = table.shape[1]
        self.d_fake = hidden.shape[2] - self.d_item
        self.n_items, self.B = table.shape[0] - 1, hidden.shape[0]

    def side(self):
        return None if self.fake_embed is None else (self.fake_embed, self.labels)

    def ref(self, table=None):
        """the reference over `table` (default: the fp32 table; a bf16 shadow passes its own values)"""
        return Ref(self.hidden, self.table if table is None else table, self.side())

    def clone(self):
        c = lambda t: None if t is None else t.clone()
        return Case(c(self.table), c(self.hidden), c(self.fake_embed), c(self.labels))


def bf16_round(t):
    """round-to-nearest-even bf16 values of an fp32 tensor, as fp32 (the host's stand-in for the shadow the device builds;
    the GPU tests read the shadow itself back)"""
    return t.to(torch.bfloat16).float()


def base_case(d_item, d_fake=0, seed=0, n_items=N_ITEMS, B=B_WIDTHS, positive=False):
    """standard normals with full 24-bit significands (the second and third bf16 planes of both operands matter); positive:
    the hidden state is |N| + 0.5 in every channel, so one table row can outrank the catalog for every user at once"""
    g = torch.Generator().manual_seed(7919 * d_item + 104_729 * d_fake + seed)
    table = torch.randn(n_items + 1, d_item, generator=g)
    hidden = torch.full((B, L_HID, d_item + d_fake), 1e3)
    last = torch.randn(B, d_item + d_fake, generator=g)
    hidden[:, -1] = last.abs() + 0.5 if positive else last
    fe = lab = None
    if d_fake:
        fe = torch.randn(3, d_fake, generator=g)
        lab = torch.randint(0, 3, (B,), generator=g)
        lab[:3] = torch.tensor([0, 1, 2])
    return Case(table, hidden, fe, lab)


LEAK_RANGES = ((0, 300), (N_ITEMS + 1 - 300, N_ITEMS + 1))


def leak_case(d_item, d_fake=0, seed=0):
    """every product of a score is <= -1 (hidden 1 + |N|, table -(1 + |N|), the side term likewise), item 0 is the zero row a
    padding row is, and the best rows of each 300-item range of LEAK_RANGES sit at the end of its first 256-row chunk: a
    zero-padded row, a stale row behind the tail's last one, item 0 or a padding column scores above every real item"""
    c = base_case(d_item, d_fake, seed + 1)
    c.table = -(1.0 + c.table.abs())
    c.table[0] = 0.0
    c.hidden[:, -1] = 1.0 + c.hidden[:, -1].abs()
    if d_fake:
        c.fake_embed = -(1.0 + c.fake_embed.abs())
    for lo, _ in LEAK_RANGES:
        for j in range(40):
            c.table[lo + 255 - j] = -(1.0 + 1e-3 * j)
    return c


def check_leak_case(c):
    s = scores64(c.hidden, c.table, c.side())
    item = _last(c.hidden, c.d_item).double().numpy() @ c.table.double().numpy().T
    assert (item[:, 1:] <= -1.0).all() and (item[:, 0] == 0.0).all()      # a zero row outranks every real item by at least 1
    if c.fake_embed is not None:
        assert float(c.fake_embed.max()) <= -1.0 and float(c.hidden[:, -1, c.d_item:].min()) >= 1.0
    for lo, hi in LEAK_RANGES:
        best = np.argmax(s[:, max(lo, 1):hi], axis=1) + max(lo, 1)
        assert (best == lo + 255).all()                       # the planted maximum leads, in the last row before the tail chunk


def tie_case(d_item, d_fake=0, seed=0):
    """positive hidden states and planted rows that lead every user's list: bit-identical rows across the 256-row seam (ids
    255 / 256 / 257, value 30 in every channel), across the 512-row seam (511 / 512 / 513, 25), three single rows (24, 23, 22)
    and a bit-identical pair (20) that slot 10 / 11 of a k = 10 list cuts"""
    c = base_case(d_item, d_fake, seed + 2, positive=True)
    for ids, v in ((TIE_IDS_A, 30.0), (TIE_IDS_B, 25.0), (TIE_SINGLES[:1], 24.0), (TIE_SINGLES[1:2], 23.0),
                   (TIE_SINGLES[2:], 22.0), (TIE_EDGE, 20.0)):
        c.table[list(ids)] = v
    return c


TIE_ORDER = list(TIE_IDS_A) + list(TIE_IDS_B) + list(TIE_SINGLES) + list(TIE_EDGE)


def check_tie_case(c, table=None):
    t = c.table if table is None else table
    for ids in (TIE_IDS_A, TIE_IDS_B, TIE_EDGE):
        assert all(torch.equal(t[ids[0]].view(torch.int32), t[i].view(torch.int32)) for i in ids[1:])
    idx, _ = topk_ref(scores64(c.hidden, t, c.side()), 11, 0, c.n_items + 1, True)
    assert (idx == np.array(TIE_ORDER)).all()


MAGNITUDES = ("x1e4", "x1e-4", "last_channel", "first_channel", "zero_row", "own_row")
ZERO_ROW, OWN_ROW0 = 1234, 300


def magnitude_case(d_item, d_fake, kind, seed=0):
    c = base_case(d_item, d_fake, seed + 3)
    if kind in ("x1e4", "x1e-4"):                 # (SRFRN: the side embedding with the table, or one term would drown the other)
        c.table *= float(kind[1:])
        if d_fake:
            c.fake_embed *= float(kind[1:])
    elif kind == "last_channel":
        c.table[:, d_item - 1] *= 1e3
    elif kind == "first_channel":
        c.table[:, 0] *= 1e3
    elif kind == "zero_row":
        c.table[ZERO_ROW] = 0.0
    elif kind == "own_row":
        for b in range(c.B):
            c.table[OWN_ROW0 + b] = c.hidden[b, -1, :d_item]
    else:
        raise ValueError(kind)
    return c


def exclusion_rows(ref, lo, hi, n_items, seed):
    """per user: its current top 3 of the range, id 0, duplicates, ids outside the range and outside the catalog, noise"""
    top, _ = topk_ref(ref.s, 3, lo, hi, True)
    g = np.random.RandomState(seed)
    rows = []
    for b in range(ref.s.shape[0]):
        r = [int(i) for i in top[b] if i >= 0] + [0, -5, n_items + 7, 10 * n_items, max(lo - 1, 0), hi]
        r += r[:3] + g.randint(1, n_items + 1, 20).tolist()
        rows.append(np.array(r, np.int64)[g.permutation(len(r))])
    rows[-1] = np.zeros(0, np.int64)                       # one user without a set
    return rows


def skip_share(ref, k, lo, hi, exclude_pad, excl_rows=None):
    """share of (user, slot) pairs the reference alone leaves to near ties: check_topk of the reference's own list"""
    idx, val = topk_ref(ref.s, k, lo, hi, exclude_pad, excl_rows)
    skipped, pairs, _ = check_topk(idx, val, ref, k, lo, hi, exclude_pad, excl_rows)
    return skipped / max(pairs, 1)


def rank_targets(ref, seed):
    """targets whose rank the reference alone decides (no other score of the catalog within the two bounds of the target's):
    per user a slot of its top 10, every third user an id drawn anywhere, and the first and the last id for the first users
    that see them clear"""
    n, B = ref.s.shape[1], ref.s.shape[0]
    top, _ = topk_ref(ref.s, 10, 0, n, True)
    g = np.random.RandomState(seed)

    def clear(b, t):
        d = np.abs(ref.s[b] - ref.s[b, t])
        d[t] = np.inf
        return bool((d > ref.eps * (ref.A[b] + ref.A[b, t])).all())

    t = top[:, 3].copy()
    for b in range(B):
        draws = (g.randint(1, n) for _ in range(100)) if b % 3 == 0 else iter(top[b, 3:])
        t[b] = next((int(c) for c in draws if clear(b, int(c))), t[b])
    for edge in (1, n - 1):
        b = next((b for b in range(1, B) if b % 3 and t[b] not in (1, n - 1) and clear(b, edge)), None)
        if b is not None:
            t[b] = edge
    return t


# ------------------------------------------------------------------------------------------------ cases of the shape file
ONE_CHUNK_ITEMS = 17
SHARD_CASES = [(50, "fp32"), (64, "fp32"), (50, "bf16")]
SHARD_COUNTS = (3, 8)
WPB1 = (8, 5, 4097 * 256)                         # (d_item, B, n_items): 4097 chunks of 256 rows


def tail_case(d, B):
    return base_case(d, 0, B, B=B)


def one_chunk_case(d):
    return base_case(d, 0, 0, n_items=ONE_CHUNK_ITEMS)


def k50_case(d, rows):
    return base_case(d, 0, rows, n_items=rows - 1)


def nu2_case(d, n_items, B):
    return base_case(d, 0, B, n_items=n_items, B=B)


def chunk512_case(n_items):
    c = base_case(50, 0, 5, n_items=n_items, positive=True)
    for ids, v in ((TIE_IDS_A, 30.0), (TIE_IDS_B, 25.0)):
        c.table[list(ids)] = v
    return c


def shard_cuts(n_shards):
    from srfrd_amd.ranker import row_shards
    return [hi for _, hi in row_shards(N_ITEMS + 1, n_shards)][:-1]


def sharded_case(d, n_shards):
    """a bit-identical pair across every shard boundary, leading every user's list"""
    c = base_case(d, 0, n_shards, positive=True)
    for j, cut in enumerate(shard_cuts(n_shards)):
        c.table[[cut - 1, cut]] = 40.0 - j
    return c


# ------------------------------------------------------------------------------------------------ the plan, asked on the host
def plan_layout(d_item, d_fake, n_items, bf16):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SRFRN", n_items, L_HID, d_item, d_fake) if d_fake else _lib.make_layout("SASRec", n_items, L_HID, d_item)
    lay.table_bf16 = int(bf16)
    return lay


def plan(d_item, d_fake, n_items, route, op, B, k, lo, hi, excl, n_cu=256):
    from srfrd_amd import _lib
    return _lib.rank_plan(plan_layout(d_item, d_fake, n_items, route == "bf16"), op, B, k, lo, hi, excl,
                          _lib.SW_TOPK_FP32 if route == "fp32_forced" else 0, n_cu)


def plan_chunk_rows(p, n_rows):
    """item rows per chunk of a top-k plan, from the dynamic LDS of topk_tau_kernel (wpb rows of stream_chunks floats)"""
    tau = next(l for l in p if l[0] == "srfrd::topk_tau_kernel")
    chunks = tau[3] // (4 * (tau[2] // 64))
    return 256 if chunks == -(-n_rows // 256) else 512 if chunks == -(-n_rows // 512) else None


def plan_wpb(p):
    return next(l for l in p if l[0] == "srfrd::topk_tau_kernel")[2] // 64


def first_n_items(d_item, route, op, B, k, n_cu, want, limit=1 << 21):
    """the smallest catalog (in steps of 256 rows, one row into a new chunk) whose plan satisfies want(plan, rows)"""
    for chunks in range(1, limit // 256):
        rows = 256 * chunks + 1
        p = plan(d_item, 0, rows - 1, route, op, B, k, 0, rows, False, n_cu)
        if not isinstance(p, int) and want(p, rows):
            return rows - 1
    raise AssertionError("no catalog size reaches the wanted plan")


def is_nu2(p, rows=None):
    return p[1 if p[0][0].startswith("srfrd::target_score") else 0][0].split("<")[1].startswith("2,")


def is_chunk512(p, rows):
    return plan_chunk_rows(p, rows) == 512


def width_calls():
    """(d_item, d_fake, n_items, route, op, B, k, lo, hi, excl) of every ranking call shape tests/test_gpu_rank_widths.py makes"""
    from srfrd_amd import _lib
    out = []
    for d, f in WIDTH_CASES:
        for route in ROUTES:
            for excl in (False, True):
                for k in KS:
                    out.append((d, f, N_ITEMS, route, _lib.RANK_TOPK, B_WIDTHS, k, 0, N_ITEMS + 1, excl))
                out.append((d, f, N_ITEMS, route, _lib.RANK_TARGET, B_WIDTHS, 1, 0, N_ITEMS + 1, excl))
    return out


def shape_calls(n_cu=256):
    """the same for tests/test_gpu_rank_shapes.py, with the catalog sizes it asks the plan for at `n_cu` CUs"""
    from srfrd_amd import _lib
    out = []
    for d, route in SHAPE_WIDTHS:
        for B in SHAPE_BATCHES:
            for excl in (False, True):
                out.append((d, 0, N_ITEMS, route, _lib.RANK_TOPK, B, 10, 0, N_ITEMS + 1, excl))
                out.append((d, 0, N_ITEMS, route, _lib.RANK_TARGET, B, 1, 0, N_ITEMS + 1, excl))
        out.append((d, 0, ONE_CHUNK_ITEMS, route, _lib.RANK_TOPK, B_WIDTHS, 64, 0, ONE_CHUNK_ITEMS + 1, False))
        for rows in EXHAUSTIVE_ROWS + (K50_THRESHOLD_ROWS,):
            out.append((d, 0, rows - 1, route, _lib.RANK_TOPK, B_WIDTHS, 50, 0, rows, False))
        if is_stream16(d, route):
            for B in NU2_BATCHES:
                n = first_n_items(d, route, _lib.RANK_TOPK, B, 10, n_cu, is_nu2)
                out.append((d, 0, n, route, _lib.RANK_TOPK, B, 10, 0, n + 1, False))
                out.append((d, 0, n, route, _lib.RANK_TARGET, B, 1, 0, n + 1, False))
    n = first_n_items(50, "bf16", _lib.RANK_TOPK, B_WIDTHS, 10, n_cu, is_chunk512)
    out.append((50, 0, n, "bf16", _lib.RANK_TOPK, B_WIDTHS, 10, 0, n + 1, False))
    return out


def is_stream16(d_item, route):
    """rank_plan's route by width, restated: the bf16 matrix-core stream, or the fp32 stream"""
    if route == "fp32_forced":
        return False
    if route == "bf16":
        return d_item <= 64 and (d_item % 2 == 0 or d_item <= 51)
    return d_item <= 52


# ------------------------------------------------------------------------------------------------ the GPU side
class Runner:
    """a model holding a Case's operands on the GPU, and the four ranking ops called on the Case's hidden state directly: the
    logits are the test's own, no encoder runs"""

    def __init__(self, case, route):
        self.case, self.route = case, route
        self.m = head_model(case.d_item, case.d_fake, case.n_items, L_HID, table=case.table.cuda())
        self.m._ensure_flat()
        if route == "bf16":
            self.m.use_bf16_table()
        self.load(case)

    def load(self, case):
        """new operands of the same shape"""
        from srfrd_amd import ops
        self.case = case
        with torch.no_grad():
            head_table(self.m).copy_(case.table.cuda())
            if case.d_fake:
                self.m.embedding_layer.fake_embed.weight.copy_(case.fake_embed.cuda())
        self.m.refresh_bf16_table()
        self.hidden = case.hidden.cuda().contiguous()
        self.ulab = case.labels.cuda() if case.d_fake else None
        self.key = ops.register_model(self.m)
        return self

    def table_seen(self):
        """the table the kernels read, on the CPU as fp32: the parameter, or the uint16 shadow's own values widened"""
        if self.route != "bf16":
            return head_table(self.m).detach().cpu().clone()
        bits = self.m._table16.cpu().to(torch.int32) & 0xFFFF
        return (bits << 16).view(torch.float32).reshape(self.case.n_items + 1, self.case.d_item)

    def ref(self):
        return self.case.ref(self.table_seen())

    def _excl(self, rows):
        from srfrd_amd import ops
        return ops.excl_csr([torch.as_tensor(r, dtype=torch.int64) for r in rows], None, self.case.B, self.hidden.device)

    def topk(self, k, lo, hi, exclude_pad=True, excl_rows=None):
        if excl_rows is None:
            idx, val = torch.ops.srfrd.logits_topk(self.hidden, self.ulab, self.key, lo, hi, k, bool(exclude_pad))
        else:
            idx, val = torch.ops.srfrd.logits_topk_excl(self.hidden, self.ulab, self.key, lo, hi, k, bool(exclude_pad),
                                                        *self._excl(excl_rows))
        return idx.cpu().numpy(), val.cpu().numpy()

    def rank(self, targets, lo, hi, exclude_pad=True, excl_rows=None):
        x = (None, None, 0) if excl_rows is None else self._excl(excl_rows)
        t = torch.as_tensor(np.asarray(targets), dtype=torch.int64).cuda()
        return torch.ops.srfrd.target_rank(self.hidden, self.ulab, t, self.key, lo, hi, bool(exclude_pad), *x).cpu().numpy()

    def predict(self, cand):
        return torch.ops.srfrd.predict_logits(self.hidden, cand.cuda().contiguous(), self.ulab, self.key).cpu().numpy()


def check_predict(got, ref, cand, tag=""):
    """predict_logits (B, n_cand) against s64 at the clamped ids, under the value bound -> largest error in units"""
    B = ref.s.shape[0]
    c = np.clip(cand.numpy(), 0, ref.s.shape[1] - 1)
    c = np.broadcast_to(c, (B, c.shape[-1]))
    want, a = np.take_along_axis(ref.s, c, 1), np.take_along_axis(ref.A, c, 1)
    err = np.abs(got.astype(np.float64) - want)
    assert got.shape == want.shape and (err <= ref.eps * a).all(), (tag, "predict", float((err / np.maximum(ref.unit * a, 1e-300)).max()))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(a > 0, err / (ref.unit * a), 0.0).max())


def set_route(monkeypatch, route):
    """the environment of a table route: SRFRD_TOPK_FP32=1 forces the fp32 stream"""
    if route == "fp32_forced":
        monkeypatch.setenv("SRFRD_TOPK_FP32", "1")
    else:
        monkeypatch.delenv("SRFRD_TOPK_FP32", raising=False)


class Tally:
    """the checks of one case, with its skipped pairs, near targets and largest value ratio; close() prints them and holds the cap"""

    def __init__(self, tag):
        self.tag, self.skipped, self.pairs, self.worst, self.near, self.targets = tag, 0, 0, 0.0, 0, 0

    def add(self, idx, val, ref, k, lo, hi, exclude_pad=True, excl_rows=None, what=""):
        s, p, w = check_topk(idx, val, ref, k, lo, hi, exclude_pad, excl_rows, tag=(self.tag, what))
        self.skipped, self.pairs, self.worst = self.skipped + s, self.pairs + p, max(self.worst, w)

    def topk(self, run, ref, k, lo, hi, exclude_pad=True, excl_rows=None, what=""):
        idx, val = run.topk(k, lo, hi, exclude_pad, excl_rows)
        self.add(idx, val, ref, k, lo, hi, exclude_pad, excl_rows, what)
        return idx, val

    def rank(self, run, ref, t, lo, hi, exclude_pad=True, excl_rows=None, dups=(), what=""):
        got = run.rank(t, lo, hi, exclude_pad, excl_rows)
        assert got.dtype == np.int32 and got.shape == (len(t),)
        self.near += check_rank(got, ref, t, lo, hi, exclude_pad, excl_rows, dups, tag=(self.tag, what))
        self.targets += len(t)
        return got

    def close(self):
        print(f"RANK_MARGIN {self.tag} ratio {self.worst:.3f} skipped {self.skipped}/{self.pairs} near {self.near}/{self.targets}")
        assert self.skipped <= SKIP_CAP * max(self.pairs, 1), (self.tag, self.skipped, self.pairs)
        assert self.near <= SKIP_CAP * max(self.targets, 1), (self.tag, self.near, self.targets)
