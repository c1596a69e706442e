"""-m gpu: the train step's tail (srfrd_amd/csrc/srfrd_optim.hip) through its C entry points, against plain float64
restatements written here.  Two kinds of input per kernel: small-integer-valued floats, whose fp32 sums are exact (a missed,
doubled or misplaced element fails by equality), and random normal data held to a bound derived from fp32 rounding (a few
units of 2^-24 per operation).  Every output buffer carries sentinel guard words on both sides, and every element outside
the range a call owns must come back bit-unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of fp32
G = 16                             # guard words on each side (a multiple of 4: the data stays 16-byte aligned)
SENT32, SENT16 = 0x5EADBEEF, 0x5EAD


def _L():
    from srfrd_amd import _lib
    return _lib.lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc, what):
    assert rc == 0, (what, rc)


class Buf:
    """a device copy of a 1-D array between sentinel guard words"""

    def __init__(self, a, dtype=torch.float32, n=None):
        a = np.ascontiguousarray(a).reshape(-1)
        self.n = a.size if n is None else n
        bits = torch.int16 if dtype == torch.int16 else (torch.int64 if dtype == torch.int64 else torch.int32)
        self.sent = SENT16 if bits == torch.int16 else SENT32
        self.full = torch.full((self.n + 2 * G,), self.sent, dtype=bits, device="cuda").view(dtype)
        if a.size:
            self.t.copy_(torch.from_numpy(a).to(dtype))

    @classmethod
    def sentinel(cls, n, dtype=torch.float32):
        """n elements, all of them sentinel words too"""
        return cls(np.zeros(0, dtype=np.float32), dtype, n)

    @property
    def t(self):
        return self.full[G:G + self.n]

    def p(self, bias=0):
        """device pointer to element 0 (minus `bias` elements: the sharded optimizer indexes its slices globally)"""
        return C.c_void_p(self.t.data_ptr() - bias * self.full.element_size())

    def get(self):
        """the data (numpy) after checking both guards"""
        f = self.full.cpu()
        b = f.view(torch.int16 if f.element_size() == 2 else (torch.int64 if f.element_size() == 8 else torch.int32))
        assert (b[:G] == self.sent).all() and (b[G + self.n:] == self.sent).all(), "a guard word was overwritten"
        return f[G:G + self.n].numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def _bf16_rne(x):
    """fp32 -> bf16 bits, round to nearest even (NaN inputs: any NaN out; callers test those on their own)"""
    b = _bits(np.ascontiguousarray(x, dtype=np.float32)).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _state(t0=4, base=12345, lr=1e-3, b1=0.9, b2=0.98):
    """an optimizer state after srfrd_step_begin from t0 (32 words, guarded); returns (Buf, fp32 step_size, fp32 bc2_sqrt)"""
    s = np.zeros(32, dtype=np.int32)
    s[0], s[1] = t0, base
    st = Buf(s, torch.int32)
    _ok(_L().srfrd_step_begin(st.p(), lr, b1, b2, _st()), "srfrd_step_begin")
    torch.cuda.synchronize()
    w = st.get()
    return st, float(w[4:5].view(np.float32)[0]), float(w[5:6].view(np.float32)[0])


# ---- srfrd_step_begin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.9, 0.98), (0.9, 0.999)])
@pytest.mark.parametrize("t0", [0, 1, 9, 999, 1 << 20])
def test_step_begin_advances_t_seed_and_bias_corrections(t0, betas):
    lr, (b1, b2), base = 3e-3, betas, 0x2468ACE
    s = np.arange(32, dtype=np.int32) * 7 + 1000          # words the advance must not touch keep these
    s[0], s[1] = t0, base
    st = Buf(s, torch.int32)
    _ok(_L().srfrd_step_begin(st.p(), lr, b1, b2, _st()), "srfrd_step_begin")
    torch.cuda.synchronize()
    w = st.get()
    t = t0 + 1
    assert int(w[0]) == t and int(w[1]) == base
    assert int(w[2:3].view(np.uint32)[0]) == O.step_seed(base, t)
    ss, bc2 = w[4:6].view(np.float32).astype(np.float64)
    want_ss, want_bc2 = lr / (1.0 - b1 ** t), np.sqrt(1.0 - b2 ** t)
    assert abs(ss - want_ss) <= np.spacing(np.float32(want_ss)), (ss, want_ss)
    assert abs(bc2 - want_bc2) <= np.spacing(np.float32(want_bc2)), (bc2, want_bc2)
    keep = [i for i in range(32) if i not in (0, 2, 4, 5)]
    assert (w[keep] == s[keep]).all()


# ---- srfrd_adam_step ----------------------------------------------------------------------------------------------------
def _adam_inputs(n, seed):
    r = np.random.default_rng(seed)
    p = r.standard_normal(n).astype(np.float32)
    g = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 4, n)).astype(np.float32)     # magnitudes up to 1e4
    if n > 2:                                        # zero gradients, away from the short vectors' scalar tails
        g[1] = 0.0
        g[r.random(n) < 0.1] = 0.0
        g[n - 4:] = np.where(g[n - 4:] == 0, 1.5, g[n - 4:])
    m = (r.standard_normal(n) * 0.1).astype(np.float32)
    v = (np.abs(r.standard_normal(n)) * 0.05).astype(np.float32)
    return p, g, m, v


def _adam_ref(p, g, m, v, b1, b2, eps, ss, bc2s, gscale):
    """fp64 Adam of fp32 inputs + elementwise error bounds of the fp32 kernel (2x the worst-case rounding sum)"""
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    b1, b2, eps = (float(np.float32(x)) for x in (b1, b2, eps))
    gs = g * gscale
    m1 = b1 * m + (1 - b1) * gs
    v1 = b2 * v + (1 - b2) * gs * gs
    den = np.sqrt(v1) / bc2s + eps
    upd = ss * m1 / den
    em = 4 * U * (b1 * np.abs(m) + (1 - b1) * np.abs(gs))
    ev = 8 * U * v1
    eu = ss / den * em + np.abs(upd) * 10 * U
    ep = U * (np.abs(p) + np.abs(upd)) + eu
    return p - upd, m1, v1, 2 * ep, 2 * em, 2 * ev


def _run_adam(p, g, m, v, i0, i1, n_zero, stats, n_table, state, b=(0.9, 0.98), eps=1e-8):
    """one srfrd_adam_step: param over the whole vector, grad / m / v over [i0, i1) only (pointers biased by -i0 as the
    sharded trainer passes them); returns the outputs as numpy (guards checked)"""
    n = p.size
    P, Gr, M, V = Buf(p), Buf(g[i0:i1]), Buf(m[i0:i1]), Buf(v[i0:i1])
    S = Buf(stats) if stats is not None else None
    H = Buf.sentinel(n_table, torch.int16) if n_table else None
    rc = _L().srfrd_adam_step(P.p(), Gr.p(i0), M.p(i0), V.p(i0), n, i0, i1, n_zero, b[0], b[1], eps, state.p(),
                              S.p() if S else None, H.p() if H else None, n_table, _st())
    _ok(rc, "srfrd_adam_step")
    torch.cuda.synchronize()
    return P.get(), Gr.get(), M.get(), V.get(), (H.get() if H else None)


def _check_adam(p, g, m, v, i0, i1, n_zero, stats, n_table, out, ss, bc2s, b=(0.9, 0.98), eps=1e-8):
    po, go, mo, vo, ho = out
    gscale = 1.0 / float(np.float32(stats[2])) if stats is not None else 1.0
    rp, rm, rv, ep, em, ev = _adam_ref(p[i0:i1], g[i0:i1], m[i0:i1], v[i0:i1], b[0], b[1], eps, ss, bc2s, gscale)
    assert (np.abs(po[i0:i1] - rp) <= ep).all(), float(np.max(np.abs(po[i0:i1] - rp) / ep))
    assert (np.abs(mo - rm) <= em).all(), float(np.max(np.abs(mo - rm) / em))
    assert (np.abs(vo - rv) <= ev).all(), float(np.max(np.abs(vo - rv) / ev))
    assert (_bits(po[:i0]) == _bits(p[:i0])).all() and (_bits(po[i1:]) == _bits(p[i1:])).all()
    idx = np.arange(i0, i1)
    assert (go[idx < n_zero] == 0).all()
    assert (_bits(go[idx >= n_zero]) == _bits(g[i0:i1][idx >= n_zero])).all()
    if ho is not None:
        hb = _bits(ho)
        lo, hi = min(i0, n_table), min(i1, n_table)
        assert (hb[lo:hi] == _bf16_rne(po[lo:hi])).all()
        assert (hb[:lo] == SENT16).all() and (hb[hi:] == SENT16).all()


def _slices(n):
    from srfrd_amd import shard_bounds
    out = [(0, n)]
    if n - 1 > 4:
        out.append((4, n - 1))
    if n >= 8:
        out.append((8, 8))
    if n >= 5:
        out.append((4, 5))
    for world in (2, 3):
        out += [shard_bounds(n, world, r) for r in range(world)]
    return out


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099, 4_200_007])
def test_adam_step_against_fp64(n):
    """slices, biased moment pointers, gscale, n_zero inside and outside a float4, the bf16 shadow boundary, the grid-stride
    loop (n > 4096 x 256 x 4)"""
    p, g, m, v = _adam_inputs(n, n)
    state, ss, bc2s = _state(t0=6)
    stats_v = np.array([3.5, 1.25, 37.0, 0.0], dtype=np.float32)
    cases = []
    for k, (i0, i1) in enumerate(_slices(n)):
        for stats in (None, stats_v):
            for n_zero in sorted({0, 3, 6, max(n - 2, 0), n}):
                cases.append((i0, i1, stats, n_zero, (None, 5, 4097)[(k + n_zero) % 3]))
    if n > 100_000:                                  # (the fp64 reference of 4.2 M elements: a sample of the cases)
        cases = [c for j, c in enumerate(cases) if j % 9 == 0] + [(0, n, stats_v, n, 4097)]
    for i0, i1, stats, n_zero, n_table in cases:
        out = _run_adam(p, g, m, v, i0, i1, n_zero, stats, n_table or 0, state)
        _check_adam(p, g, m, v, i0, i1, n_zero, stats, n_table, out, ss, bc2s)


@pytest.mark.parametrize("n", [5, 4099, 4_200_007])
@pytest.mark.parametrize("world", [2, 3])
def test_adam_step_world_slices_equal_the_whole_vector_step(n, world):
    from srfrd_amd import shard_bounds
    p, g, m, v = _adam_inputs(n, 7 * n + world)
    state, ss, bc2s = _state(t0=2)
    stats = np.array([1.0, 2.0, 129.0, 0.0], dtype=np.float32)
    whole = _run_adam(p, g, m, v, 0, n, n, stats, 0, state)
    _check_adam(p, g, m, v, 0, n, n, stats, None, whole, ss, bc2s)
    po, mo, vo = p.copy(), np.empty_like(m), np.empty_like(v)
    same = np.zeros(n, dtype=bool)                      # elements both runs step in the same loop form (float4 body / scalar tail)
    body_whole = np.arange(n) < (n // 4) * 4
    for r in range(world):
        i0, i1 = shard_bounds(n, world, r)
        out = _run_adam(p, g, m, v, i0, i1, n, stats, 0, state)
        po[i0:i1], mo[i0:i1], vo[i0:i1] = out[0][i0:i1], out[2], out[3]
        assert (out[1] == 0).all()
        body = np.arange(i0, i1) < i0 + ((i1 - i0) // 4) * 4
        same[i0:i1] = body == body_whole[i0:i1]
    rp, rm, rv, ep, em, ev = _adam_ref(p, g, m, v, 0.9, 0.98, 1e-8, ss, bc2s, 1.0 / 129.0)
    assert (np.abs(po - rp) <= ep).all() and (np.abs(mo - rm) <= em).all() and (np.abs(vo - rv) <= ev).all()
    assert same.sum() >= n - 3 * world
    for a, b in ((po, whole[0]), (mo, whole[2]), (vo, whole[3])):
        assert (_bits(a)[same] == _bits(b)[same]).all()


# ---- srfrd_adam_pack_step -----------------------------------------------------------------------------------------------
PACK_CASES = [("SASRec", 60, 20, 50, 0, 0, 1),         # SASRec D = 50, grid 10 (< 16 ticket shards)
              ("SRFR", 500, 20, 43, 5, 0, 3),          # 43 + 5 with last_conv
              ("SRFRN", 300, 20, 45, 5, 0, 8),         # 45 + 5, eight blocks
              ("SRFU_B", 30000, 20, 64, 0, 2, 1)]      # D = 64, 1.95 M floats: grid at the 768-workgroup cap


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"{c[0]}_{c[3]}+{c[4]}_b{c[6]}")
def test_adam_pack_step_equals_adam_step_and_fresh_pack(case):
    from srfrd_amd import _lib
    kind, I, L, d_item, d_fake, n_labels, n_blocks = case
    lay = _lib.make_layout(kind, I, L, d_item, d_fake, n_labels, n_blocks, 1)
    n_tab = (lay.n_table + 3) // 4 * 4
    n = (n_tab + lay.n_dense + 3) // 4 * 4
    grid = min(((n >> 2) + 1 + 511) // 512, 768)
    assert (grid < 16) == (kind == "SASRec") and (grid == 768) == (kind == "SRFU_B")
    lr, b1, b2, eps = 2e-3, 0.9, 0.98, 1e-8
    p, g, m, v = _adam_inputs(n, I)
    p[lay.n_table:n_tab] = 0.0
    P, M, V = Buf(p), Buf(m), Buf(v)
    stats = Buf(np.array([2.0, 3.0, 41.0, 0.0], dtype=np.float32))
    st0 = np.zeros(32, dtype=np.int32)
    st0[1] = 777
    state = Buf(st0, torch.int32)
    _ok(_L().srfrd_step_begin(state.p(), lr, b1, b2, _st()), "srfrd_step_begin")
    n_packed = _L().srfrd_packed_floats(C.byref(lay))
    packed = Buf(np.zeros(n_packed, dtype=np.float32))
    dense = lambda buf: C.c_void_p(buf.t.data_ptr() + 4 * n_tab)        # noqa: E731
    _ok(_L().srfrd_pack_weights(C.byref(lay), dense(P), packed.p(), None, 0.0, 0.0, 0.0, _st()), "srfrd_pack_weights")
    H = Buf.sentinel(lay.n_table, torch.int16)
    r = np.random.default_rng(5)
    for launch in range(3):
        g = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n)).astype(np.float32)
        Gr = Buf(g)
        # the same step by srfrd_adam_step on copies of the same inputs
        P2, G2, M2, V2 = Buf(P.get()), Buf(g), Buf(M.get()), Buf(V.get())
        H2 = Buf(H.get(), torch.int16)
        s_before = state.get()
        S2 = Buf(s_before, torch.int32)
        _ok(_L().srfrd_adam_step(P2.p(), G2.p(), M2.p(), V2.p(), n, 0, n, n_tab, b1, b2, eps, S2.p(), stats.p(), H2.p(),
                                 lay.n_table, _st()), "srfrd_adam_step")
        _ok(_L().srfrd_adam_pack_step(C.byref(lay), P.p(), Gr.p(), M.p(), V.p(), n, n_tab, n_tab, lr, b1, b2, eps, state.p(),
                                      stats.p(), packed.p(), H.p(), _st()), "srfrd_adam_pack_step")
        fresh = Buf(np.zeros(n_packed, dtype=np.float32))
        _ok(_L().srfrd_pack_weights(C.byref(lay), dense(P), fresh.p(), None, 0.0, 0.0, 0.0, _st()), "srfrd_pack_weights")
        adv = Buf(s_before, torch.int32)
        _ok(_L().srfrd_step_begin(adv.p(), lr, b1, b2, _st()), "srfrd_step_begin")
        torch.cuda.synchronize()
        for a, b in ((P, P2), (Gr, G2), (M, M2), (V, V2), (H, H2)):
            assert (_bits(a.get()) == _bits(b.get())).all(), launch
        assert (Gr.get()[:n_tab] == 0).all() and (_bits(Gr.get()[n_tab:]) == _bits(g[n_tab:])).all()
        assert (_bits(packed.get()) == _bits(fresh.get())).all(), launch
        s, want = state.get(), adv.get()
        assert s[6] == 0 and (s[8:24] == 0).all(), launch
        assert all(s[i] == want[i] for i in (0, 1, 2, 4, 5)), (launch, s[:6], want[:6])
        assert int(s[0]) == launch + 2


# ---- srfrd_reduce_dense / srfrd_loss_stats / srfrd_loss_finalize --------------------------------------------------------
def _c2_dense():
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 50_000, 50, 50, 0, 0, 2, 1)
    return lay.n_dense, _L().srfrd_bwd_grid(C.byref(lay), 512, 50)


def _reduce(slabs, n_dense):
    S, out = Buf(slabs), Buf.sentinel(n_dense)
    _ok(_L().srfrd_reduce_dense(S.p(), slabs.shape[0], n_dense, out.p(), None, 1, None, None, _st()), "srfrd_reduce_dense")
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize("n_dense", [1, 63, 64, 65, "C2"])
def test_reduce_dense_sums_every_slab_exactly_and_reproducibly(n_dense):
    c2_dense, c2_grid = _c2_dense()
    n_dense = c2_dense if n_dense == "C2" else n_dense
    r = np.random.default_rng(n_dense)
    for n_slabs in sorted({1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 100, 257, c2_grid}):
        ints = r.integers(-8, 9, (n_slabs, n_dense)).astype(np.float32)
        got = _reduce(ints, n_dense)
        assert (got == ints.astype(np.int64).sum(0)).all(), n_slabs
        x = r.standard_normal((n_slabs, n_dense)).astype(np.float32)
        a, b = _reduce(x, n_dense), _reduce(x, n_dense)
        assert (_bits(a) == _bits(b)).all(), n_slabs
        ref = x.astype(np.float64).sum(0)
        bound = (n_slabs + 4) * U * np.abs(x.astype(np.float64)).sum(0)
        assert (np.abs(a - ref) <= bound).all(), n_slabs


def _loss_part(B, r, ints):
    if ints:
        lp = np.stack([r.integers(0, 40, B), r.integers(0, 40, B), r.integers(0, 50, B)], 1).astype(np.float32)
    else:
        lp = np.stack([np.abs(r.standard_normal(B)) * 20, np.abs(r.standard_normal(B)) * 20, r.integers(0, 50, B)], 1)
    lp[0, 2] = max(lp[0, 2], 1.0)                        # at least one target
    return lp.astype(np.float32)


@pytest.mark.parametrize("B", [1, 255, 256, 257, 512])
def test_reduce_dense_loss_part_matches_loss_stats_and_finalize(B):
    r = np.random.default_rng(B)
    slabs = r.integers(-3, 4, (5, 65)).astype(np.float32)
    for ints in (True, False):
        lp = _loss_part(B, r, ints)
        LP, S1, O1 = Buf(lp), Buf.sentinel(4), Buf.sentinel(1)
        out, SL = Buf.sentinel(65), Buf(slabs)
        _ok(_L().srfrd_reduce_dense(SL.p(), 5, 65, out.p(), LP.p(), B, S1.p(), O1.p(), _st()), "srfrd_reduce_dense")
        S2, O2, O3 = Buf.sentinel(4), Buf.sentinel(1), Buf.sentinel(1)
        _ok(_L().srfrd_loss_stats(LP.p(), B, S2.p(), O2.p(), _st()), "srfrd_loss_stats")
        _ok(_L().srfrd_loss_finalize(S1.p(), O3.p(), _st()), "srfrd_loss_finalize")
        S4, O4 = Buf.sentinel(4), Buf.sentinel(1)                          # loss_out NULL: statistics only
        _ok(_L().srfrd_reduce_dense(SL.p(), 5, 65, out.p(), LP.p(), B, S4.p(), None, _st()), "srfrd_reduce_dense")
        torch.cuda.synchronize()
        s1, l1 = S1.get(), O1.get()
        assert (out.get() == slabs.astype(np.int64).sum(0)).all()
        sums = lp.astype(np.float64).sum(0)
        if ints:
            assert (s1 == np.array([sums[0], sums[1], sums[2], 0.0])).all(), (s1, sums)
        else:
            bound = (B / 256 + 12) * U * np.abs(lp.astype(np.float64)).sum(0)
            assert (np.abs(s1[:3] - sums) <= bound).all() and s1[3] == 0.0
        s64 = s1.astype(np.float64)
        want = s64[0] / s64[2] + s64[1] / s64[2]
        assert abs(float(l1[0]) - want) <= 4 * U * abs(want)
        assert (_bits(S2.get()) == _bits(s1)).all() and (_bits(S4.get()) == _bits(s1)).all()
        assert _bits(O2.get())[0] == _bits(l1)[0] and _bits(O3.get())[0] == _bits(l1)[0]
        assert _bits(O4.get())[0] == SENT32


# ---- srfrd_table_reduce -------------------------------------------------------------------------------------------------
def _table_keys(name, r, n_items):
    if name == "random":                                  # 3 x 8 x 20 + 1 rows: many repeats, pad ids, n % 4 != 0
        k = r.integers(0, n_items + 1, 481)
        k[r.random(481) < 0.3] = 0
        return k
    if name == "one_key":
        return np.full(1000, 7)
    if name == "zero_runs":
        k = r.integers(1, 20, 203)
        k[:120] = 0
        return r.permutation(k)
    if name == "one_row":
        return np.array([n_items])
    return np.zeros(9, dtype=np.int64)                   # all padding: nothing is written


@pytest.mark.parametrize("d", [1, 13, 45, 50, 64])
def test_table_reduce_sums_runs_in_sorted_order(d):
    n_items = 300
    r = np.random.default_rng(d)
    for name in ("random", "one_key", "zero_runs", "one_row", "all_pad"):
        keys = torch.from_numpy(_table_keys(name, r, n_items).astype(np.int64))
        sk, order = torch.sort(keys, stable=True)
        n = keys.numel()
        for ints in (True, False):
            contrib = (r.integers(-5, 6, (n, d)) if ints else r.standard_normal((n, d))).astype(np.float32)
            T = Buf.sentinel((n_items + 1) * d)
            K, Od, Ct = Buf(sk.numpy(), torch.int64), Buf(order.numpy(), torch.int64), Buf(contrib)
            _ok(_L().srfrd_table_reduce(K.p(), Od.p(), Ct.p(), n, d, T.p(), _st()), "srfrd_table_reduce")
            torch.cuda.synchronize()
            got = T.get().reshape(n_items + 1, d)
            want = np.full((n_items + 1, d), np.array([SENT32], dtype=np.uint32).view(np.float32)[0], dtype=np.float32)
            skn, on = sk.numpy(), order.numpy()
            i = 0
            while i < n:
                j = i
                acc = np.zeros(d, dtype=np.float32)
                while j < n and skn[j] == skn[i]:
                    acc = (acc + contrib[on[j]]).astype(np.float32)       # float32 sequential sum in `order`
                    j += 1
                if skn[i] != 0:
                    want[skn[i]] = acc
                i = j
            assert (_bits(got) == _bits(want)).all(), (name, ints)


# ---- srfrd_table_to_bf16 ------------------------------------------------------------------------------------------------
SPECIAL = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000,           # +-0, +-Inf
                    0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0xFFC00001,           # NaNs (quiet, signalling, negative)
                    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                       # round to +-Inf; a tie at the top that does too
                    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,           # exact ties: to even down / up, both signs
                    0x3F808001, 0x3F807FFF, 0x3F800000,
                    0x00000001, 0x80000001, 0x00008000, 0x00018000,           # fp32 denormals, ties among them
                    0x00007FFF, 0x007FFFFF, 0x807FFFFF, 0x007F8000, 0x00400000], dtype=np.uint32)


def _to_bf16(x):
    X, Hb = Buf(x), Buf.sentinel(x.size, torch.int16)
    _ok(_L().srfrd_table_to_bf16(X.p(), x.size, Hb.p(), _st()), "srfrd_table_to_bf16")
    torch.cuda.synchronize()
    return _bits(Hb.get())


def _check_bf16(x, h):
    xb = _bits(x)
    nan = (xb & 0x7FFFFFFF) > 0x7F800000
    assert ((h[nan] & 0x7F80) == 0x7F80).all() and ((h[nan] & 0x7F) != 0).all(), "NaN must stay NaN"
    want = _bf16_rne(x)
    assert (h[~nan] == want[~nan]).all(), [(hex(a), hex(b), hex(c)) for a, b, c in zip(xb[~nan], h[~nan], want[~nan]) if b != c][:5]
    # the restatement agrees with torch's CPU conversion wherever that is not host-dependent (normal numbers)
    normal = ~nan & ((xb & 0x7F800000) != 0)
    t = torch.from_numpy(x[normal].copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (t == want[normal]).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 2_100_003])
def test_table_to_bf16_rounds_to_nearest_even(n):
    if n <= 5:
        for k in range(SPECIAL.size):                     # every special value at every position of the float4 and the tail
            x = np.roll(SPECIAL, -k)[:n].view(np.float32).copy()
            _check_bf16(x, _to_bf16(x))
        return
    r = np.random.default_rng(1)
    xb = r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # every pattern: NaNs, denormals, ties included
    xb[::3] = (r.standard_normal(xb[::3].size).astype(np.float32)).view(np.uint32) & 0xFFFF8000 | 0x8000   # exact ties
    xb[1::97] = np.resize(SPECIAL, xb[1::97].size)
    x = xb.view(np.float32)
    _check_bf16(x, _to_bf16(x))


# ---- srfrd_l2_norms / srfrd_l2_apply ------------------------------------------------------------------------------------
def _l2_depth(seg_len):
    """rounding steps of one segment's sum of squares: the per-thread accumulator chain, the 4-way + wave + block trees"""
    return int(np.ceil(seg_len / 1024)) + 24


def _run_l2(param, segs, n_table_pad, n_dense, l2):
    n_seg = len(segs)
    P = Buf(param)
    so = Buf(np.array([o for o, _ in segs], dtype=np.int64), torch.int64)
    sl = Buf(np.array([k for _, k in segs], dtype=np.int64), torch.int64)
    part, l2buf, ds = Buf.sentinel(240 + n_seg), Buf.sentinel(2), Buf(np.zeros(n_dense, dtype=np.float32))
    _ok(_L().srfrd_l2_norms(P.p(), so.p(), sl.p(), n_seg, n_table_pad, l2, part.p(), l2buf.p(), ds.p(), _st()), "srfrd_l2_norms")
    torch.cuda.synchronize()
    part.get()
    return l2buf.get(), ds.get()


def _check_l2(param, segs, n_table_pad, l2, l2buf, ds):
    l2f = float(np.float32(l2))
    n_table = segs[0][1]
    per = ((n_table + 239) // 240 + 3) // 4 * 4
    nrm, scale, rel = [], [], []
    for k, (o, ln) in enumerate(segs):
        x = param[o:o + ln].astype(np.float64)
        nr = float(np.sqrt(x @ x))
        r = 2 * (_l2_depth(per if k == 0 else ln) / 2 + 3) * U
        nrm.append(nr); rel.append(r)
        scale.append(l2f / nr if nr > 0 else 0.0)
    if scale[0] == 0:
        assert l2buf[0] == 0
    else:
        assert abs(l2buf[0] - scale[0]) <= rel[0] * scale[0], (l2buf[0], scale[0])
    tot = l2f * sum(nrm)
    assert abs(l2buf[1] - tot) <= (2 * len(segs) * U + max(rel)) * tot, (l2buf[1], tot)
    want_zero = np.ones(ds.size, dtype=bool)
    for k in range(1, len(segs)):
        o, ln = segs[k]
        s = ds[o - n_table_pad:o - n_table_pad + ln]
        want_zero[o - n_table_pad:o - n_table_pad + ln] = False
        assert (_bits(s) == _bits(s[:1])).all(), k                     # one scale per tensor
        if scale[k] == 0:
            assert (s == 0).all(), k
        else:
            assert abs(float(s[0]) - scale[k]) <= rel[k] * scale[k], (k, float(s[0]), scale[k])
    assert (ds[want_zero] == 0).all()                                     # alignment gaps


def _model_segs(kind):
    import srfrd_amd
    torch.manual_seed(0)
    m = srfrd_amd.SASRec(400, 50, 50, 0.0, 2, 1, "cuda") if kind == "SASRec" else srfrd_amd.SRFRN(300, 20, 45, 5, 0.0, 3, 1, "cuda")
    m = m.cuda()
    m.flat_parameters()
    return [(off, p.numel()) for p, off in m._slots], m.n_table_pad, m.n_flat


def _synthetic_segs(name, r):
    """(segs, n_table_pad, n) of a synthetic flat vector: segment 0 the table at 0, the others at or above n_table_pad"""
    n_table = {"one_seg": 1001 * 50, "seg128": 7 * 13, "big": 1_000_000 * 50, "zero_table": 45 * 10}[name]
    ntp = (n_table + 3) // 4 * 4
    segs, o = [(0, n_table)], ntp
    n_dense_segs = {"one_seg": 0, "seg128": 127, "big": 5, "zero_table": 3}[name]
    for _ in range(n_dense_segs):
        o += int(r.integers(0, 4))                                       # alignment gaps between tensors
        ln = int(r.integers(1, 3000))
        segs.append((o, ln))
        o += ln
    return segs, ntp, (o + 3) // 4 * 4 + 4


@pytest.mark.parametrize("name", ["SASRec", "SRFRN", "one_seg", "seg128", "zero_table", "big"])
def test_l2_norms_against_fp64(name):
    r = np.random.default_rng(len(name))
    if name in ("SASRec", "SRFRN"):
        segs, ntp, n = _model_segs(name)
    else:
        segs, ntp, n = _synthetic_segs(name, r)
    param = r.standard_normal(n).astype(np.float32)
    if name == "seg128":
        o, ln = segs[40]
        param[o:o + ln] = 0.0                                             # an all-zero tensor: scale 0, norm 0
    if name == "zero_table":
        param[:segs[0][1]] = 0.0
    l2 = 1e-3 if name != "big" else 0.37
    l2buf, ds = _run_l2(param, segs, ntp, n - ntp, l2)
    _check_l2(param, segs, ntp, l2, l2buf, ds)


@pytest.mark.parametrize("kind", ["SASRec", "SRFRN"])
def test_l2_apply_over_slices_that_cross_the_table_end(kind):
    r = np.random.default_rng(3)
    segs, ntp, n = _model_segs(kind)
    param = r.standard_normal(n).astype(np.float32)
    l2buf, ds = _run_l2(param, segs, ntp, n - ntp, 1e-2)
    g = r.standard_normal(n).astype(np.float32)
    P, LB, DS = Buf(param), Buf(l2buf), Buf(ds)
    for i0, i1 in ((0, n), (ntp - 6, ntp + 10), (ntp, ntp + 1), (ntp - 1, ntp), (3, ntp - 1), (n - 5, n), (5, 5)):
        for stats in (None, np.array([1.0, 2.0, 37.0, 0.0], dtype=np.float32)):
            Gr, S = Buf(g), (Buf(stats) if stats is not None else None)
            _ok(_L().srfrd_l2_apply(Gr.p(), P.p(), i0, i1, ntp, LB.p(), DS.p(), S.p() if S else None, _st()), "srfrd_l2_apply")
            torch.cuda.synchronize()
            got = Gr.get()
            cnt = 1.0 if stats is None else 37.0
            sc = np.where(np.arange(n) < ntp, float(l2buf[0]), np.concatenate([np.zeros(ntp), ds.astype(np.float64)]))
            add = cnt * sc[i0:i1] * param[i0:i1].astype(np.float64)
            want = g[i0:i1].astype(np.float64) + add
            bound = 2 * U * (np.abs(want) + 3 * np.abs(add))
            assert (np.abs(got[i0:i1] - want) <= bound).all(), (i0, i1)
            assert (_bits(got[:i0]) == _bits(g[:i0])).all() and (_bits(got[i1:]) == _bits(g[i1:])).all()
