"""-m gpu: the device side of the learning-rate schedule, gradient-norm clipping and decoupled weight decay (srfrd_step_begin_sched,
srfrd_grad_norm, srfrd_adamw_step, srfrd_adamw_pack_step) through the C ABI, against float64 restatements written here.  The
buffers sit between the guard words of tests/test_gpu_optim_kernels.py, whose inputs and reference the Adam cases reuse; what
a call does not own must come back bit-unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import srfrd_oracle as O
from tests.test_gpu_optim_kernels import (PACK_CASES, SENT16, U, Buf, _adam_inputs, _adam_ref, _bf16_rne, _bits, _L, _ok,
                                          _run_adam, _slices, _st)

pytestmark = pytest.mark.gpu

KINDS = ("constant", "linear", "cosine")
INF = float("inf")


def _opts(lr=1e-3, b1=0.9, b2=0.98, wd=0.0, kind="constant", warmup=0, total=0, ratio=0.0):
    from srfrd_amd import _lib
    return _lib.OptimOpts(lr, b1, b2, wd, ratio, warmup, total, _lib.SCHEDULES[kind], 0)


def _f32(words, i):
    return float(words[i:i + 1].view(np.float32)[0])


def _near(got, want):
    """within one fp32 spacing of the fp64 value"""
    return abs(got - want) <= np.spacing(np.float32(abs(want)))


# ---- srfrd_step_begin_sched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_step_begin_sched_words(kind):
    from srfrd_amd import lr_at
    lr, b1, b2, wd, w, total, r, base = 3e-3, 0.9, 0.98, 0.1, 4, 11, 0.1, 0x2468ACE
    o = _opts(lr, b1, b2, wd, kind, w, total, r)
    for t0 in (0, 1, w - 1, w, w + 1, total - 1, total, total + 5, 1 << 20):
        s = np.arange(32, dtype=np.int32) * 7 + 1000          # words the advance must not touch keep these
        s[0], s[1] = t0, base
        st = Buf(s, torch.int32)
        _ok(_L().srfrd_step_begin_sched(st.p(), C.byref(o), _st()), "srfrd_step_begin_sched")
        torch.cuda.synchronize()
        got = st.get()
        t = t0 + 1
        lr_t = lr_at(t, lr, kind, w, total, r)
        assert int(got[0]) == t and int(got[1]) == base
        assert int(got[2:3].view(np.uint32)[0]) == O.step_seed(base, t)
        assert _near(_f32(got, 3), lr_t), (t, _f32(got, 3), lr_t)
        assert _near(_f32(got, 4), lr_t / (1.0 - b1 ** t)), t
        assert _near(_f32(got, 5), np.sqrt(1.0 - b2 ** t)), t
        assert _near(_f32(got, 7), 1.0 - lr_t * wd), (t, _f32(got, 7))
        keep = [i for i in range(32) if i not in (0, 2, 3, 4, 5, 7)]
        assert (got[keep] == s[keep]).all(), t


@pytest.mark.parametrize("t0", [0, 1, 9, 999, 1 << 20])
def test_step_begin_sched_neutral_is_step_begin(t0):
    lr, b1, b2 = 3e-3, 0.9, 0.999
    s = np.arange(32, dtype=np.int32) * 7 + 1000
    s[0], s[1] = t0, 0x13579B
    a, b = Buf(s, torch.int32), Buf(s, torch.int32)
    _ok(_L().srfrd_step_begin(a.p(), lr, b1, b2, _st()), "srfrd_step_begin")
    _ok(_L().srfrd_step_begin_sched(b.p(), C.byref(_opts(lr, b1, b2)), _st()), "srfrd_step_begin_sched")
    torch.cuda.synchronize()
    wa, wb = a.get(), b.get()
    assert all(wa[i] == wb[i] for i in (0, 1, 2, 4, 5)), (wa[:8], wb[:8])
    assert _f32(wb, 3) == float(np.float32(lr)) and _f32(wb, 7) == 1.0


# ---- srfrd_grad_norm ----------------------------------------------------------------------------------------------------
def _grad_norm(g, stats=None, max_norm=INF, twice=False):
    """-> out (2 floats); every buffer guarded, the gradient bit-unchanged; `twice`: also a second call, bitwise the first"""
    from srfrd_amd import _lib
    Gr = Buf(g)
    S = Buf(stats) if stats is not None else None
    outs = []
    for _ in range(2 if twice else 1):
        part, out = Buf.sentinel(_lib.GRAD_NORM_PARTIALS, torch.int64), Buf.sentinel(2)
        _ok(_L().srfrd_grad_norm(Gr.p(), g.size, S.p() if S else None, max_norm, part.p(), out.p(), _st()), "srfrd_grad_norm")
        torch.cuda.synchronize()
        part.get()
        outs.append(out.get())
    assert (_bits(Gr.get()) == _bits(g)).all()
    if S:
        assert (_bits(S.get()) == _bits(stats)).all()
    if twice:
        assert (_bits(outs[0]) == _bits(outs[1])).all()
    return outs[0]


def _sizes():
    from srfrd_amd import _lib
    share, parts = _lib.GRAD_NORM_SHARE, _lib.GRAD_NORM_PARTIALS
    # the float4 body and its tail, one workgroup's share +-1, two shares + 3, beyond one pass of the whole grid (every
    # workgroup loops), and beyond `parts` minimum shares (where the shares grow)
    return [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, share - 1, share, share + 1, 2 * share + 3, 3 * (1 << 20) + 5,
            share * parts + share + 5]


@pytest.mark.parametrize("n", _sizes())
def test_grad_norm_sizes(n):
    r = np.random.default_rng(n)
    ints = r.integers(-2, 3, n).astype(np.float32)               # the fp64 sum of squares is exact
    S = float((ints.astype(np.int64) ** 2).sum())
    out = _grad_norm(ints, twice=True)
    assert _near(float(out[0]), np.sqrt(S)), (out[0], np.sqrt(S))
    assert out[1] == 1.0
    x = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 4, n)).astype(np.float32)
    want = float(np.sqrt(np.sum(x.astype(np.float64) ** 2)))
    stats = np.array([3.5, 1.25, 37.0, 0.0], dtype=np.float32)
    out = _grad_norm(x, twice=True)
    assert _near(float(out[0]), want), (out[0], want)
    out = _grad_norm(x, stats)
    assert _near(float(out[0]), want / 37.0), (out[0], want / 37.0)


def test_grad_norm_coefficient():
    r = np.random.default_rng(5)
    x = r.standard_normal(5003).astype(np.float32)
    norm = float(np.sqrt(np.sum(x.astype(np.float64) ** 2)))
    stats = np.array([0.0, 2.0, 8.0, 0.0], dtype=np.float32)
    assert _grad_norm(x, None, 2.0 * norm)[1] == 1.0              # below max_norm
    assert _grad_norm(x, None, INF)[1] == 1.0                     # measuring only
    assert _grad_norm(x, stats, 0.2 * norm)[1] == 1.0             # (the norm is that of the SCALED gradient: norm / 8)
    zero = _grad_norm(np.zeros(777, dtype=np.float32), None, 0.5)
    assert zero[0] == 0.0 and zero[1] == 1.0
    for st, scale in ((None, 1.0), (stats, 1.0 / 8.0)):
        for frac in (0.999, 0.5, 1e-3):
            mx = frac * norm * scale
            out = _grad_norm(x, st, mx)
            assert _near(float(out[0]), norm * scale)
            want = mx / (float(out[0]) + 1e-6)                    # the header's definition: from the norm it reports
            assert want < 1.0 and abs(float(out[1]) - want) <= 2 * U * want, (out, want)
            assert abs(float(out[1]) - mx / (norm * scale + 1e-6)) <= 3 * U * want
    for at in (0, 4097, 5002):                                    # one NaN element: the body, another workgroup, the tail
        y = x.copy()
        y[at] = np.nan
        out = _grad_norm(y, None, 1.0)
        assert np.isnan(out[0]) and np.isnan(out[1]), (at, out)
        assert np.isnan(_grad_norm(y, None, INF)[1])


# ---- srfrd_adamw_step ---------------------------------------------------------------------------------------------------
def _sched_state(t0, o, base=12345):
    """an optimizer state after srfrd_step_begin_sched from t0; -> (Buf, step_size, bc2_sqrt, decay) as the device holds them"""
    s = np.zeros(32, dtype=np.int32)
    s[0], s[1] = t0, base
    st = Buf(s, torch.int32)
    _ok(_L().srfrd_step_begin_sched(st.p(), C.byref(o), _st()), "srfrd_step_begin_sched")
    torch.cuda.synchronize()
    w = st.get()
    return st, _f32(w, 4), _f32(w, 5), _f32(w, 7)


def _run_adamw(p, g, m, v, i0, i1, n_zero, stats, clip, n_table, state, b=(0.9, 0.98), eps=1e-8):
    """tests/test_gpu_optim_kernels._run_adam for srfrd_adamw_step"""
    n = p.size
    P, Gr, M, V = Buf(p), Buf(g[i0:i1]), Buf(m[i0:i1]), Buf(v[i0:i1])
    S = Buf(stats) if stats is not None else None
    Cl = Buf(clip) if clip is not None else None
    H = Buf.sentinel(n_table, torch.int16) if n_table else None
    rc = _L().srfrd_adamw_step(P.p(), Gr.p(i0), M.p(i0), V.p(i0), n, i0, i1, n_zero, b[0], b[1], eps, state.p(),
                               S.p() if S else None, Cl.p() if Cl else None, H.p() if H else None, n_table, _st())
    _ok(rc, "srfrd_adamw_step")
    torch.cuda.synchronize()
    if Cl:
        assert (_bits(Cl.get()) == _bits(clip)).all()
    return P.get(), Gr.get(), M.get(), V.get(), (H.get() if H else None)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 4099])
def test_adamw_step_neutral_is_adam_step(n):
    """clip NULL, decay 0, a constant schedule: bitwise srfrd_adam_step on the n % 4 tails, the [i0, i1) slices, n_zero and the
    bf16 shadow"""
    p, g, m, v = _adam_inputs(n, n)
    state, _, _, decay = _sched_state(6, _opts())
    assert decay == 1.0
    stats_v = np.array([3.5, 1.25, 37.0, 0.0], dtype=np.float32)
    for k, (i0, i1) in enumerate(_slices(n)):
        for stats in (None, stats_v):
            for n_zero in sorted({0, 3, 6, max(n - 2, 0), n}):
                n_table = (0, 5, 4097)[(k + n_zero) % 3]
                a = _run_adam(p, g, m, v, i0, i1, n_zero, stats, n_table, state)
                b = _run_adamw(p, g, m, v, i0, i1, n_zero, stats, None, n_table, state)
                for x, y in zip(a, b):
                    assert (x is None and y is None) or (_bits(x) == _bits(y)).all(), (i0, i1, n_zero, n_table)


def _adamw_ref(p, g, m, v, b1, b2, eps, ss, bc2s, gscale, coef, decay):
    """fp64 AdamW of fp32 inputs + elementwise bounds: _adam_ref's on the decayed parameter and the clipped scale, widened by the
    two roundings it does not know - gs = fl(gscale coef), one relative U on every g gs (so U (1 - b1) |g gs| on m, 2 U (1 - b2)
    (g gs)^2 on v, hence at most U relative on the denominator and on the update), and fl(p decay), U |p decay| on p; doubled
    like the rest."""
    gs = gscale * coef
    pd = p.astype(np.float64) * decay
    rp, rm, rv, ep, em, ev = _adam_ref(pd, g, m, v, b1, b2, eps, ss, bc2s, gs)      # (pd is passed on in float64)
    b1f, b2f = float(np.float32(b1)), float(np.float32(b2))
    ggs = np.abs(g.astype(np.float64) * gs)
    em_x = U * (1 - b1f) * ggs
    ev_x = 2 * U * (1 - b2f) * ggs * ggs
    den = np.sqrt(rv) / bc2s + float(np.float32(eps))
    upd = np.abs(pd - rp)
    ep_x = U * np.abs(pd) + ss / den * em_x + upd * U
    return rp, rm, rv, ep + 2 * ep_x, em + 2 * em_x, ev + 2 * ev_x


@pytest.mark.parametrize("n", [5, 4099])
def test_adamw_step_against_fp64(n):
    p, g, m, v = _adam_inputs(n, 3 * n)
    o = _opts(lr=1e-2, wd=0.1, kind="linear", warmup=2, total=9, ratio=0.1)
    state, ss, bc2s, decay = _sched_state(4, o)
    assert 0.99 < decay < 1.0
    stats_v = np.array([3.5, 1.25, 37.0, 0.0], dtype=np.float32)
    clip_v = np.array([12.5, 0.37], dtype=np.float32)
    for i0, i1 in _slices(n)[:3]:
        for stats in (None, stats_v):
            for clip in (None, clip_v):
                n_zero, n_table = (3, 5) if clip is None else (n, 4097)
                po, go, mo, vo, ho = _run_adamw(p, g, m, v, i0, i1, n_zero, stats, clip, n_table, state)
                gscale = 1.0 / 37.0 if stats is not None else 1.0
                coef = float(clip[1]) if clip is not None else 1.0
                rp, rm, rv, ep, em, ev = _adamw_ref(p[i0:i1], g[i0:i1], m[i0:i1], v[i0:i1], 0.9, 0.98, 1e-8, ss, bc2s, gscale,
                                                    coef, decay)
                assert (np.abs(po[i0:i1] - rp) <= ep).all(), float(np.max(np.abs(po[i0:i1] - rp) / ep))
                assert (np.abs(mo - rm) <= em).all(), float(np.max(np.abs(mo - rm) / em))
                assert (np.abs(vo - rv) <= ev).all(), float(np.max(np.abs(vo - rv) / ev))
                assert (_bits(po[:i0]) == _bits(p[:i0])).all() and (_bits(po[i1:]) == _bits(p[i1:])).all()
                idx = np.arange(i0, i1)
                assert (go[idx < n_zero] == 0).all() and (_bits(go[idx >= n_zero]) == _bits(g[i0:i1][idx >= n_zero])).all()
                hb = _bits(ho)
                lo, hi = min(i0, n_table), min(i1, n_table)
                assert (hb[lo:hi] == _bf16_rne(po[lo:hi])).all() and (hb[:lo] == SENT16).all() and (hb[hi:] == SENT16).all()
    # the decay and the clip are really applied: far outside the bound of the plain step
    plain = _run_adam(p, g, m, v, 0, n, 0, stats_v, 0, state)
    full = _run_adamw(p, g, m, v, 0, n, 0, stats_v, clip_v, 0, state)
    assert np.abs(plain[0] - full[0]).max() > 1e-4 and np.abs(plain[2] - full[2]).max() > 1e-4


# ---- srfrd_adamw_pack_step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neutral", [True, False], ids=["neutral", "options"])
@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"{c[0]}_{c[3]}+{c[4]}_b{c[6]}")
def test_adamw_pack_step(case, neutral):
    """neutral: every output and state word 0, 1, 2, 4, 5 bitwise srfrd_adam_pack_step's.  With the options: parameters,
    moments, gradient and shadow bitwise srfrd_adamw_step's (held to fp64 above), the packed copy a fresh srfrd_pack_weights,
    the state srfrd_step_begin_sched's advance, the ticket words back at 0."""
    from srfrd_amd import _lib
    kind, I, L, d_item, d_fake, n_labels, n_blocks = case
    lay = _lib.make_layout(kind, I, L, d_item, d_fake, n_labels, n_blocks, 1)
    n_tab = (lay.n_table + 3) // 4 * 4
    n = (n_tab + lay.n_dense + 3) // 4 * 4
    lr, b1, b2, eps = 2e-3, 0.9, 0.98, 1e-8
    o = _opts(lr, b1, b2) if neutral else _opts(lr, b1, b2, 0.05, "cosine", 1, 3, 0.2)
    p, g, m, v = _adam_inputs(n, I)
    p[lay.n_table:n_tab] = 0.0
    P, M, V = Buf(p), Buf(m), Buf(v)
    stats = Buf(np.array([2.0, 3.0, 41.0, 0.0], dtype=np.float32))
    clip = None if neutral else Buf(np.array([7.0, 0.61], dtype=np.float32))
    st0 = np.zeros(32, dtype=np.int32)
    st0[1] = 777
    state = Buf(st0, torch.int32)
    _ok(_L().srfrd_step_begin_sched(state.p(), C.byref(o), _st()), "srfrd_step_begin_sched")
    n_packed = _L().srfrd_packed_floats(C.byref(lay))
    packed = Buf(np.zeros(n_packed, dtype=np.float32))
    dense = lambda buf: C.c_void_p(buf.t.data_ptr() + 4 * n_tab)        # noqa: E731
    _ok(_L().srfrd_pack_weights(C.byref(lay), dense(P), packed.p(), None, 0.0, 0.0, 0.0, _st()), "srfrd_pack_weights")
    H = Buf.sentinel(lay.n_table, torch.int16)
    r = np.random.default_rng(5)
    for launch in range(3):
        g = (r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n)).astype(np.float32)
        Gr = Buf(g)
        P2, G2, M2, V2 = Buf(P.get()), Buf(g), Buf(M.get()), Buf(V.get())
        H2 = Buf(H.get(), torch.int16)
        s_before = state.get()
        S2 = Buf(s_before, torch.int32)
        if neutral:
            packed2 = Buf(packed.get())
            _ok(_L().srfrd_adam_pack_step(C.byref(lay), P2.p(), G2.p(), M2.p(), V2.p(), n, n_tab, n_tab, lr, b1, b2, eps, S2.p(),
                                          stats.p(), packed2.p(), H2.p(), _st()), "srfrd_adam_pack_step")
        else:
            _ok(_L().srfrd_adamw_step(P2.p(), G2.p(), M2.p(), V2.p(), n, 0, n, n_tab, b1, b2, eps, S2.p(), stats.p(), clip.p(),
                                      H2.p(), lay.n_table, _st()), "srfrd_adamw_step")
            _ok(_L().srfrd_step_begin_sched(S2.p(), C.byref(o), _st()), "srfrd_step_begin_sched")
        _ok(_L().srfrd_adamw_pack_step(C.byref(lay), P.p(), Gr.p(), M.p(), V.p(), n, n_tab, n_tab, C.byref(o), eps, state.p(),
                                       stats.p(), clip.p() if clip else None, packed.p(), H.p(), _st()), "srfrd_adamw_pack_step")
        fresh = Buf(np.zeros(n_packed, dtype=np.float32))
        _ok(_L().srfrd_pack_weights(C.byref(lay), dense(P), fresh.p(), None, 0.0, 0.0, 0.0, _st()), "srfrd_pack_weights")
        torch.cuda.synchronize()
        for a, b in ((P, P2), (Gr, G2), (M, M2), (V, V2), (H, H2)):
            assert (_bits(a.get()) == _bits(b.get())).all(), launch
        assert (Gr.get()[:n_tab] == 0).all() and (_bits(Gr.get()[n_tab:]) == _bits(g[n_tab:])).all()
        assert (_bits(packed.get()) == _bits(fresh.get())).all(), launch
        if neutral:
            assert (_bits(packed.get()) == _bits(packed2.get())).all(), launch
        s, want = state.get(), S2.get()
        assert s[6] == 0 and (s[8:24] == 0).all(), launch
        words = (0, 1, 2, 4, 5) if neutral else (0, 1, 2, 3, 4, 5, 7)
        assert all(s[i] == want[i] for i in words), (launch, s[:8], want[:8])
        assert (s[24:] == 0).all() and int(s[0]) == launch + 2
        if neutral:
            assert _f32(s, 3) == float(np.float32(lr)) and _f32(s, 7) == 1.0
        else:
            # (the state now holds t = launch + 2: half-way down the cosine, then at its floor from t = total = 3 on)
            assert _f32(s, 7) < 1.0 and (launch < 1) == (_f32(s, 3) > float(np.float32(0.2 * lr)))
    stats.get()
    if clip:
        clip.get()
