"""CPU-only: the entry points of the losses with K negatives per position (srfrd_tneg_workspace_floats, srfrd_tneg_fwd,
srfrd_tneg_bwd, srfrd_table_reduce_rank1) are declared, exported and typed; the workspace query grows with K; arguments they
refuse are refused before anything touches a GPU (null pointers, K <= 0, an unknown objective, log_q with gbce, a negative
or non-finite beta -> SRFRD_E_ARG; a bf16-table layout, hidden width > 64 or SRFRN with gbce -> SRFRD_E_UNSUPPORTED);
the ops are registered with fake impls; srfrd_amd.gbce_beta and srfrd_amd.sample_token_negatives do what they state."""
import ctypes as C
import math
import os

import pytest

NEW = ("srfrd_tneg_workspace_floats", "srfrd_tneg_fwd", "srfrd_tneg_bwd", "srfrd_table_reduce_rank1")
E_ARG, E_UNSUPPORTED = -1, -2
SOFTMAX, GBCE = 0, 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


FWD_PTRS = ("table", "hidden", "targets", "negatives", "log_q", "token_loss", "lse", "stats", "workspace")
BWD_PTRS = ("table", "hidden", "targets", "negatives", "log_q", "lse", "d_token_loss", "d_hidden", "contrib_coef",
            "contrib_keys", "workspace")


def _fwd(lib, lay, B=4, L=20, K=10, objective=SOFTMAX, beta=1.0, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in FWD_PTRS}
    return lib.srfrd_tneg_fwd(C.byref(lay), a["table"], a["hidden"], a["targets"], a["negatives"], a["log_q"], K, objective, beta,
                              1, B, L, a["token_loss"], a["lse"], a["stats"], a["workspace"], ws_floats, None)


def _bwd(lib, lay, B=4, L=20, K=10, objective=SOFTMAX, beta=1.0, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in BWD_PTRS}
    return lib.srfrd_tneg_bwd(C.byref(lay), a["table"], a["hidden"], a["targets"], a["negatives"], a["log_q"], K, objective, beta,
                              1, a["lse"], a["d_token_loss"], B, L, a["d_hidden"], a["contrib_coef"], a["contrib_keys"],
                              a["workspace"], ws_floats, None)


def _reduce(lib, n=1000, d_item=50, d_out=50, rpt=11, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in ("sorted_keys", "order", "contrib_coef", "hidden", "grad_table", "workspace")}
    return lib.srfrd_table_reduce_rank1(a["sorted_keys"], a["order"], a["contrib_coef"], a["hidden"], d_out, rpt, n, d_item,
                                        a["grad_table"], a["workspace"], ws_floats, None)


def test_new_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import ROOT, header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), s)
    assert len(_lib.SIGNATURES["srfrd_tneg_fwd"][1]) == 18 and len(_lib.SIGNATURES["srfrd_tneg_bwd"][1]) == 20
    assert len(_lib.SIGNATURES["srfrd_table_reduce_rank1"][1]) == 12
    assert _lib.SIGNATURES["srfrd_tneg_fwd"][1][8] is C.c_double            # beta
    assert _lib.TNEG_OBJECTIVES == {"softmax": SOFTMAX, "gbce": GBCE}
    hdr = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    assert f"#define SRFRD_TNEG_SPLIT_ROWS {_lib.TNEG_SPLIT_ROWS}\n" in hdr
    assert "#define SRFRD_TNEG_SOFTMAX 0\n" in hdr and "#define SRFRD_TNEG_GBCE 1\n" in hdr


def test_workspace_floats_grow_with_k(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 50_000, 50, 50, 0, 0, 2, 1)
    T = 512 * 50
    sizes = [lib.srfrd_tneg_workspace_floats(C.byref(lay), 512, 50, K) for K in (1, 16, 64, 256, 1024)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for K, s in zip((1, 16, 64, 256, 1024), sizes):
        segs = -(-T * (1 + K) // _lib.TNEG_SPLIT_ROWS)
        assert s >= 2 * segs * 50                   # two partial rows per segment of the rank-1 reduce
        assert s <= 2 * segs * 50 + T + 256         # and little else: nothing of size tokens x K x d_item
    assert lib.srfrd_tneg_workspace_floats(C.byref(lay), 0, 50, 16) == 0
    assert lib.srfrd_tneg_workspace_floats(C.byref(lay), 512, 50, 0) == 0
    assert lib.srfrd_tneg_workspace_floats(C.byref(lay), 512, 50, -5) == 0
    assert lib.srfrd_tneg_workspace_floats(C.byref(lay), 512, 50, 1 << 20) == 0     # B L (1 + K) >= 2^31
    assert lib.srfrd_tneg_workspace_floats(None, 4, 20, 10) == 0


def test_null_pointers_and_sizes_are_refused(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SRFRN", 100, 20, 45, 5, 0, 2, 1)
    for k in FWD_PTRS:
        if k != "log_q":
            assert _fwd(lib, lay, **{k: 1}) == E_ARG, k
    for k in BWD_PTRS:
        if k != "log_q":
            assert _bwd(lib, lay, **{k: 1}) == E_ARG, k
    for K in (0, -1):
        assert _fwd(lib, lay, K=K) == E_ARG and _bwd(lib, lay, K=K) == E_ARG
    assert _fwd(lib, lay, B=0) == E_ARG and _bwd(lib, lay, L=0) == E_ARG
    need = lib.srfrd_tneg_workspace_floats(C.byref(lay), 4, 20, 10)
    assert need > 0
    assert _fwd(lib, lay, ws_floats=need - 1) == E_ARG and _bwd(lib, lay, ws_floats=need - 1) == E_ARG
    assert lib.srfrd_tneg_fwd(None, _d(), _d(), _d(), _d(), None, 10, SOFTMAX, 1.0, 1, 4, 20, _d(), _d(), _d(), _d(), 1 << 40,
                              None) == E_ARG


def test_objective_beta_and_log_q_are_checked(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    for f in (_fwd, _bwd):
        for objective in (-1, 2, 7):
            assert f(lib, lay, objective=objective) == E_ARG
        assert f(lib, lay, objective=GBCE) == E_ARG                          # log_q given with gbce
        for beta in (-0.5, float("inf"), float("-inf"), float("nan")):
            assert f(lib, lay, objective=GBCE, beta=beta, log_q=1) == E_ARG, beta


def test_unsupported_layouts(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    lay.table_bf16 = 1
    assert _fwd(lib, lay) == E_UNSUPPORTED and _bwd(lib, lay) == E_UNSUPPORTED
    assert lib.srfrd_tneg_workspace_floats(C.byref(lay), 4, 20, 10) == 0
    wide = _lib.make_layout("SASRec", 100, 20, 72, 0, 0, 2, 1)
    assert _fwd(lib, wide) == E_UNSUPPORTED and _bwd(lib, wide) == E_UNSUPPORTED
    assert lib.srfrd_tneg_workspace_floats(C.byref(wide), 4, 20, 10) == 0
    srfrn = _lib.make_layout("SRFRN", 100, 20, 45, 5, 0, 2, 1)
    assert _fwd(lib, srfrn, objective=GBCE, log_q=1) == E_UNSUPPORTED and _bwd(lib, srfrn, objective=GBCE, log_q=1) == E_UNSUPPORTED
    srfr = _lib.make_layout("SRFR", 100, 20, 45, 5, 0, 2, 1)
    need = lib.srfrd_tneg_workspace_floats(C.byref(srfr), 4, 20, 10)
    assert _fwd(lib, srfr, objective=GBCE, log_q=1, ws_floats=need - 1) == E_ARG      # SRFR passes the kind check


def test_rank1_reduce_refusals(lib):
    from srfrd_amd import _lib
    for k in ("sorted_keys", "order", "contrib_coef", "hidden", "grad_table", "workspace"):
        assert _reduce(lib, **{k: 1}) == E_ARG, k
    assert _reduce(lib, n=0) == E_ARG and _reduce(lib, n=1 << 31) == E_ARG
    assert _reduce(lib, rpt=0) == E_ARG
    assert _reduce(lib, d_item=0) == E_ARG and _reduce(lib, d_item=65, d_out=65) == E_ARG and _reduce(lib, d_out=49) == E_ARG
    need = 2 * -(-1000 // _lib.TNEG_SPLIT_ROWS) * 50
    assert _reduce(lib, ws_floats=need - 1) == E_ARG


def test_ops_registered_with_fake_impls():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import srfrd_amd
    from srfrd_amd import ops
    assert "tneg_fwd" in ops.OPS and "tneg_bwd" in ops.OPS
    assert torch.ops.srfrd.tneg_fwd.default._schema.name == "srfrd::tneg_fwd"
    assert torch.ops.srfrd.tneg_bwd.default._schema.name == "srfrd::tneg_bwd"
    assert hasattr(srfrd_amd.SASRec, "token_negatives_loss")
    with FakeTensorMode():
        h = torch.empty(3, 7, 50)
        y = torch.empty(3, 7, dtype=torch.int64)
        neg = torch.empty(3, 7, 5, dtype=torch.int64)
        table = torch.empty(101, 50)
        tl, lse, stats = torch.ops.srfrd.tneg_fwd(h, y, neg, None, table, 0, 1.0, True, 0)
        assert tl.shape == (3, 7) and lse.shape == (3, 7) and stats.shape == (2,) and tl.dtype == torch.float32
        dh, de = torch.ops.srfrd.tneg_bwd(h, y, neg, None, table, 1, 0.5, False, lse, tl, 0)
        assert dh.shape == h.shape and de.shape == table.shape


def test_gbce_beta():
    import srfrd_amd
    n, K = 50_000, 256
    a = K / (n - 1)
    assert srfrd_amd.gbce_beta(n, K, 0.0) == pytest.approx(1.0, rel=1e-12)
    assert srfrd_amd.gbce_beta(n, K, 1.0) == pytest.approx(a, rel=1e-12)
    t = 0.75
    assert srfrd_amd.gbce_beta(n, K, t) == pytest.approx(a * (t * (1.0 - 1.0 / a) + 1.0 / a), rel=1e-12)
    assert srfrd_amd.gbce_beta(n, K, t) == pytest.approx(1.0 - t * (1.0 - a), rel=1e-9)       # the same, expanded
    assert srfrd_amd.gbce_beta(2, 1, 0.3) == pytest.approx(1.0, rel=1e-12)                     # alpha = 1: beta = 1 for any t
    for bad in (dict(t=-0.01), dict(t=1.01), dict(t=float("nan")), dict(K=0), dict(K=n), dict(K=-3)):
        with pytest.raises(ValueError):
            srfrd_amd.gbce_beta(n, bad.get("K", K), bad.get("t", 0.5))


def _positives(B, L, n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(1, n + 1, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 0.4] = 0
    y[1] = 0
    return y


def test_sample_token_negatives_uniform_on_cpu():
    import torch
    import srfrd_amd
    n, num = 1000, 33
    y = _positives(6, 40, n, 0)
    ids, log_q = srfrd_amd.sample_token_negatives(n, y, num, generator=torch.Generator().manual_seed(1))
    assert ids.dtype == torch.int64 and ids.shape == (6, 40, num) and log_q.dtype == torch.float32 and log_q.shape == (6, 40, num)
    live = y != 0
    assert int(ids[live].min()) >= 1 and int(ids[live].max()) <= n
    assert bool((ids[~live] == 0).all())
    assert torch.allclose(log_q[live], torch.full_like(log_q[live], math.log(num / n)))
    assert len(torch.unique(ids[live])) > 900
    again, log_q2 = srfrd_amd.sample_token_negatives(n, y, num, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ids, again) and torch.equal(log_q, log_q2)
    other, _ = srfrd_amd.sample_token_negatives(n, y, num, generator=torch.Generator().manual_seed(2))
    assert not torch.equal(ids, other)


def test_sample_token_negatives_by_counts_on_cpu():
    import torch
    import srfrd_amd
    n, num = 50, 40
    counts = torch.zeros(n + 1)
    counts[0] = 1e9                                             # the padding id: ignored
    counts[1:11] = torch.arange(1, 11, dtype=torch.float32)     # items 11..50 never occur
    y = _positives(16, 50, n, 3)
    live = y != 0
    for alpha in (1.0, 0.5):
        ids, log_q = srfrd_amd.sample_token_negatives(n, y, num, counts=counts, alpha=alpha,
                                                      generator=torch.Generator().manual_seed(1))
        assert int(ids[live].min()) >= 1 and int(ids[live].max()) <= 10 and bool((ids[~live] == 0).all())
        w = counts[1:11].double() ** alpha
        q = w / w.sum()
        assert torch.allclose(log_q[live].double(), torch.log(num * q[ids[live] - 1]), atol=1e-6)
        freq = torch.bincount(ids[live].view(-1), minlength=n + 1)[1:11].double() / ids[live].numel()
        assert float((freq - q).abs().max()) < 0.02
    with pytest.raises(ValueError):
        srfrd_amd.sample_token_negatives(n, y, 4, counts=torch.ones(n))
    with pytest.raises(ValueError):
        srfrd_amd.sample_token_negatives(n, y, 0)
    with pytest.raises(ValueError):
        srfrd_amd.sample_token_negatives(n, y[0], 4)
