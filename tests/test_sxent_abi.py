"""CPU-only: the sampled softmax cross-entropy entry points (srfrd_sxent_workspace_floats, srfrd_sxent_fwd, srfrd_sxent_bwd)
are declared, exported and typed; the workspace query grows with K; arguments they refuse are refused before anything
touches a GPU (null pointers and K <= 0 -> SRFRD_E_ARG, a bf16-table layout or hidden width > 64 -> SRFRD_E_UNSUPPORTED);
srfrd_amd.sample_negatives draws in-range ids with the stated log-Q correction."""
import ctypes as C
import math

import pytest

NEW = ("srfrd_sxent_workspace_floats", "srfrd_sxent_fwd", "srfrd_sxent_bwd")
E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def _fwd(lib, lay, B=4, L=20, K=100, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in ("table", "hidden", "targets", "negatives", "log_q", "token_loss", "lse",
                                                     "stats", "workspace")}
    return lib.srfrd_sxent_fwd(C.byref(lay), a["table"], a["hidden"], a["targets"], a["negatives"], a["log_q"], K, 1, B, L,
                               a["token_loss"], a["lse"], a["stats"], a["workspace"], ws_floats, None)


def _bwd(lib, lay, B=4, L=20, K=100, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in ("table", "hidden", "targets", "negatives", "log_q", "lse", "d_token_loss",
                                                     "d_hidden", "table_contrib", "contrib_keys", "workspace")}
    return lib.srfrd_sxent_bwd(C.byref(lay), a["table"], a["hidden"], a["targets"], a["negatives"], a["log_q"], K, 1, a["lse"],
                               a["d_token_loss"], B, L, a["d_hidden"], a["table_contrib"], a["contrib_keys"], a["workspace"],
                               ws_floats, None)


def test_new_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), s)
    assert len(_lib.SIGNATURES["srfrd_sxent_fwd"][1]) == 16 and len(_lib.SIGNATURES["srfrd_sxent_bwd"][1]) == 18


def test_workspace_floats_grow_with_k(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 50_000, 50, 50, 0, 0, 2, 1)
    T = 512 * 50
    sizes = [lib.srfrd_sxent_workspace_floats(C.byref(lay), 512, 50, K) for K in (1, 256, 1024, 8192, 65536)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[0] >= 2 * T + 2 * T               # token list + target logits + at least one split of (max, sum) partials
    assert sizes[-1] >= 65536 * 50                 # the backward's dE partials (one token split at least)
    assert lib.srfrd_sxent_workspace_floats(C.byref(lay), 0, 50, 1024) == 0
    assert lib.srfrd_sxent_workspace_floats(C.byref(lay), 512, 50, 0) == 0
    assert lib.srfrd_sxent_workspace_floats(C.byref(lay), 512, 50, -5) == 0
    assert lib.srfrd_sxent_workspace_floats(None, 4, 20, 10) == 0


def test_null_pointers_and_sizes_are_refused(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SRFRN", 100, 20, 45, 5, 0, 2, 1)
    for k in ("table", "hidden", "targets", "negatives", "token_loss", "lse", "stats", "workspace"):
        assert _fwd(lib, lay, **{k: 1}) == E_ARG, k
    for k in ("table", "hidden", "targets", "negatives", "lse", "d_token_loss", "d_hidden", "table_contrib", "contrib_keys",
              "workspace"):
        assert _bwd(lib, lay, **{k: 1}) == E_ARG, k
    for K in (0, -1):
        assert _fwd(lib, lay, K=K) == E_ARG and _bwd(lib, lay, K=K) == E_ARG
    assert _fwd(lib, lay, B=0) == E_ARG and _bwd(lib, lay, L=0) == E_ARG
    need = lib.srfrd_sxent_workspace_floats(C.byref(lay), 4, 20, 100)
    assert _fwd(lib, lay, ws_floats=need - 1) == E_ARG and _bwd(lib, lay, ws_floats=need - 1) == E_ARG
    assert lib.srfrd_sxent_fwd(None, _d(), _d(), _d(), _d(), None, 10, 1, 4, 20, _d(), _d(), _d(), _d(), 1 << 40, None) == E_ARG


def test_unsupported_layouts(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    lay.table_bf16 = 1
    assert _fwd(lib, lay) == E_UNSUPPORTED and _bwd(lib, lay) == E_UNSUPPORTED
    wide = _lib.make_layout("SASRec", 100, 20, 72, 0, 0, 2, 1)
    assert _fwd(lib, wide) == E_UNSUPPORTED and _bwd(lib, wide) == E_UNSUPPORTED
    assert lib.srfrd_sxent_workspace_floats(C.byref(wide), 4, 20, 10) == 0


def test_ops_registered_with_fake_impls():
    import torch
    import srfrd_amd  # noqa: F401
    from srfrd_amd import ops
    assert "sxent_fwd" in ops.OPS and "sxent_bwd" in ops.OPS
    assert torch.ops.srfrd.sxent_fwd.default._schema.name == "srfrd::sxent_fwd"
    assert torch.ops.srfrd.sxent_bwd.default._schema.name == "srfrd::sxent_bwd"
    assert hasattr(srfrd_amd.SASRec, "sampled_softmax_loss")


def test_sample_negatives_uniform_on_cpu():
    import torch
    import srfrd_amd
    g = torch.Generator().manual_seed(0)
    ids, log_q = srfrd_amd.sample_negatives(1000, 4096, generator=g, device="cpu")
    assert ids.dtype == torch.int64 and ids.shape == (4096,) and log_q.dtype == torch.float32 and log_q.shape == (4096,)
    assert int(ids.min()) >= 1 and int(ids.max()) <= 1000
    assert torch.allclose(log_q, torch.full((4096,), math.log(4096 / 1000)))
    assert len(torch.unique(ids)) > 900                         # uniform over the catalog: nearly every item drawn


def test_sample_negatives_by_counts_on_cpu():
    import torch
    import srfrd_amd
    n = 50
    counts = torch.zeros(n + 1)
    counts[0] = 1e9                                             # the padding id: ignored
    counts[1:11] = torch.arange(1, 11, dtype=torch.float32)     # items 11..50 never occur
    for alpha in (1.0, 0.5):
        g = torch.Generator().manual_seed(1)
        num = 20_000
        ids, log_q = srfrd_amd.sample_negatives(n, num, counts=counts, alpha=alpha, generator=g, device="cpu")
        assert int(ids.min()) >= 1 and int(ids.max()) <= 10
        w = counts[1:11].double() ** alpha
        q = w / w.sum()
        assert torch.allclose(log_q.double(), torch.log(num * q[ids - 1]), atol=1e-6)
        freq = torch.bincount(ids, minlength=n + 1)[1:11].double() / num
        assert float((freq - q).abs().max()) < 0.02
    with pytest.raises(ValueError):
        srfrd_amd.sample_negatives(n, 10, counts=torch.ones(n), device="cpu")
    with pytest.raises(ValueError):
        srfrd_amd.sample_negatives(n, 10, counts=torch.zeros(n + 1), device="cpu")
