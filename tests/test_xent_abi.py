"""CPU-only: the full-catalog cross-entropy entry points (srfrd_xent_workspace_floats, srfrd_xent_fwd, srfrd_xent_bwd) are
declared, exported and typed; the workspace query sizes both calls; arguments they refuse are refused before anything
touches a GPU (null pointers -> SRFRD_E_ARG, a bf16-table layout or hidden width > 64 -> SRFRD_E_UNSUPPORTED)."""
import ctypes as C

import pytest

NEW = ("srfrd_xent_workspace_floats", "srfrd_xent_fwd", "srfrd_xent_bwd")
E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def _fwd(lib, lay, B=4, L=20, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in ("table", "hidden", "targets", "token_loss", "lse", "stats", "workspace")}
    return lib.srfrd_xent_fwd(C.byref(lay), a["table"], a["hidden"], a["targets"], B, L, a["token_loss"], a["lse"], a["stats"],
                              a["workspace"], ws_floats, None)


def _bwd(lib, lay, B=4, L=20, ws_floats=1 << 40, **null):
    a = {k: (None if k in null else _d()) for k in ("table", "hidden", "targets", "lse", "d_token_loss", "d_hidden", "grad_table",
                                                     "workspace")}
    return lib.srfrd_xent_bwd(C.byref(lay), a["table"], a["hidden"], a["targets"], a["lse"], a["d_token_loss"], B, L, a["d_hidden"],
                              a["grad_table"], 0, a["workspace"], ws_floats, None)


def test_new_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), s)


def test_workspace_floats(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 50_000, 50, 50, 0, 0, 2, 1)
    n = lib.srfrd_xent_workspace_floats(C.byref(lay), 512, 50)
    T = 512 * 50
    assert n >= 2 * T + 2 * T          # token list + target logits + at least one split of (max, sum) partials
    assert n >= T * 50                 # the backward's d_hidden partials (one split at least)
    big = _lib.make_layout("SASRec", 1_000_000, 200, 50, 0, 0, 2, 1)
    assert lib.srfrd_xent_workspace_floats(C.byref(big), 512, 200) >= lib.srfrd_xent_workspace_floats(C.byref(big), 64, 200) > 0
    assert lib.srfrd_xent_workspace_floats(C.byref(lay), 0, 50) == 0
    assert lib.srfrd_xent_workspace_floats(None, 4, 20) == 0


def test_null_pointers_and_sizes_are_refused(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SRFRN", 100, 20, 45, 5, 0, 2, 1)
    for k in ("table", "hidden", "targets", "token_loss", "lse", "stats", "workspace"):
        assert _fwd(lib, lay, **{k: 1}) == E_ARG, k
    for k in ("table", "hidden", "targets", "lse", "d_token_loss", "d_hidden", "grad_table", "workspace"):
        assert _bwd(lib, lay, **{k: 1}) == E_ARG, k
    assert _fwd(lib, lay, B=0) == E_ARG and _bwd(lib, lay, L=0) == E_ARG
    need = lib.srfrd_xent_workspace_floats(C.byref(lay), 4, 20)
    assert _fwd(lib, lay, ws_floats=need - 1) == E_ARG and _bwd(lib, lay, ws_floats=need - 1) == E_ARG
    assert lib.srfrd_xent_fwd(None, _d(), _d(), _d(), 4, 20, _d(), _d(), _d(), _d(), 1 << 40, None) == E_ARG


def test_unsupported_layouts(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    lay.table_bf16 = 1
    assert _fwd(lib, lay) == E_UNSUPPORTED and _bwd(lib, lay) == E_UNSUPPORTED
    wide = _lib.make_layout("SASRec", 100, 20, 72, 0, 0, 2, 1)
    assert _fwd(lib, wide) == E_UNSUPPORTED and _bwd(lib, wide) == E_UNSUPPORTED
    assert lib.srfrd_xent_workspace_floats(C.byref(wide), 4, 20) == 0


def test_ops_registered_with_fake_impls():
    import torch
    import srfrd_amd  # noqa: F401
    from srfrd_amd import ops
    assert "xent_fwd" in ops.OPS and "xent_bwd" in ops.OPS
    assert torch.ops.srfrd.xent_fwd.default._schema.name == "srfrd::xent_fwd"
    assert torch.ops.srfrd.xent_bwd.default._schema.name == "srfrd::xent_bwd"
    assert hasattr(srfrd_amd.SASRec, "full_catalog_loss")
