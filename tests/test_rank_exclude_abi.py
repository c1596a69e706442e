"""CPU-only: the exclusion-masked ranking entry points (srfrd_logits_topk_excl, srfrd_target_rank,
srfrd_excl_workspace_bytes) are declared, exported and typed; their fake impls give the right shapes; malformed arguments
that need no device read are refused before anything touches a GPU."""
import ctypes as C

import pytest
import torch

NEW = ("srfrd_excl_workspace_bytes", "srfrd_logits_topk_excl", "srfrd_target_rank")
E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def test_new_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    syms = header_symbols()
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), s)


def test_excl_workspace_bytes(lib):
    from srfrd_amd import _lib
    assert lib.srfrd_excl_workspace_bytes(512, 200, 1_000_001) >= 512 * 200 * 4 + 512 * 3907 * 4
    assert lib.srfrd_excl_workspace_bytes(4, 0, 100) > 0
    assert lib.srfrd_excl_workspace_bytes(4, _lib.EXCL_CAP + 1, 100) == 0
    assert lib.srfrd_excl_workspace_bytes(0, 10, 100) == 0


def _dummy(n=64):
    return C.c_void_p(n)           # never dereferenced: the calls below must fail on the host


def _topk(lib, lay, B=4, k=10, excl_ptr=_dummy(), excl_items=_dummy(), max_row=8, xws=_dummy()):
    d = _dummy()
    return lib.srfrd_logits_topk_excl(C.byref(lay), d, d, d, B, 1, 0, 101, 1, None, k, excl_ptr, excl_items, max_row, d, d, d,
                                      xws, None)


def _rank(lib, lay, B=4, cut_k=10, excl_ptr=_dummy(), excl_items=_dummy(), max_row=8, targets=_dummy()):
    d = _dummy()
    return lib.srfrd_target_rank(C.byref(lay), d, d, d, B, 1, 0, 101, 1, None, targets, excl_ptr, excl_items, max_row, cut_k, d,
                                 None, d, None)


def test_malformed_arguments_are_refused_without_a_gpu(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    assert _topk(lib, lay, excl_items=None) == E_ARG           # a CSR without its item array
    assert _topk(lib, lay, xws=None) == E_ARG                   # no exclusion workspace
    assert _topk(lib, lay, B=0) == E_ARG
    assert _topk(lib, lay, k=65) == E_ARG
    assert _topk(lib, lay, k=0) == E_ARG
    assert _topk(lib, lay, max_row=-1) == E_ARG
    assert _topk(lib, lay, max_row=_lib.EXCL_CAP + 1) == E_UNSUPPORTED
    assert _rank(lib, lay, excl_items=None) == E_ARG
    assert _rank(lib, lay, B=0) == E_ARG
    assert _rank(lib, lay, B=-3) == E_ARG
    assert _rank(lib, lay, cut_k=0) == E_ARG
    assert _rank(lib, lay, targets=None) == E_ARG
    assert _rank(lib, lay, max_row=_lib.EXCL_CAP + 1) == E_UNSUPPORTED


def test_fake_impls_give_shapes_and_dtypes(lib):
    import srfrd_amd
    from srfrd_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    key = ops.register_model(m)
    with FakeTensorMode():
        h = torch.empty(6, 1, 50, device="meta")
        xp = torch.empty(7, dtype=torch.int64, device="meta")
        xi = torch.empty(11, dtype=torch.int32, device="meta")
        t = torch.empty(6, dtype=torch.int64, device="meta")
        idx, val = torch.ops.srfrd.logits_topk_excl(h, None, key, 0, 101, 7, True, xp, xi, 3)
        r = torch.ops.srfrd.target_rank(h, None, t, key, 0, 101, True, xp, xi, 3)
    assert tuple(idx.shape) == (6, 7) and idx.dtype == torch.int64
    assert tuple(val.shape) == (6, 7) and val.dtype == torch.float32
    assert tuple(r.shape) == (6,) and r.dtype == torch.int32


def test_exclusion_arguments_normalise_to_one_csr():
    from srfrd_amd import ops
    inp = torch.tensor([[0, 0, 3, 4], [5, 6, 7, 8], [0, 0, 0, 0]])
    p, i, mr = ops.excl_csr("input", inp, 3, torch.device("cpu"))
    assert p.tolist() == [0, 2, 6, 6] and i.tolist() == [3, 4, 5, 6, 7, 8] and mr == 4 and i.dtype == torch.int32
    p, i, mr = ops.excl_csr([torch.tensor([9, 9, 1]), torch.tensor([], dtype=torch.int64), torch.tensor([2])], None, 3,
                            torch.device("cpu"))
    assert p.tolist() == [0, 3, 3, 4] and i.tolist() == [9, 9, 1, 2] and mr == 3
    p2, i2, mr2 = ops.excl_csr((p, i), None, 3, torch.device("cpu"))
    assert p2.tolist() == p.tolist() and i2.tolist() == i.tolist() and mr2 == 3
    assert ops.excl_csr(None, inp, 3, torch.device("cpu")) == (None, None, 0)
    with pytest.raises(ValueError):
        ops.excl_csr((torch.tensor([0, 2, 1, 3]), i), None, 3, torch.device("cpu"))       # decreasing pointer
    with pytest.raises(ValueError):
        ops.excl_csr([torch.tensor([1])], None, 3, torch.device("cpu"))                    # one row for three users
