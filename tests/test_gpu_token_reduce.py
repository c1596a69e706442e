"""srfrd_table_reduce_mixed alone, at every shape of tests/token_trainer_refs.REDUCE_CASES (the list whose indices
tests/test_token_trainer_abi.py audits on the CPU): values against the fp64 reference, untouched rows, and its bits against
itself, against srfrd_table_reduce_rank1 and against the same rows expressed the other way."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import token_trainer_refs as R

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sorted(keys):
    return torch.sort(keys, stable=True)


def _mixed(lib, keys, rows, coef, hidden, d_out, rpt, d_item, n_items):
    """one call on a sentinel-filled table and a NaN-filled workspace of exactly the queried size -> the table (host)"""
    n, n_rows = keys.numel(), 0 if rows is None else rows.shape[0]
    skeys, order = _sorted(keys)
    ws = torch.full((int(lib.srfrd_table_reduce_mixed_workspace_floats(n, d_item)),), float("nan"), device="cuda")
    assert ws.numel() == R.ws_floats(n, d_item)
    G = torch.full((n_items + 1, d_item), SENTINEL, device="cuda")
    rc = lib.srfrd_table_reduce_mixed(_p(skeys), _p(order), n, _p(rows), n_rows, _p(coef), _p(hidden), d_out, rpt, d_item, _p(G),
                                      _p(ws), ws.numel(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return G.cpu()


def _device(case):
    a = case.inputs()
    dev = {k: torch.from_numpy(np.ascontiguousarray(a[k])).cuda() for k in ("keys", "rows", "coef", "hidden")}
    rows = dev["rows"] if case.n_rows else None
    coef, hidden = (dev["coef"], dev["hidden"]) if case.n > case.n_rows else (None, None)
    return a, dev["keys"], rows, coef, hidden


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=repr)
def test_values_untouched_rows_and_bits(lib, case):
    a, keys, rows, coef, hidden = _device(case)
    d, n_items = case.d_item, a["n_items"]
    R.audit_indices(a["keys"], case.n_rows, case.rpt, case.T, n_items, d, R.ws_floats(case.n, d))
    G = _mixed(lib, keys, rows, coef, hidden, case.d_out, case.rpt, d, n_items)
    ref, m, S = R.mixed_reduce_ref(a["keys"], a["rows"], a["coef"], a["hidden"], case.rpt, d, n_items)
    got = G.double().numpy()
    touched = m > 0
    # a sequential fp32 fused multiply-add sum of m terms: |error| <= (m + 1) 2^-24 sum |term| (derived, not measured)
    bound = 1.01 * (m[:, None] + 1) * R.U24 * S
    err = np.abs(got - ref)
    worst = float((err[touched] / np.maximum(bound[touched], 1e-300)).max()) if touched.any() else 0.0
    print(f"{case}: touched rows {int(touched.sum())}, worst error / bound {worst:.3f}")
    assert np.all(err[touched] <= bound[touched]), worst
    assert np.all(got[~touched] == SENTINEL)                    # rows without a contribution, row 0 among them
    if case.hist == "zero":
        assert not touched.any()
    # the same call again: the same bits
    G2 = _mixed(lib, keys, rows, coef, hidden, case.d_out, case.rpt, d, n_items)
    assert torch.equal(G, G2)
    if case.n_rows == 0:
        # ... and the bits of srfrd_table_reduce_rank1
        skeys, order = _sorted(keys)
        ws = torch.full((R.ws_floats(case.n, d),), float("nan"), device="cuda")
        G1 = torch.full((n_items + 1, d), SENTINEL, device="cuda")
        rc = lib.srfrd_table_reduce_rank1(_p(skeys), _p(order), _p(coef), _p(hidden), case.d_out, case.rpt, case.n, d, _p(G1),
                                          _p(ws), ws.numel(), _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(G, G1.cpu())
    if case.n == case.n_rows:
        # only full rows, coef and hidden NULL: the bits of the same rows as rank-1 rows, coefficient 1 over hidden = rows
        ones = torch.ones(case.n, device="cuda")
        Gr = _mixed(lib, keys, None, ones, rows, d, 1, d, n_items)
        assert torch.equal(G, Gr)


def test_helper_checks_the_sizes_the_kernel_indexes_by(lib):
    """loss_heads.table_mixed refuses a hidden tensor with too few rows, a key list of another length and a workspace below
    the query before it launches anything, and gives the entry point's result otherwise"""
    from srfrd_amd import _lib, loss_heads
    case = next(c for c in R.REDUCE_CASES if c.name == "n769_r37_d50+5_t2_catalog8")
    a, keys, rows, coef, hidden = _device(case)
    lay = _lib.make_layout("SRFRN", a["n_items"], 20, 50, 5, 0, 2, 1)
    assert (lay.d_item, lay.d_out) == (50, 55)
    ws = torch.zeros(R.ws_floats(case.n, 50), device="cuda")
    G = torch.full((a["n_items"] + 1, 50), SENTINEL, device="cuda")
    K = case.rpt - 1
    with pytest.raises(ValueError, match="hidden rows"):
        loss_heads.table_mixed(lay, hidden[:-1].contiguous(), K, rows, coef, keys, ws, G)
    with pytest.raises(ValueError, match="keys"):
        loss_heads.table_mixed(lay, hidden, K, rows, coef, keys[:-1].contiguous(), ws, G)
    with pytest.raises(ValueError, match="workspace"):
        loss_heads.table_mixed(lay, hidden, K, rows, coef, keys, ws[:-64], G)
    assert float(G.min()) == float(G.max()) == SENTINEL
    loss_heads.table_mixed(lay, hidden, K, rows, coef, keys, ws, G)
    torch.cuda.synchronize()
    assert torch.equal(G.cpu(), _mixed(lib, keys, rows, coef, hidden, 55, case.rpt, 50, a["n_items"]))
    # a stable sort the caller made already (FusedTrainer sorts between its two graphs)
    G.fill_(SENTINEL)
    loss_heads.table_mixed(lay, hidden, K, rows, coef, keys, ws, G, sorted_pair=_sorted(keys))
    torch.cuda.synchronize()
    assert torch.equal(G.cpu(), _mixed(lib, keys, rows, coef, hidden, 55, case.rpt, 50, a["n_items"]))
    with pytest.raises(ValueError, match="sorted_pair"):
        loss_heads.table_mixed(lay, hidden, K, rows, coef, keys, ws, G, sorted_pair=tuple(t[:-1] for t in _sorted(keys)))
