"""CPU-only: srfrd_table_reduce_mixed and its workspace query are declared, exported and typed, the query is the documented
formula, every documented refusal is a return code made before a launch; the fp64 reference of tests/token_trainer_refs.py
is anchored to a brute-force sum; the index audit passes on every shape the GPU files run; FusedTrainer refuses the
token-negatives losses' bad arguments at construction."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import token_trainer_refs as R

E_ARG = -1
INT_MAX = 2 ** 31 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def test_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    for name, n_args in (("srfrd_table_reduce_mixed", 14), ("srfrd_table_reduce_mixed_workspace_floats", 2)):
        assert name in header_symbols()
        assert name in _lib.SIGNATURES
        assert hasattr(C.CDLL(_lib.LIB_PATH), name)
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert _lib.SIGNATURES["srfrd_table_reduce_mixed_workspace_floats"][0] is C.c_int64
    assert set(header_symbols()) == set(_lib.SIGNATURES)       # (test_abi.py's agreement, with the two new names in it)
    assert _lib.TNEG_SPLIT_ROWS == R.SEG


def test_workspace_query_is_the_formula(lib):
    q = lib.srfrd_table_reduce_mixed_workspace_floats
    for n in (1, 255, 256, 257, 769, 2100, 21_440, 512 * 50 * 66, INT_MAX):
        for d in (1, 45, 50, 64):
            assert q(n, d) == R.ws_floats(n, d), (n, d)
            assert q(n, d) % 64 == 0 and q(n, d) >= 2 * (-(-n // 256)) * d
    for n, d in ((0, 50), (-1, 50), (INT_MAX + 1, 50), (100, 0), (100, -3), (100, 65)):
        assert q(n, d) == 0, (n, d)


def _call(lib, keys=True, order=True, n=100, rows=True, n_rows=10, coef=True, hidden=True, d_out=50, rpt=3, d_item=50,
          grad=True, ws=True, ws_floats=None):
    p = lambda on: _d() if on else None                         # noqa: E731
    if ws_floats is None:
        ws_floats = R.ws_floats(max(n, 1), max(1, min(d_item, 64)))
    return lib.srfrd_table_reduce_mixed(p(keys), p(order), n, p(rows), n_rows, p(coef), p(hidden), d_out, rpt, d_item, p(grad),
                                        p(ws), ws_floats, None)


@pytest.mark.parametrize("kw", [
    dict(keys=False), dict(order=False), dict(grad=False), dict(ws=False),
    dict(rows=False),                                           # rows NULL while n_rows > 0
    dict(coef=False), dict(hidden=False),                       # NULL while n > n_rows
    dict(n=0), dict(n=-5), dict(n=INT_MAX + 1, ws_floats=2 ** 40),
    dict(n_rows=-1), dict(n_rows=101),
    dict(rpt=0), dict(rpt=-2),
    dict(d_item=0, d_out=50), dict(d_item=65, d_out=80), dict(d_item=50, d_out=49),
    dict(ws_floats=R.ws_floats(100, 50) - 1), dict(ws_floats=0), dict(n=257, ws_floats=R.ws_floats(257, 50) - 1),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals_are_return_codes(lib, kw):
    assert _call(lib, **kw) == E_ARG


def test_null_sources_are_refused_only_where_they_would_be_read(lib):
    """rows may be NULL with n_rows == 0 and coef / hidden with n == n_rows: those calls get past the pointer checks (they
    are refused here for their workspace, one float short, so that nothing is launched)"""
    short = R.ws_floats(100, 50) - 1
    assert _call(lib, rows=False, n_rows=0, ws_floats=short) == E_ARG
    assert _call(lib, coef=False, hidden=False, n_rows=100, ws_floats=short) == E_ARG
    assert _call(lib, rows=False, n_rows=1) == E_ARG
    assert _call(lib, coef=False, n_rows=99) == E_ARG
    assert _call(lib, hidden=False, n_rows=99) == E_ARG


@pytest.mark.parametrize("case", R.REDUCE_CASES, ids=repr)
def test_reference_is_anchored_and_indices_are_in_range(case):
    a = case.inputs()
    G, m, S = R.mixed_reduce_ref(a["keys"], a["rows"], a["coef"], a["hidden"], case.rpt, case.d_item, a["n_items"])
    terms = R.terms_of(a["keys"], a["rows"], a["coef"], a["hidden"], case.rpt, case.d_item)
    brute = np.zeros_like(G)
    live = a["keys"] > 0
    np.add.at(brute, a["keys"][live], terms[live])
    assert np.all(np.abs(G - brute) <= 1e-13 * S)
    count = np.bincount(a["keys"][live], minlength=a["n_items"] + 1)
    assert np.array_equal(m, count)
    assert np.all(S[m == 0] == 0) and np.all(G[0] == 0)
    segs, _ = R.audit_indices(a["keys"], case.n_rows, case.rpt, case.T, a["n_items"], case.d_item, R.ws_floats(case.n, case.d_item))
    assert segs == -(-case.n // R.SEG)


def test_shape_list_covers_the_issue():
    cs = R.REDUCE_CASES
    assert {c.d_item for c in cs} == {1, 50, 64}
    assert {c.d_out - c.d_item for c in cs} == {0, 5}
    assert {c.rpt for c in cs} == {1, 2, 17}
    assert {c.n_rows for c in cs} >= {0, 1, 37, 300}
    assert {c.n for c in cs} >= {1, 255, 256, 257, 769, 2100}
    assert {c.hist for c in cs} == {"one", "zero", "boundary", "straddle", "catalog8", "distinct"}
    assert any(c.n == c.n_rows for c in cs) and any(c.n_rows == 0 for c in cs)
    assert any(c.hist == "one" and c.n >= 3 * R.SEG for c in cs)
    # the straddle really straddles: item 5's full rows end segment 0, its rank-1 rows start segment 1
    c = next(c for c in cs if c.hist == "straddle")
    keys, _ = c.keys()
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    assert sk[R.SEG - 1] == 5 and sk[R.SEG] == 5 and order[R.SEG - 1] < c.n_rows <= order[R.SEG]
    c = next(c for c in cs if c.hist == "boundary")
    sk = np.sort(c.keys()[0])
    assert sk[R.SEG - 1] == 1 and sk[R.SEG] != 1 and sk[0] == 1


@pytest.mark.parametrize("B, L, K, n_items", R.TRAINER_SHAPES)
def test_index_audit_on_the_train_steps_key_list(B, L, K, n_items):
    """the sizes FusedTrainer's step rests on: a list of T (2 + K) entries, T of them full rows, 1 + K rank-1 rows per
    token, a workspace of max(srfrd_tneg_workspace_floats, the mixed query)"""
    rs = np.random.RandomState(B + K)
    T = B * L
    inp = rs.randint(0, n_items + 1, (B, L))
    tgt = rs.randint(0, n_items + 1, (B, L)) * (rs.rand(B, L) < 0.7)
    neg = rs.randint(-2, n_items + 3, (B, L, K))                # (ids outside the table are clamped by the kernels)
    keys = R.step_keys(inp, tgt, neg, n_items, True)
    assert keys.shape[0] == T * (2 + K) < 2 ** 31
    R.audit_indices(keys, T, 1 + K, T, n_items, 50, R.ws_floats(T * (2 + K), 50))
    assert R.ws_floats(T * (2 + K), 50) > R.ws_floats(T * (1 + K), 50) - 64


def _model_cpu(kind="SASRec", n_items=300, L=20, d=50):
    import srfrd_amd
    if kind == "SRFRN":
        return srfrd_amd.SRFRN(n_items, L, 45, 5, 0.0, 2, 1, "cpu")
    return srfrd_amd.SASRec(n_items, L, d, 0.0, 2, 1, "cpu")


@pytest.mark.parametrize("kw, match", [
    (dict(loss="token_softmax", num_negatives=0), "num_negatives"),
    (dict(loss="gbce", num_negatives=-4), "num_negatives"),
    (dict(loss="gbce", num_negatives=4, gbce_beta=-0.5), "gbce_beta"),
    (dict(loss="gbce", num_negatives=4, gbce_beta=float("nan")), "gbce_beta"),
    (dict(loss="token_softmax", num_negatives=4, gbce_beta=float("inf")), "gbce_beta"),
    (dict(loss="token_softmax", num_negatives=4, neg_counts=torch.ones(301)), "sampler owns the distribution"),
    (dict(loss="gbce", num_negatives=4, neg_counts=torch.ones(301)), "sampler owns the distribution"),
    (dict(loss="token_softmax", num_negatives=2 ** 25), r"K = 33554432.*2\^31"),
    (dict(loss="tneg", num_negatives=4), "loss must be one of"),
])
def test_constructor_refusals(lib, kw, match):
    import srfrd_amd
    with pytest.raises(ValueError, match=match):
        srfrd_amd.FusedTrainer(_model_cpu(), 4, 20, **kw)


def test_gbce_refuses_srfrn_with_the_module_methods_message(lib):
    import srfrd_amd
    with pytest.raises(ValueError, match="objective='gbce' is not built for SRFRN"):
        srfrd_amd.FusedTrainer(_model_cpu("SRFRN"), 4, 20, loss="gbce", num_negatives=4)


@pytest.mark.parametrize("loss", ["token_softmax", "gbce"])
def test_wide_hidden_and_bf16_table_are_refused(lib, loss):
    import srfrd_amd
    with pytest.raises(ValueError, match="hidden width"):
        srfrd_amd.FusedTrainer(_model_cpu(d=72), 4, 20, loss=loss, num_negatives=4)
    m = _model_cpu()
    m._table16 = torch.zeros(1, dtype=torch.int16)              # what use_bf16_table() leaves: bf16_table is True
    assert m.bf16_table
    with pytest.raises(ValueError, match="fp32 item table"):
        srfrd_amd.FusedTrainer(m, 4, 20, loss=loss, num_negatives=4)


_DP_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
import srfrd_amd
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], world_size=1, rank=0)
m = srfrd_amd.SASRec(300, 20, 50, 0.0, 2, 1, "cpu")
for loss in ("token_softmax", "gbce"):
    try:
        srfrd_amd.FusedTrainer(m, 4, 20, loss=loss, num_negatives=4)
    except ValueError as e:
        assert "single rank" in str(e), e
    else:
        raise SystemExit("not refused: " + loss)
dist.destroy_process_group()
print("refused")
"""


def test_data_parallel_is_refused(lib):
    """a forced exchange in a group of one takes the data-parallel step: the token-negatives losses refuse it"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, SRFRD_FORCE_EXCHANGE="1")
    r = subprocess.run([sys.executable, "-c", _DP_SCRIPT, ROOT, str(port)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
