"""CPU-only: the device-side shared-negative sampler (srfrd_shared_negatives) is declared, exported and typed and refuses bad
arguments before anything touches a GPU; the host alias-table builder reproduces the sampling distribution; FusedTrainer's
cross-entropy arguments are refused at construction where that needs no GPU; the encoder plan of the cross-entropy step
still runs the ragged pair at seq_len 50."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def test_symbol_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    assert "srfrd_shared_negatives" in header_symbols()
    assert "srfrd_shared_negatives" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "srfrd_shared_negatives")
    assert len(_lib.SIGNATURES["srfrd_shared_negatives"][1]) == 9


def test_argument_errors_are_return_codes(lib):
    f = lib.srfrd_shared_negatives
    assert f(None, 100, 8, None, None, None, _d(), _d(), None) == E_ARG            # no state
    assert f(_d(), 100, 8, None, None, None, None, _d(), None) == E_ARG            # no ids output
    assert f(_d(), 100, 8, None, None, None, _d(), None, None) == E_ARG            # no log_q output
    for K in (0, -3):
        assert f(_d(), 100, K, None, None, None, _d(), _d(), None) == E_ARG
    for n in (0, -1):
        assert f(_d(), n, 8, None, None, None, _d(), _d(), None) == E_ARG
    assert f(_d(), 100, 8, _d(), None, _d(), _d(), _d(), None) == E_ARG            # alias_prob without alias_idx
    assert f(_d(), 100, 8, None, _d(), _d(), _d(), _d(), None) == E_ARG            # alias_idx without alias_prob
    assert f(_d(), 100, 8, _d(), _d(), None, _d(), _d(), None) == E_ARG            # an alias table needs item_log_q


def _q_of_table(prob, alias):
    """the distribution an alias table draws: bucket b uniform, kept with prob[b], else alias[b]"""
    n = prob.size
    p = prob.astype(np.float64)
    q = p.copy()
    np.add.at(q, alias.astype(np.int64), 1.0 - p)
    return q / n


@pytest.mark.parametrize("case", ["skewed", "uniform", "one_item", "zero_heavy"])
def test_alias_table_reproduces_q(case):
    from srfrd_amd.sampler import alias_table, negative_q
    rs = np.random.RandomState(3)
    n = {"skewed": 5000, "uniform": 300, "one_item": 1, "zero_heavy": 2000}[case]
    counts = np.zeros(n + 1)
    if case == "skewed":
        counts[1:] = rs.pareto(1.2, n) * 100
    elif case == "uniform":
        counts[1:] = 7.0
    elif case == "one_item":
        counts[1] = 3.0
    else:
        counts[1 + rs.choice(n, 5, replace=False)] = [1.0, 2.0, 1e6, 3.0, 0.5]
    counts[0] = 1e9                                            # the padding id's entry is ignored
    q = negative_q(n, torch.from_numpy(counts), 0.75)
    assert abs(q.sum() - 1.0) < 1e-12
    prob, alias = alias_table(q)
    assert prob.dtype == np.float32 and alias.dtype == np.int32 and prob.shape == alias.shape == (n,)
    assert alias.min() >= 0 and alias.max() < n and prob.min() >= 0.0 and prob.max() <= 1.0
    rec = _q_of_table(prob, alias)
    # fp32 rounding of each stored probability: at most 2^-24 per bucket and term, divided by n
    assert np.abs(rec - q).max() <= 4 * 2.0 ** -24 / n + 1e-15, np.abs(rec - q).max()
    assert np.all(rec[q == 0] <= 2.0 ** -24 / n)
    if case == "uniform":
        assert np.all(prob == 1.0)


def _model_cpu(n_items=300, L=20, d=50):
    import srfrd_amd
    return srfrd_amd.SASRec(n_items, L, d, 0.0, 2, 1, "cpu")


@pytest.mark.parametrize("kw, match", [
    (dict(loss="xent"), "loss must be one of"),
    (dict(loss="sampled_softmax", num_negatives=0), "num_negatives"),
    (dict(loss="sampled_softmax", num_negatives=-4), "num_negatives"),
    (dict(loss="sampled_softmax", neg_counts=torch.ones(300)), "shape"),
    (dict(loss="sampled_softmax", neg_counts=torch.ones(2, 301)), "shape"),
    (dict(loss="sampled_softmax", neg_counts=torch.zeros(301)), "positive"),
    (dict(loss="sampled_softmax", neg_counts=-torch.ones(301)), "positive"),
    (dict(loss="softmax", neg_counts=torch.ones(301)), "sampled_softmax"),
])
def test_constructor_refusals(lib, kw, match):
    import srfrd_amd
    with pytest.raises(ValueError, match=match):
        srfrd_amd.FusedTrainer(_model_cpu(), 4, 20, **kw)


@pytest.mark.parametrize("loss", ["softmax", "sampled_softmax"])
def test_wide_hidden_is_refused(lib, loss):
    import srfrd_amd
    with pytest.raises(ValueError, match="hidden width"):
        srfrd_amd.FusedTrainer(_model_cpu(d=72), 4, 20, loss=loss)


_DP_SCRIPT = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
import srfrd_amd
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], world_size=1, rank=0)
m = srfrd_amd.SASRec(300, 20, 50, 0.0, 2, 1, "cpu")
for loss in ("softmax", "sampled_softmax"):
    try:
        srfrd_amd.FusedTrainer(m, 4, 20, loss=loss)
    except ValueError as e:
        assert "single rank" in str(e), e
    else:
        raise SystemExit("not refused: " + loss)
dist.destroy_process_group()
print("refused")
"""


def test_data_parallel_is_refused(lib):
    """a forced exchange in a group of one takes the data-parallel step: the cross-entropy losses refuse it"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, SRFRD_FORCE_EXCHANGE="1")
    r = subprocess.run([sys.executable, "-c", _DP_SCRIPT, ROOT, str(port)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("kind, d, d_fake, n_labels", [("SASRec", 50, 0, 0), ("SRFR", 45, 5, 0), ("SRFRN", 45, 5, 0),
                                                       ("SRFU_B", 50, 0, 3)])
def test_ce_step_plan_runs_the_ragged_pair_at_seq_len_50(lib, kind, d, d_fake, n_labels):
    from srfrd_amd import _lib
    lay = _lib.make_layout(kind, 50_000, 50, d, d_fake, n_labels, 2, 1)
    for mode in (_lib.PLAN_CKPT, _lib.PLAN_CKPT | _lib.PLAN_DROPOUT):
        (fwd, _), (bwd, _) = _lib.encoder_plan(lay, 512, 50, mode)
        assert fwd.startswith("srfrd::encoder_fwd_ragged_kernel<"), fwd
        assert bwd.startswith("srfrd::encoder_bwd_ragged_kernel<"), bwd
