"""CPU-only: the learning-rate schedule, gradient-norm clipping and decoupled weight decay of the fused step, as far as no GPU is
needed: ``srfrd_amd.lr_at`` against torch's LambdaLR, the refusals of ``_optim_config`` and of the four new entry points
(srfrd_step_begin_sched, srfrd_grad_norm, srfrd_adamw_step, srfrd_adamw_pack_step; the pointers are never dereferenced), and
the agreement of header, signature table and exported symbols."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

E_ARG, E_UNSUPPORTED = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"srfrd_step_begin_sched": 3, "srfrd_grad_norm": 7, "srfrd_adamw_step": 17, "srfrd_adamw_pack_step": 16}
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced (64: 16-byte aligned, as srfrd_grad_norm asks of the gradient)


# ---- lr_at --------------------------------------------------------------------------------------------------------------
def _factor(kind, w, total, r):
    """the closed form of include/srfrd_hip.h as a LambdaLR multiplier (LambdaLR's epoch e is the 0-based step: t = e + 1)"""
    def f(e):
        t = e + 1
        if t <= w:
            return t / w
        if kind == "constant":
            return 1.0
        u = min(1.0, (t - w) / max(1, total - w))
        return 1.0 - (1.0 - r) * u if kind == "linear" else r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u))
    return f


@pytest.mark.parametrize("w", [0, 1, 4])
@pytest.mark.parametrize("kind", ["constant", "linear", "cosine"])
def test_lr_at_is_the_lambda_lr_of_the_closed_form(kind, w):
    from srfrd_amd import lr_at
    lr, total, r = 3e-3, 11, 0.1
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _factor(kind, w, total, r))
    for t in range(1, total + 6):
        want = opt.param_groups[0]["lr"]                 # the rate step t runs at
        got = lr_at(t, lr, kind, w, total, r)
        assert got == want, (t, got, want)
        opt.step()
        sched.step()
    # the end points: f(w) = 1, f(total) = r, and r from there on
    if w:
        assert lr_at(w, lr, kind, w, total, r) == lr
    if kind != "constant":
        for t in (total, total + 1, total + 5, 1 << 20):
            assert abs(lr_at(t, lr, kind, w, total, r) - r * lr) <= 2.0 ** -52 * lr
    else:
        assert lr_at(total + 5, lr, kind, w, None, r) == lr


def test_lr_at_refuses_what_it_cannot_answer():
    from srfrd_amd import lr_at
    with pytest.raises(ValueError, match="lr_schedule"):
        lr_at(1, 1e-3, "step")
    with pytest.raises(ValueError, match="total_steps"):
        lr_at(1, 1e-3, "cosine")
    with pytest.raises(ValueError, match="from 1"):
        lr_at(0, 1e-3)


# ---- _optim_config ------------------------------------------------------------------------------------------------------
def test_optim_config_neutral_is_none():
    from srfrd_amd.trainer import _optim_config
    assert _optim_config(1e-3, (0.9, 0.98)) == (None, None)
    assert _optim_config(1e-3, (0.9, 0.98), 0.0, None, "constant", 0, None, 0.5) == (None, None)
    assert _optim_config(1e-3, (0.9, 0.98), total_steps=100) == (None, None)


def test_optim_config_fills_the_struct():
    from srfrd_amd import _lib
    from srfrd_amd.trainer import _optim_config
    o, mx = _optim_config(2e-3, (0.9, 0.98), 0.1, 0.5, "cosine", 3, 10, 0.25)
    assert (o.lr, o.beta1, o.beta2, o.weight_decay, o.final_ratio) == (2e-3, 0.9, 0.98, 0.1, 0.25)
    assert (o.warmup_steps, o.total_steps, o.schedule, mx) == (3, 10, _lib.SCHEDULES["cosine"], 0.5)
    assert C.sizeof(_lib.OptimOpts) == 64
    for kw in (dict(weight_decay=0.1), dict(max_grad_norm=INF), dict(warmup_steps=1), dict(lr_schedule="linear", total_steps=5)):
        o, mx = _optim_config(1e-3, (0.9, 0.98), **kw)
        assert o is not None and (mx == INF) == ("max_grad_norm" in kw)


@pytest.mark.parametrize("kw, match", [
    (dict(weight_decay=-0.1), "weight_decay"), (dict(weight_decay=NAN), "weight_decay"), (dict(weight_decay=INF), "weight_decay"),
    (dict(max_grad_norm=0.0), "max_grad_norm"), (dict(max_grad_norm=-1.0), "max_grad_norm"), (dict(max_grad_norm=NAN), "max_grad_norm"),
    (dict(warmup_steps=-1), "warmup_steps"), (dict(warmup_steps=1.5), "warmup_steps"),
    (dict(lr_schedule="step"), "lr_schedule"),
    (dict(lr_schedule="linear"), "total_steps"), (dict(lr_schedule="cosine", warmup_steps=5, total_steps=4), "total_steps"),
    (dict(final_lr_ratio=-0.1), "final_lr_ratio"), (dict(final_lr_ratio=1.1), "final_lr_ratio"), (dict(final_lr_ratio=NAN), "final_lr_ratio"),
])
def test_optim_config_refusals(kw, match):
    from srfrd_amd.trainer import _optim_config
    with pytest.raises(ValueError, match=match):
        _optim_config(1e-3, (0.9, 0.98), **kw)


def test_constructor_refuses_before_anything_is_allocated(lib):
    import srfrd_amd
    m = srfrd_amd.SASRec(300, 20, 50, 0.0, 2, 1, "cpu")
    with pytest.raises(ValueError, match="max_grad_norm"):
        srfrd_amd.FusedTrainer(m, 4, 20, max_grad_norm=0.0)
    with pytest.raises(ValueError, match="total_steps"):
        srfrd_amd.FusedTrainer(m, 4, 20, lr_schedule="cosine")


_DP_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch.distributed as dist
from srfrd_amd.trainer import _optim_config
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], world_size=1, rank=0)
assert _optim_config(1e-3, (0.9, 0.98)) == (None, None)              # the neutral options stay welcome
for kw in (dict(weight_decay=0.1), dict(max_grad_norm=1.0), dict(warmup_steps=2), dict(lr_schedule="linear", total_steps=9)):
    try:
        _optim_config(1e-3, (0.9, 0.98), **kw)
    except ValueError as e:
        assert "single rank" in str(e) and "srfrd_pack_weights" in str(e), e
    else:
        raise SystemExit("not refused: " + repr(kw))
dist.destroy_process_group()
print("refused")
"""


def test_a_forced_exchange_refuses_every_option():
    """a forced exchange in a group of one takes the data-parallel step, which has none of the three"""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, SRFRD_FORCE_EXCHANGE="1")
    r = subprocess.run([sys.executable, "-c", _DP_SCRIPT, ROOT, str(port)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import header_symbols
    exported = C.CDLL(_lib.LIB_PATH)
    for name, n_args in NEW.items():
        assert name in header_symbols() and name in _lib.SIGNATURES and hasattr(exported, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
    hdr = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    assert f"#define SRFRD_GRAD_NORM_PARTIALS {_lib.GRAD_NORM_PARTIALS}\n" in hdr
    assert f"#define SRFRD_GRAD_NORM_SHARE {_lib.GRAD_NORM_SHARE}\n" in hdr
    for name, k in _lib.SCHEDULES.items():
        assert f"SRFRD_SCHED_{name.upper()} = {k}" in hdr


def _opts(**kw):
    from srfrd_amd import _lib
    f = dict(lr=1e-3, beta1=0.9, beta2=0.98, weight_decay=0.0, final_ratio=0.0, warmup_steps=0, total_steps=0, schedule=0, reserved=0)
    f.update(kw)
    return _lib.OptimOpts(**f)


BAD_OPTS = [dict(weight_decay=-1e-3), dict(weight_decay=NAN), dict(warmup_steps=-1), dict(schedule=3), dict(schedule=-1),
            dict(schedule=1, warmup_steps=5, total_steps=4), dict(schedule=2, warmup_steps=1, total_steps=0),
            dict(final_ratio=-0.01), dict(final_ratio=1.01), dict(final_ratio=NAN)]


def test_step_begin_sched_refusals(lib):
    f = lib.srfrd_step_begin_sched
    assert f(None, C.byref(_opts()), None) == E_ARG
    assert f(_d(), None, None) == E_ARG
    for bad in BAD_OPTS:
        assert f(_d(), C.byref(_opts(**bad)), None) == E_ARG, bad


def test_grad_norm_refusals(lib):
    f = lib.srfrd_grad_norm
    d = _d()
    assert f(None, 16, None, 1.0, d, d, None) == E_ARG
    assert f(d, 16, None, 1.0, None, d, None) == E_ARG
    assert f(d, 16, None, 1.0, d, None, None) == E_ARG
    for n in (0, -4):
        assert f(d, n, None, 1.0, d, d, None) == E_ARG
    for max_norm in (0.0, -1.0, NAN, -INF):
        assert f(d, 16, None, max_norm, d, d, None) == E_ARG, max_norm
    assert f(_d(68), 16, None, 1.0, d, d, None) == E_ARG                  # the float4 loads need 16-byte alignment


def _adamw(lib, n=16, i0=0, i1=16, param=_d(), state=_d()):
    d = _d()
    return lib.srfrd_adamw_step(param, d, d, d, n, i0, i1, 0, 0.9, 0.98, 1e-8, state, None, None, None, 0, None)


def test_adamw_step_refusals_and_the_empty_slice(lib):
    assert _adamw(lib, i0=2, i1=8) == E_ARG
    assert _adamw(lib, i0=8, i1=4) == E_ARG
    assert _adamw(lib, i0=0, i1=17) == E_ARG
    assert _adamw(lib, i0=-4, i1=8) == E_ARG
    assert _adamw(lib, n=0, i0=0, i1=0) == E_ARG
    assert _adamw(lib, param=None) == E_ARG
    assert _adamw(lib, state=None) == E_ARG
    assert _adamw(lib, n=5, i0=5, i1=5) == 0                               # an empty slice launches nothing
    assert _adamw(lib, n=16, i0=8, i1=8) == 0
    assert _adamw(lib, n=5, i0=6, i1=6) == E_ARG


def _packw(lib, lay, n, n_table_pad, opts, packed=_d()):
    d = _d()
    return lib.srfrd_adamw_pack_step(C.byref(lay), d, d, d, d, n, n_table_pad, n_table_pad, opts, 1e-8, d, None, None, packed,
                                     None, None)


def test_adamw_pack_step_refusals(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    ntp = (lay.n_table + 3) // 4 * 4
    n = (ntp + lay.n_dense + 3) // 4 * 4
    ok = C.byref(_opts(weight_decay=0.1, schedule=1, warmup_steps=2, total_steps=5))
    assert _packw(lib, lay, n, ntp - 2, ok) == E_ARG
    assert _packw(lib, lay, n, -4, ok) == E_ARG
    assert _packw(lib, lay, ntp + lay.n_dense - 1, ntp, ok) == E_ARG
    assert _packw(lib, lay, 0, 0, ok) == E_ARG
    assert _packw(lib, lay, n, ntp, ok, packed=None) == E_ARG
    assert _packw(lib, lay, n, ntp, None) == E_ARG
    for bad in BAD_OPTS:
        assert _packw(lib, lay, n, ntp, C.byref(_opts(**bad))) == E_ARG, bad
    wide = _lib.make_layout("SASRec", 100, 20, 80, 0, 0, 2, 1)
    ntp = (wide.n_table + 3) // 4 * 4
    assert _packw(lib, wide, (ntp + wide.n_dense + 3) // 4 * 4, ntp, ok) == E_UNSUPPORTED


def test_module_level_adamw_refusals():
    import srfrd_amd
    p = [torch.nn.Parameter(torch.zeros(4))]
    for wd in (-0.1, NAN, INF):
        with pytest.raises(ValueError, match="weight_decay"):
            srfrd_amd.AdamW(p, weight_decay=wd)
    with pytest.raises(ValueError, match="amsgrad"):
        srfrd_amd.AdamW(p, amsgrad=True)
    with pytest.raises(ValueError):                    # srfrd_amd.Adam itself keeps refusing a decay
        srfrd_amd.Adam(p, weight_decay=0.1)
    opt = srfrd_amd.AdamW(p, lr=2e-3, weight_decay=0.05)
    g = opt.state_dict()["param_groups"][0]
    assert g["weight_decay"] == 0.05 and g["decoupled_weight_decay"] is True and g["lr"] == 2e-3
    coupled = {"state": {}, "param_groups": [dict(g, decoupled_weight_decay=False)]}
    with pytest.raises(ValueError, match="decoupled"):
        opt.load_state_dict(coupled)
