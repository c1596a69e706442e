"""CPU: the train direction of the encoder's kernel plan (srfrd_encoder_plan_train) and its entry point
(srfrd_encoder_train_sched).

The plan offers the one-launch train kernel exactly where it pairs the ragged seq_len-50 kernels for a call that carries
everything a fused train step computes, on the backward's grid; the entry point refuses what either of the two calls it
replaces refuses (SRFRD_E_ARG), and SRFRD_E_UNSUPPORTED wherever the plan has no train kernel - before anything touches a GPU.
"""
import ctypes as C
import itertools

import pytest

from srfrd_amd import _lib
from tests.test_encoder_plan import LAYOUTS, LENGTHS, MODES, SWITCH_SETS, _layout

P = _lib
E_ARG, E_UNSUPPORTED = -1, -2
TRAIN = P.PLAN_POS | P.PLAN_NEG | P.PLAN_CKPT | P.PLAN_LOSS | P.PLAN_FUSED_BCE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


def _expected_train(lay, B, L, mode, sw):
    (fwd, _), (bwd, bgrid) = _lib.encoder_plan(lay, B, L, mode, sw)
    ragged = fwd.startswith("srfrd::encoder_fwd_ragged_kernel<") and bwd.startswith("srfrd::encoder_bwd_ragged_kernel<")
    if not ragged or (mode & TRAIN) != TRAIN or (mode & P.PLAN_TAPS):
        return "", E_UNSUPPORTED
    targs = bwd[len("srfrd::encoder_bwd_ragged_kernel<"):]          # <K,DI,rmw>: the backward's instantiation and grid
    return "srfrd::encoder_train_ragged_kernel<" + targs, bgrid


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda t: "-".join(map(str, t)))
def test_train_direction_follows_the_ragged_pair(lib, layout):
    lay = _layout(*layout)
    for L, B, (mname, mode), sw in itertools.product(LENGTHS, (7, 300, 512, 513, 1500), MODES.items(), SWITCH_SETS):
        sw_bits = 0 if sw is None else P.SWITCHES[sw]
        got = _lib.encoder_plan_train(lay, B, L, mode, sw_bits)
        assert got == _expected_train(lay, B, L, mode, sw_bits), (layout, L, B, mname, sw)


def test_train_plan_at_the_flagship_shape(lib):
    lay = _layout("SASRec", 50, 0, 0, 1)
    assert _lib.encoder_plan_train(lay, 512, 50, TRAIN | P.PLAN_DROPOUT) == ("srfrd::encoder_train_ragged_kernel<0,50,false>", 512)
    assert _lib.encoder_plan_train(lay, 512, 50, TRAIN) == ("srfrd::encoder_train_ragged_kernel<0,50,false>", 512)
    assert _lib.encoder_plan_train(lay, 1024, 50, TRAIN) == ("srfrd::encoder_train_ragged_kernel<0,50,true>", 512)
    for missing in (P.PLAN_POS, P.PLAN_NEG, P.PLAN_CKPT, P.PLAN_LOSS, P.PLAN_FUSED_BCE):
        assert _lib.encoder_plan_train(lay, 512, 50, TRAIN & ~missing) == ("", E_UNSUPPORTED)
    assert _lib.encoder_plan_train(lay, 512, 50, TRAIN | P.PLAN_TAPS) == ("", E_UNSUPPORTED)
    assert _lib.encoder_plan_train(lay, 512, 50, TRAIN, P.SWITCHES["SRFRD_NO_RAGGED"]) == ("", E_UNSUPPORTED)
    # (the full-rows switch keeps the ragged kernels, computing every row: the train kernel too)
    assert _lib.encoder_plan_train(lay, 512, 50, TRAIN, P.SWITCHES["SRFRD_RAGGED_FULL_ROWS"])[0].startswith("srfrd::encoder_train_ragged")


def test_plan_train_refuses_bad_arguments(lib):
    lay = _layout("SASRec", 50, 0, 0, 1)
    name, grid = C.create_string_buffer(64), C.c_int32(0)
    assert lib.srfrd_encoder_plan_train(None, 8, 50, TRAIN, 0, 256, 0, name, 64, C.byref(grid)) == E_ARG
    assert lib.srfrd_encoder_plan_train(C.byref(lay), 0, 50, TRAIN, 0, 256, 0, name, 64, C.byref(grid)) == E_ARG
    assert lib.srfrd_encoder_plan_train(C.byref(lay), 8, 0, TRAIN, 0, 256, 0, name, 64, C.byref(grid)) == E_ARG
    assert lib.srfrd_encoder_plan_train(C.byref(lay), 8, 50, TRAIN, 0, 0, 0, name, 64, C.byref(grid)) == E_ARG
    assert lib.srfrd_encoder_plan_train(C.byref(lay), 8, 50, TRAIN, 0, 256, 0, name, 64, None) == E_ARG


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


ARGS = ("table", "dense", "packed", "ids", "fk", "pos", "pfk", "neg", "nfk", "hidden", "pl", "nl", "save_x", "save_h1",
        "save_aux", "loss_part", "grad_table", "contrib", "slabs", "sched")


def _train(lib, lay, B=8, L=50, p=0.5, fused_bce=1, d_hidden=None, sched_mode=1, **null):
    a = {k: (None if k in null else _d()) for k in ARGS}
    return lib.srfrd_encoder_train_sched(C.byref(lay), a["table"], a["dense"], a["packed"], a["ids"], a["fk"], a["pos"], a["pfk"],
                                         a["neg"], a["nfk"], B, L, p, 0, None, 0, a["hidden"], a["pl"], a["nl"], a["save_x"],
                                         a["save_h1"], a["save_aux"], a["loss_part"], d_hidden, None, None, fused_bce,
                                         a["grad_table"], a["contrib"], a["slabs"], None, 0, a["sched"], sched_mode, None)


def test_train_entry_declared_and_typed(lib):
    from tests.test_abi import header_symbols
    syms = header_symbols()
    for name in ("srfrd_encoder_train_sched", "srfrd_encoder_plan_train"):
        assert name in syms and name in _lib.SIGNATURES
        getattr(lib, name)


@pytest.mark.parametrize("null", ["table", "dense", "packed", "ids", "hidden", "pl", "nl", "save_x", "save_h1", "save_aux",
                                  "grad_table", "slabs", "sched"])
def test_train_entry_refuses_missing_buffers(lib, null):
    lay = _layout("SASRec", 50, 0, 0, 1)
    assert _train(lib, lay, **{null: True}) == E_ARG


def test_train_entry_refuses_malformed_calls(lib):
    lay = _layout("SASRec", 50, 0, 0, 1)
    assert _train(lib, lay, B=0) == E_ARG
    assert _train(lib, lay, L=0) == E_ARG
    assert _train(lib, lay, L=300) == E_ARG                  # longer than the layout's max_len
    assert _train(lib, lay, p=1.0) == E_ARG
    assert _train(lib, lay, sched_mode=2) == E_ARG
    assert _train(lib, lay, pos=True, pl=True) == E_ARG      # loss partials (and the fused BCE) without positive targets


def test_train_entry_refuses_where_the_plan_has_no_train_kernel(lib):
    sas = _layout("SASRec", 50, 0, 0, 1)
    assert _train(lib, sas, L=20) == E_UNSUPPORTED           # not the ragged geometry
    assert _train(lib, sas, L=100) == E_UNSUPPORTED
    assert _train(lib, sas, fused_bce=0) == E_UNSUPPORTED    # upstream logit gradients: the two calls
    assert _train(lib, sas, d_hidden=_d()) == E_UNSUPPORTED  # a hidden-state gradient: the two calls
    assert _train(lib, sas, loss_part=True) == E_UNSUPPORTED
    assert _train(lib, _layout("SASRec", 50, 0, 0, 2)) == E_UNSUPPORTED      # two attention heads
    assert _train(lib, _layout("SASRec", 40, 0, 0, 1)) == E_UNSUPPORTED      # hidden 40


def test_train_entry_honours_the_switches(lib, monkeypatch):
    monkeypatch.setenv("SRFRD_NO_RAGGED", "1")
    assert _train(lib, _layout("SASRec", 50, 0, 0, 1)) == E_UNSUPPORTED
    assert _lib.env_switches() & P.SWITCHES["SRFRD_NO_RAGGED"]
