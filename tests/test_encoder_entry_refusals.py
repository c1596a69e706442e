"""CPU: what the seven launching entry points of the encoder refuse, and with which code.

srfrd_encoder_fwd / _fwd_sched / _fwd_last, srfrd_encoder_bwd / _bwd_sched and srfrd_encoder_train_sched / _train_ranked each
check their own arguments, the shared ones, their outputs and checkpoints, and then ask the kernel plan - in that order.  Every
row below carries at least one defect, so every call returns SRFRD_E_ARG or SRFRD_E_UNSUPPORTED before anything is launched:
the pointers are dummies that nothing dereferences.  (The accepting direction is the GPU tests'.)
"""
import ctypes as C

import pytest

from srfrd_amd import _lib

E_ARG, E_UNSUPPORTED = -1, -2
ENTRIES = ("fwd", "fwd_sched", "fwd_last", "bwd", "bwd_sched", "train_sched", "train_ranked")
ALL = set(ENTRIES)
FULL = ALL - {"fwd_last"}                                   # take targets, dropout and checkpoints
FORWARD = {"fwd", "fwd_sched", "train_sched", "train_ranked"}
BACKWARD = {"bwd", "bwd_sched", "train_sched", "train_ranked"}
SCHED = {"fwd_sched", "bwd_sched", "train_sched"}
TRAIN = {"train_sched", "train_ranked"}

# every layout: max_len 200, 2 blocks, 1 head
LAYOUTS = {"sas": ("SASRec", 50, 0), "srfrn": ("SRFRN", 45, 5), "wide": ("SASRec", 80, 0), "h40": ("SASRec", 40, 0)}
BUFFERS = ("table", "dense", "packed", "ids", "fk", "pos", "pfk", "neg", "nfk", "hidden", "pl", "nl", "save_x", "save_h1",
           "save_aux", "loss_part", "d_pos", "d_neg", "grad_table", "contrib", "slabs", "sched")
NEG = ("neg", "nfk", "nl")
POS = ("pos", "pfk", "pl")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def layouts(lib):
    return {name: _lib.make_layout(kind, 300, 200, di, df, 0, 2, 1) for name, (kind, di, df) in LAYOUTS.items()}


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def _call(lib, layouts, entry, layout="sas", null=(), B=8, L=50, p=0.5, fused_bce=1, d_hidden=None, scratch=None,
          scratch_floats=0, sched_mode=1, pair_stride=256, ids_at=64):
    """The base call - every buffer present - with the row's defects applied, marshalled for `entry`."""
    a = {k: (None if k in null else _d()) for k in BUFFERS}
    a["ids"] = None if "ids" in null else _d(ids_at)
    lay = None if layout is None else C.byref(layouts[layout])
    head = (lay, a["table"], a["dense"], a["packed"], a["ids"], a["fk"])
    targets = (a["pos"], a["pfk"], a["neg"], a["nfk"], B, L, p, 0, None, 0)
    fwd_out = (a["hidden"], a["pl"], a["nl"], a["save_x"], a["save_h1"], a["save_aux"])
    upstream = (d_hidden, a["d_pos"], a["d_neg"], fused_bce)
    grads = (a["grad_table"], a["contrib"], a["slabs"])
    scr = (scratch, scratch_floats)
    if entry == "fwd":
        return lib.srfrd_encoder_fwd(*head, *targets, *fwd_out, a["loss_part"], *scr, None, 0, None)
    if entry == "fwd_sched":
        return lib.srfrd_encoder_fwd_sched(*head, *targets, *fwd_out, a["loss_part"], *scr, a["sched"], sched_mode, None)
    if entry == "fwd_last":
        return lib.srfrd_encoder_fwd_last(*head, B, L, a["hidden"], *scr, None)
    if entry == "bwd":
        return lib.srfrd_encoder_bwd(*head, *targets, *fwd_out, *upstream, *grads, *scr, None, 0, None)
    if entry == "bwd_sched":
        return lib.srfrd_encoder_bwd_sched(*head, *targets, *fwd_out, *upstream, *grads, *scr, a["sched"], sched_mode, None)
    if entry == "train_sched":
        return lib.srfrd_encoder_train_sched(*head, *targets, *fwd_out, a["loss_part"], *upstream, *grads, *scr, a["sched"],
                                             sched_mode, None)
    assert entry == "train_ranked"
    return lib.srfrd_encoder_train_ranked(*head, *targets, *fwd_out, a["loss_part"], fused_bce, *grads, pair_stride, None)


def _short_scratch(lib, layouts):
    """srfrd_encoder_train_sched's scratch demand at the base shape, one float short"""
    return dict(scratch=_d(), scratch_floats=lib.srfrd_train_scratch_floats(C.byref(layouts["sas"]), 8, 50) - 1)


# (row, the entry points it applies to, the defects, the code)
ROWS = [
    ("no_layout", ALL, dict(layout=None), E_ARG),
    *[(f"no_{b}", ALL, dict(null=(b,)), E_ARG) for b in ("table", "dense", "packed", "ids", "hidden")],
    ("B0", ALL, dict(B=0), E_ARG),
    ("L0", ALL, dict(L=0), E_ARG),
    ("L201", ALL, dict(L=201), E_ARG),                                              # longer than the layout's max_len
    ("wide", ALL, dict(layout="wide"), E_UNSUPPORTED),
    ("wide_no_hidden", ALL, dict(layout="wide", null=("hidden",)), E_UNSUPPORTED),  # the layout is judged first
    ("h40_L200_no_scratch", ALL, dict(layout="h40", L=200), E_UNSUPPORTED),

    ("p1", FULL, dict(p=1.0), E_ARG),
    ("p_negative", FULL, dict(p=-0.1), E_ARG),
    *[(f"no_{b}", FULL, dict(null=(b,)), E_ARG) for b in ("pl", "nl", "save_x", "save_h1", "save_aux")],
    ("srfrn_no_pos_fake", FULL, dict(layout="srfrn", null=("pfk",)), E_ARG),
    ("srfrn_no_neg_fake", FULL, dict(layout="srfrn", null=("nfk",)), E_ARG),

    ("loss_without_negatives", FORWARD, dict(null=NEG), E_ARG),
    ("loss_without_positives", FORWARD, dict(null=POS), E_ARG),

    ("no_grad_table", BACKWARD, dict(null=("grad_table",)), E_ARG),
    ("no_slabs", BACKWARD, dict(null=("slabs",)), E_ARG),
    ("fused_bce_no_pos_ids", BACKWARD, dict(null=("pos",)), E_ARG),

    ("sched_mode_2", SCHED, dict(sched_mode=2), E_ARG),
    ("sched_mode_negative", SCHED, dict(sched_mode=-1), E_ARG),
    ("no_sched", SCHED, dict(null=("sched",)), E_ARG),
    ("sched_mode_2_wide", SCHED, dict(sched_mode=2, layout="wide"), E_ARG),         # the schedule check comes before the layout
    ("sched_mode_2_L200", SCHED, dict(sched_mode=2, L=200), E_ARG),

    ("L20", TRAIN, dict(L=20), E_UNSUPPORTED),                                      # not the ragged geometry
    ("L100", TRAIN, dict(L=100), E_UNSUPPORTED),
    ("no_fused_bce", TRAIN, dict(fused_bce=0), E_UNSUPPORTED),                      # upstream logit gradients: the two calls
    ("no_loss_part", TRAIN, dict(null=("loss_part",)), E_UNSUPPORTED),
    ("h40", TRAIN, dict(layout="h40"), E_UNSUPPORTED),

    ("d_hidden", {"train_sched"}, dict(d_hidden=_d()), E_UNSUPPORTED),              # a hidden-state gradient: the two calls
    ("no_scratch", {"train_sched"}, dict(), E_ARG),                                 # a valid plan: the scratch is demanded
    ("scratch_one_short", {"train_sched"}, _short_scratch, E_ARG),
    ("L20_no_scratch", {"train_sched"}, dict(L=20), E_UNSUPPORTED),                 # the plan answers before the scratch demand

    ("pair_stride_negative", {"train_ranked"}, dict(pair_stride=-1), E_ARG),
    ("ids_misaligned", {"train_ranked"}, dict(ids_at=72), E_ARG),                   # (the scan reads two ids per lane)
    ("pair_stride_negative_wide", {"train_ranked"}, dict(pair_stride=-1, layout="wide"), E_ARG),
]
CASES = [(entry, row, defects, code) for row, entries, defects, code in ROWS for entry in ENTRIES if entry in entries]


def test_every_row_carries_a_defect():
    """The base call itself is never made: on a GPU machine it would launch on the dummy pointers."""
    assert len(CASES) == 190
    for entry, row, defects, code in CASES:
        assert code in (E_ARG, E_UNSUPPORTED), (entry, row)
        assert callable(defects) or defects or (entry, row) == ("train_sched", "no_scratch"), (entry, row)
    assert sum(code == E_ARG for *_, code in CASES) == 157 and sum(code == E_UNSUPPORTED for *_, code in CASES) == 33


@pytest.mark.parametrize("entry,row,defects,code", CASES, ids=[f"{e}-{r}" for e, r, _, _ in CASES])
def test_entry_refuses(lib, layouts, entry, row, defects, code):
    if callable(defects):
        defects = defects(lib, layouts)
    assert _call(lib, layouts, entry, **defects) == code
