"""Host-only guard of the bf16 item-table tests (tests/test_gpu_bf16_families.py, test_gpu_bf16_table.py): their shapes reach
every encoder kernel family the plan can choose, and the kernel names the GPU cases assert are what the plan answers here too.
A later trimming of the case list, or a plan change that moves a case onto another family, turns these red on a machine
without a GPU."""
import re

import pytest

from srfrd_amd import _lib
from tests import test_gpu_bf16_families as F
from tests.test_encoder_plan import MODES, N_CU, _layout, _rows
from tests.test_gpu_bf16_table import FUSED_KIND, SHAPES

RUN_MODES = ("eval", "eval_last", "autograd", "fused_p")
_NAME = re.compile(r"(srfrd(?:_long)?::encoder_(?:fwd|bwd)(?:_[a-z]+)?_kernel)<(.*)>")
FIRST = {"srfrd::encoder_fwd_kernel", "srfrd::encoder_bwd_kernel", "srfrd_long::encoder_fwd_kernel", "srfrd_long::encoder_bwd_kernel"}
# backward families that read the table through a kind variant <K, DI>: the bf16 branch selects between the shadow and the
# fp32 side table, so each needs a kind without a fake channel and SRFRN
KIND_VARIANT_BWD = ("srfrd::encoder_bwd_kernel<50,64,8,50>", "srfrd::encoder_bwd_slots_kernel<L=50>",
                    "srfrd::encoder_bwd_slots_kernel<L=100>", "srfrd::encoder_bwd_chunks_kernel",
                    "srfrd::encoder_bwd_ragged_kernel")
# every key test_encoder_plan's rows produce in the four modes that launch (a new family in the plan has to be added here,
# and then needs a bf16 case)
TARGETS = {
    "srfrd::encoder_fwd_kernel<0,0,0,0>", "srfrd::encoder_fwd_kernel<50,32,8,0>", "srfrd::encoder_fwd_kernel<50,64,8,0>",
    "srfrd::encoder_fwd_kernel<50,64,8,50>", "srfrd::encoder_fwd_kernel<50,112,8,100>", "srfrd::encoder_fwd_kernel<50,112,16,100>",
    "srfrd::encoder_fwd_ragged_kernel<mode=0>", "srfrd::encoder_fwd_ragged_kernel<mode=1>",
    "srfrd::encoder_fwd_rows_kernel<mode=0>", "srfrd::encoder_fwd_rows_kernel<mode=1>", "srfrd_long::encoder_fwd_kernel<0,0,0,0>",
    "srfrd::encoder_bwd_kernel<0,0,0,0>", "srfrd::encoder_bwd_kernel<50,32,8,0>", "srfrd::encoder_bwd_kernel<50,64,8,0>",
    "srfrd::encoder_bwd_kernel<50,64,8,50>", "srfrd::encoder_bwd_ragged_kernel", "srfrd::encoder_bwd_slots_kernel<L=50>",
    "srfrd::encoder_bwd_slots_kernel<L=100>", "srfrd::encoder_bwd_chunks_kernel", "srfrd_long::encoder_bwd_kernel<0,0,0,0>",
    "srfrd_long::encoder_bwd_kernel<50,112,8,100>",
}


def family_key(name):
    """A plan name without kind, DI and the read-modify-write flag: the kernel function with its namespace, plus the first four
    template arguments (first-generation and srfrd_long:: kernels), the mode flag (row-owner and ragged forward) or the sequence
    length (slot-placed backward)."""
    m = _NAME.fullmatch(name)
    assert m, name
    fn, t = m.group(1), m.group(2).split(",")
    if fn in FIRST:
        return f"{fn}<{','.join(t[:4])}>"
    if fn == "srfrd::encoder_fwd_rows_kernel":
        return f"{fn}<mode={t[3]}>"
    if fn == "srfrd::encoder_fwd_ragged_kernel":
        return f"{fn}<mode={t[1]}>"
    if fn == "srfrd::encoder_bwd_slots_kernel":
        return f"{fn}<L={t[1]}>"
    assert fn in ("srfrd::encoder_bwd_chunks_kernel", "srfrd::encoder_bwd_ragged_kernel"), name
    return fn


def _keys(lay, B, L, mname, sw):
    (f, _), (b, _) = _lib.encoder_plan(lay, B, L, MODES[mname], _lib.SWITCHES[sw] if sw else 0, N_CU,
                                       max(_lib.scratch_floats(lay, B, L)))
    return [family_key(n) for n in (f, b) if n]               # (an unsupported direction reads "")


def _targets():
    out = set()
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        if mname in RUN_MODES:
            out.update(_keys(_layout(kind, di, df, nl, heads), B, L, mname, sw))
    return out


def _case_layout(c):
    return _lib.make_layout(c.kind, F.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)


def _produced():
    """family key -> kinds of the bf16 cases that run it"""
    out = {}
    for c in F.CASES:
        for mname in RUN_MODES:
            for k in _keys(_case_layout(c), c.B, c.L, mname, c.switch):
                out.setdefault(k, set()).add(c.kind)
    # tests/test_gpu_bf16_table.py: a training-mode forward with its autograd backward and the last-position forward at every
    # shape, the fused step at seq_len 50 (I = 400, B = 9 / 12 there; neither enters a name)
    for kind, L in SHAPES:
        di, df, nl = {"SASRec": (50, 0, 0), "SRFRN": (45, 5, 0)}.get(kind, (50, 0, 3))
        lay = _lib.make_layout(kind, 400, L, di, df, nl, 2, 1)
        for mname in ("autograd", "eval_last") + (("fused_p",) if (kind, L) == (FUSED_KIND, 50) else ()):
            for k in _keys(lay, 9, L, mname, None):
                out.setdefault(k, set()).add(kind)
    return out


def test_family_key_reduction_and_target_set():
    assert family_key("srfrd::encoder_fwd_kernel<50,112,16,100,0,1,50>") == "srfrd::encoder_fwd_kernel<50,112,16,100>"
    assert family_key("srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>") == "srfrd_long::encoder_bwd_kernel<0,0,0,0>"
    assert family_key("srfrd::encoder_fwd_rows_kernel<50,2,45,0>") == "srfrd::encoder_fwd_rows_kernel<mode=0>"
    assert family_key("srfrd::encoder_fwd_ragged_kernel<2,1,45>") == "srfrd::encoder_fwd_ragged_kernel<mode=1>"
    assert family_key("srfrd::encoder_bwd_slots_kernel<50,100,2,45,true>") == "srfrd::encoder_bwd_slots_kernel<L=100>"
    assert family_key("srfrd::encoder_bwd_chunks_kernel<50,-1,50,false>") == "srfrd::encoder_bwd_chunks_kernel"
    assert _targets() == TARGETS and set(KIND_VARIANT_BWD) <= TARGETS


def test_every_family_key_is_run_on_the_bf16_table():
    produced = _produced()
    for key in sorted(_targets()):
        assert key in produced, f"no bf16 case runs {key}"


def test_kind_variant_backwards_meet_both_sides_of_the_select():
    produced = _produced()
    for key in KIND_VARIANT_BWD:
        kinds = produced.get(key, set())
        assert "SRFRN" in kinds, f"{key}: no SRFRN case (shadow / side-table select)"
        assert kinds & {"SASRec", "SRFU_B", "SRFU_F", "SRFU_R"}, f"{key}: no case without a fake channel"
    assert any(c.kind == "SRFR" for c in F.CASES)             # d_out < D: the last_conv head


@pytest.mark.parametrize("c", F.CASES, ids=[c.id for c in F.CASES])
def test_case_names_are_the_plans(c):
    """the literal names each GPU case asserts before it launches, against the host-only plan"""
    lay = _case_layout(c)
    sw = _lib.SWITCHES[c.switch] if c.switch else 0
    want = {"eval": (c.eval_fwd, None), "last": (c.last_fwd, None), "autograd": c.autograd, "fused": c.fused}
    for launch, names in want.items():
        assert F.planned(lay, c.B, c.L, launch, sw, N_CU, *F.case_scratch(lay, c.B, c.L, launch)) == names, (c.id, launch)
    assert c.B in (5, 6) and len({x.id for x in F.CASES}) == len(F.CASES)
