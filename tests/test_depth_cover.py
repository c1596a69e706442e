"""Host-only guard of the depth cases (tests/grad_refs.py, DEPTH; run by tests/test_gpu_grad_fp64.py and test_gpu_fwd_fp64.py):
at depths 1 and 3 they reach every encoder kernel family the plan can choose there, at depth 8 they run what the plan answers
once the LayerNorm caches are at their largest, and the kernel names the GPU cases assert are what the plan answers here too.
Removing a depth-1 or depth-3 case, or a plan change that moves one onto another family, turns these red without a GPU."""
import pytest

from srfrd_amd import _lib
from tests import grad_refs as G
from tests import test_bf16_family_cover as C
from tests import test_gpu_bf16_families as F
from tests.test_encoder_plan import MODES, N_CU, _layout, _rows

COVERED = (1, 3)
BY_DEPTH = {n: [c for c in G.DEPTH if c.blocks == n] for n in (1, 3, 8)}
# what the five depth-8 cases run, as literals (autograd and fused; the forwards of eval / last are the cases' own fields)
DEPTH8 = {
    "t0.8": ("srfrd::encoder_fwd_ragged_kernel<0,0,50>", "srfrd::encoder_fwd_ragged_kernel<0,1,50>", "srfrd::encoder_bwd_ragged_kernel<0,50>"),
    "t2.8": ("srfrd::encoder_fwd_ragged_kernel<2,0,45>", "srfrd::encoder_fwd_ragged_kernel<2,1,45>", "srfrd::encoder_bwd_ragged_kernel<2,45>"),
    "g.8": ("srfrd::encoder_fwd_kernel<50,112,8,100,0,0,50>", "srfrd::encoder_fwd_kernel<50,112,16,100,0,1,50>",
            "srfrd::encoder_bwd_slots_kernel<50,100,0,50>"),
    "l.8": ("srfrd::encoder_fwd_rows_kernel<50,-1,50,1>", "srfrd::encoder_fwd_rows_kernel<50,-1,50,1>", "srfrd::encoder_bwd_chunks_kernel<50,-1,50>"),
    # with eight blocks the first-generation backward's LDS no longer fits at LP = 64: two heads leave it for the global-scratch build
    "d.8": ("srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd::encoder_fwd_kernel<0,0,0,0,-1,0,0>", "srfrd_long::encoder_bwd_kernel<0,0,0,0,-1,0,0>"),
}


def _case_layout(c):
    return _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)


def _targets(nb):
    """every family key the plan test's rows produce at depth nb in the four modes that launch"""
    out = set()
    for kind, di, df, nl, heads, L, mname, sw, B in _rows():
        if mname in C.RUN_MODES:
            out.update(C._keys(_layout(kind, di, df, nl, heads, nb), B, L, mname, sw))
    return out


def _produced(nb):
    """family key -> kinds of the depth-nb cases that run it"""
    out = {}
    for c in BY_DEPTH[nb]:
        for mname in C.RUN_MODES:
            for k in C._keys(_case_layout(c), c.B, c.L, mname, c.switch):
                out.setdefault(k, set()).add(c.kind)
    return out


def test_the_depth_list_is_what_it_claims():
    assert len({c.id for c in G.DEPTH}) == len(G.DEPTH) and all(c in G.ALL_CASES for c in G.DEPTH)
    assert {c.blocks for c in G.DEPTH} == {1, 3, 8} and len(BY_DEPTH[8]) == 5 and not any(c.blocks != 2 for c in F.CASES)
    assert all(c.B in (5, 6) or c.id.startswith("t") and c.B == len(G.TILE_PADS) for c in G.DEPTH)
    assert all(cid in G.TRAIN_KERNEL_IDS for cid in ("t0.1", "t0.3", "t0.8"))
    assert all(i.endswith(f"-b{c.blocks}") for i, c in zip(G.case_ids(G.DEPTH), G.DEPTH))
    assert not any("-b" in i for i in G.case_ids(G.DEPTH2_CASES))
    for c in G.DEPTH:                                     # a twin: the depth-2 case of its id, but for the depth and k.3's length
        base = G.BY_ID[c.id.split(".")[0]]
        assert c.id == f"{base.id}.{c.blocks}" and base.blocks == 2
        assert c[1:5] + (c.B, c.switch) == base[1:5] + (base.B, base.switch)
        assert c.L == base.L or (c.id, c.L) == ("k.3", 200)


@pytest.mark.parametrize("nb", COVERED)
def test_every_family_key_of_the_depth_is_run(nb):
    targets = _targets(nb)
    assert targets == C.TARGETS                           # depths 1 and 3 lose no family and gain none
    produced = _produced(nb)
    for key in sorted(targets):
        assert key in produced, f"no depth-{nb} case runs {key}"
    for key in C.KIND_VARIANT_BWD:
        assert "SRFRN" in produced[key], f"depth {nb}, {key}: no SRFRN case"
        assert produced[key] & {"SASRec", "SRFU_B", "SRFU_F", "SRFU_R"}, f"depth {nb}, {key}: no case without a fake channel"
    mine = BY_DEPTH[nb]
    assert any(c.kind == "SRFR" for c in mine)                                              # d_out < D: the last_conv head
    assert any(c.heads == 2 and c.autograd == (F._F + F._GEN, F._B + F._GEN) for c in mine)  # the two-head generic pair


def test_depth_8_loses_two_first_generation_backwards():
    """at depth 8 the first-generation backward's working set passes 160 KB from LP = 64 on: the plan's rows no longer hold
    its <50,64,8,0> and <50,64,8,50> instantiations, and hold nothing new"""
    assert C.TARGETS - _targets(8) == {"srfrd::encoder_bwd_kernel<50,64,8,0>", "srfrd::encoder_bwd_kernel<50,64,8,50>"}
    assert _targets(8) <= C.TARGETS


@pytest.mark.parametrize("c", G.DEPTH, ids=[c.id for c in G.DEPTH])
def test_depth_case_names_are_the_plans(c):
    """the literal names each GPU case asserts before it launches, against the host-only plan"""
    lay = _case_layout(c)
    sw = _lib.SWITCHES[c.switch] if c.switch else 0
    want = {"eval": (c.eval_fwd, None), "last": (c.last_fwd, None), "autograd": c.autograd, "fused": c.fused}
    for launch, names in want.items():
        assert F.planned(lay, c.B, c.L, launch, sw, N_CU, *F.case_scratch(lay, c.B, c.L, launch)) == names, (c.id, launch)
    if c.blocks == 8:
        f0, f1, b = DEPTH8[c.id]
        assert (c.autograd, c.fused) == ((f0, b), (f1, b))
    offered = _lib.encoder_plan_train(lay, c.B, c.L, MODES["fused_p"], sw)[0].startswith("srfrd::encoder_train_ragged_kernel<")
    assert offered == c.id.startswith("t")                # the one-launch train kernel: the default geometry, at every depth
