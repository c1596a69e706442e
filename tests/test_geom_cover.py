"""Host-only guard of the width and head-split cases (tests/geom_refs.py; run by tests/test_gpu_geom_fp64.py): the list is what it
claims, it covers the run-time values it names, and the kernel names the GPU cases assert are what the plan answers here too.
Removing a case, or a plan change that moves one onto another kernel pair, turns these red without a GPU."""
import pytest

from srfrd_amd import _lib
from tests import geom_refs as W
from tests import grad_refs as G
from tests import test_gpu_bf16_families as F
from tests.test_encoder_plan import MODES, N_CU, _variant


def _lay(c):
    return _lib.make_layout(c.kind, G.I, c.L, c.d_item, c.d_fake, 3 if c.kind.startswith("SRFU") else 0, c.blocks, c.heads)


def test_the_list_is_what_it_claims():
    assert len(W.CASES) == 16 and len({c.id for c in W.CASES}) == 16
    assert len(G.ALL_CASES) == 61 and not {c.id for c in W.CASES} & set(G.BY_ID)
    assert all(G.case_of(c.id) is c for c in W.CASES)
    assert not any(c.id[0] in "tu" or c.id in G.SKEW_PADS for c in W.CASES)      # (grad_refs.batch_of: the synthetic batch)
    for c in W.CASES:
        D = W.width(c)
        assert c.blocks == 2 and c.switch is None and G.I == 300 and c.B == (6 if c.L < 100 else 5)
        assert (c.seed, c.fused_seed) == (W.FIRST_SEED, W.FIRST_SEED) == (50, 50)
        assert D <= 64 and D % c.heads == 0 and (c.d_fake > 0) == (c.kind in ("SRFR", "SRFRN"))
        assert _variant(c.kind, c.d_item, D, c.heads) is None                    # kind_variant == -1: no specialised family
        assert D != 50 or c.heads > 1
        assert G.cfg_of(c, "fused").D == D and G.cfg_of(c, "fused").num_heads == c.heads
    assert len(W.GRAD_JOBS) == 32 and len(W.FWD_JOBS) == 48
    assert [c.id for c in W.BF16_CASES] == ["w33", "w64b"] and not {c.id for c in W.BF16_CASES} & {c.id for c in F.CASES}
    for c in W.BF16_CASES:                                 # 2-byte shadow rows of 66 and 128 bytes
        assert c._replace(seed=50, fused_seed=50) == W.BY_ID[c.id]
    assert [2 * W.width(c) for c in W.BF16_CASES] == [66, 128] and W.BF16_CASES[1].autograd == W.LDS_LONG


def test_the_cases_cover_the_run_time_geometry():
    geo = {c.id: W.geometry(c) for c in W.CASES}
    assert {g["NT"] for g in geo.values()} == {1, 2, 3, 4}
    assert any(g["DK"] > g["D"] for g in geo.values()) and any(g["DK"] == g["D"] == 64 for g in geo.values())
    assert any(g["D"] % 16 == 1 for g in geo.values())                           # one live column in the last tile
    assert {g["D"] for g in geo.values()} >= {64, 63, 33, 32, 17, 16, 8, 4}
    assert {geo[c.id]["dh"] for c in W.MULTI_HEAD} >= {1, 4, 5, 8, 9, 10, 11, 16, 32}
    assert any(c.d_fake > 0 for c in W.MULTI_HEAD) and any(c.kind.startswith("SRFU") for c in W.MULTI_HEAD)
    assert len({g["conv_tiles"] for c in W.CASES if c.kind == "SRFR" for g in [geo[c.id]]}) >= 2
    assert all(g["d_out"] < g["D"] for c in W.CASES if c.kind == "SRFR" for g in [geo[c.id]])
    assert any(c.L == g["LP"] == 16 for c in W.CASES for g in [geo[c.id]])        # one row tile, no padded row
    assert any(g["LP"] % 32 == 16 and g["LP"] > c.L for c in W.CASES for g in [geo[c.id]])   # an odd number of row tiles
    # S (LP x SLD) against the state (LP x DS): each is the larger overlay somewhere
    assert any(g["LP"] + 2 > g["DK"] + 2 for g in geo.values()) and any(g["LP"] + 2 < g["DK"] + 2 for g in geo.values())


def test_each_generic_pair_is_reached_off_width_50_and_with_heads():
    for pair in W.PAIRS:
        mine = [c for c in W.CASES if tuple(c.autograd) == pair]
        assert any(W.width(c) != 50 for c in mine), pair
        assert any(c.heads > 1 for c in mine), pair
    assert all(tuple(c.autograd) in W.PAIRS for c in W.CASES)
    # the rows whose seam IS the pair: the backward leaves LDS at LP = 64 and width 64, LP = 48 is the last that stays, the
    # forward leaves at LP = 112
    assert tuple(W.BY_ID["w64b"].autograd) == W.LDS_LONG and tuple(W.BY_ID["w64e"].autograd) == W.LONG_LONG
    assert tuple(W.BY_ID["w64d"].autograd) == tuple(W.BY_ID["w64c"].autograd) == W.LDS_LDS
    assert tuple(W.BY_ID["w32b"].autograd) == W.LDS_LONG


@pytest.mark.parametrize("c", W.CASES, ids=[c.id for c in W.CASES])
def test_case_names_are_the_plans(c):
    """the literal names each GPU case asserts before it launches, against the host-only plan, in all four launch modes"""
    lay = _lay(c)
    want = {"eval": (c.eval_fwd, None), "last": (c.last_fwd, None), "autograd": tuple(c.autograd), "fused": tuple(c.fused)}
    for launch, names in want.items():
        assert F.planned(lay, c.B, c.L, launch, 0, N_CU, *F.case_scratch(lay, c.B, c.L, launch)) == names, (c.id, launch)
    assert c.eval_fwd == c.last_fwd == c.autograd[0] == c.fused[0] and c.autograd[1] == c.fused[1]
    assert not _lib.encoder_plan_train(lay, c.B, c.L, MODES["fused_p"], 0)[0]    # no one-launch train kernel off the default geometry
    fwd_lds, bwd_lds = _lib.lds_bytes(lay, c.L)
    assert (fwd_lds == 0) == c.eval_fwd.startswith("srfrd_long::") and (bwd_lds == 0) == c.autograd[1].startswith("srfrd_long::")


def test_w64d_is_the_last_length_whose_backward_stays_in_lds():
    c = W.BY_ID["w64d"]
    assert c.L == 48 and _lib.lds_bytes(_lay(c), 48)[1] > 0 and _lib.lds_bytes(_lay(c._replace(L=49)), 49)[1] == 0
