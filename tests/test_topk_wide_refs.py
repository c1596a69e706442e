"""CPU: the wide top-k plan over every call shape tests/test_gpu_topk_wide.py makes, and the admissibility of its cases.

The plan is asked on the host (srfrd_topk_wide_plan makes no HIP call): every workgroup width is one the skew libraries split,
no launch asks for more than 160 KiB of dynamic LDS, a plan without a threshold can hold every score it may meet, the kernels
come in the order the path needs, the three planned paths are each reached (the fallback is in every plan: it is armed on the
device), the group count stays inside what the workspace query reserves, and the plan's rules hold as DESIGN section 26 states
them.  Every case is admissible on the reference alone: the share of (user, slot) pairs the fp64 reference itself leaves to
near ties stays under rank_refs.SKIP_CAP.  No GPU anywhere."""
import numpy as np
import pytest

from tests import rank_refs as R
from tests import topk_wide_refs as W


@pytest.fixture(scope="module")
def calls():
    import __graft_entry__ as g
    g.build()
    return W.wide_calls()


def test_every_planned_launch_fits_the_device_and_the_skew_libraries(calls):
    from srfrd_amd import _lib
    seen, widths = set(), set()
    for d, f, n_items, route, B, k, lo, hi, excl in calls:
        p = W.plan(d, f, n_items, route, B, k, lo, hi, excl)
        path, cap, groups = W.check_plan(p)
        seen.add(path)
        for name, grid, threads, lds in p[0]:
            assert threads in (64, 256, 512, 1024), (name, threads)
            assert 0 <= lds <= 160 * 1024 and grid >= 1, (name, grid, lds)
            widths.add((name.split("<")[0], threads))
        assert (p[0][0][0] == "srfrd::excl_prep_kernel") == excl
        if path == W.ALL:
            assert hi - lo <= cap and groups == 0, (d, route, k, lo, hi)          # tau = -inf: every row may be a candidate
        else:
            assert groups >= 2 * k, (d, route, k, lo, hi, groups)
        # the workspace holds the plan's maxima, the thresholds, the cursors and the lists
        need = _lib.query("srfrd_topk_wide_workspace_bytes", B=B, k=k, n_rows=hi - lo)
        assert need >= B * (groups * 4 + 8 + cap * 8), (d, route, k, lo, hi)
        select = next(l for l in p[0] if l[0] == "srfrd::wide_select_kernel")
        assert select[1] == B and select[3] == cap * 8                                # one workgroup per user sorts its list in LDS
    assert seen == {W.FINE, W.CHUNK, W.ALL}
    print(sorted(widths))


def test_the_listed_shapes_take_the_paths_the_gpu_file_names():
    full = (0, W.N_ITEMS + 1)
    for route, d in (("fp32", 50), ("fp32_forced", 50), ("bf16", 50), ("fp32", 64)):
        assert W.check_plan(W.plan(d, 0, W.N_ITEMS, route, W.B_WIDTHS, 100, *full, False))[0] == W.FINE
        assert W.check_plan(W.plan(d, 0, W.N_ITEMS, route, W.B_WIDTHS, 1024, *full, False))[0] == W.ALL
        assert W.check_plan(W.plan(d, 0, W.ONE_CHUNK_ITEMS, route, W.B_WIDTHS, 100, 0, W.ONE_CHUNK_ITEMS + 1, False))[0] == W.ALL
    cap = W.capacity()
    assert W.check_plan(W.plan(8, 0, cap, "fp32", 3, 1024, 0, cap + 1, False))[0] == W.FINE       # the fallback cases: planned fine,
    assert W.check_plan(W.plan(8, 0, cap, "fp32", 3, 100, 0, cap + 1, False))[0] == W.FINE        # overflowed on the device
    for d, route, B, k in W.CHUNK_CASES:
        rows = W.first_rows(d, route, B, k, W.CHUNK)
        assert W.check_plan(W.plan(d, 0, rows - 1, route, B, k, 0, rows, False), W.CHUNK)[2] >= 2 * k
        assert W.check_plan(W.plan(d, 0, rows - 257, route, B, k, 0, rows - 256, False))[0] == W.FINE    # one chunk fewer


def test_the_plan_rules():
    """2 k stream chunks keep the chunk maxima; below, the coarsest fine groups that give 4 k (stream16) or the 32 per chunk
    (fp32 stream); below 2 k groups no threshold, and then the range fits the capacity"""
    cap = W.capacity()
    for route, d in (("fp32", 50), ("bf16", 50), ("fp32_forced", 50), ("fp32", 60)):
        stream16 = R.is_stream16(d, route)
        for k in (65, 100, 256, 1024):
            for rows in (17, 257, 2601, 8193, cap, cap + 1, 40_001, 300_001, 600_001):
                p = W.plan(d, 0, rows - 1, route, 17, k, 0, rows, False)
                path, c, groups = W.check_plan(p)
                assert c == cap
                stream = next(l for l in p[0] if "collect" in l[0])
                if path == W.CHUNK:
                    assert groups in (-(-rows // 256), -(-rows // 512)) and groups >= 2 * k
                elif path == W.FINE:
                    assert groups >= 2 * k and -(-rows // 512) < 2 * k
                    if stream16:
                        assert groups < 8 * k + 128 and groups % 4 == 0
                    else:
                        assert groups == 32 * -(-rows // 256)
                else:
                    assert rows <= cap and groups == 0
                assert ("collect16" in stream[0]) == stream16


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("d", W.ADMISSIBLE_WIDTHS)
def test_the_width_cases_are_admissible_on_the_reference_alone(d, bf16):
    full = (0, W.N_ITEMS + 1)
    for case in (R.base_case(d), R.tie_case(d)):
        ref = case.ref(R.bf16_round(case.table) if bf16 else None)
        rows = R.exclusion_rows(ref, *full, W.N_ITEMS, d)
        for k in W.KS:
            assert R.skip_share(ref, k, *full, True) < R.SKIP_CAP, (d, bf16, k)
            assert R.skip_share(ref, k, *full, True, rows) < R.SKIP_CAP, (d, bf16, k, "excl")


@pytest.mark.parametrize("d, route, B, k", W.CHUNK_CASES)
def test_the_chunk_cases_are_admissible(d, route, B, k):
    rows = W.first_rows(d, route, B, k, W.CHUNK)
    case = R.base_case(d, 0, k, n_items=rows - 1, B=B)
    ref = case.ref(R.bf16_round(case.table) if route == "bf16" else None)
    assert R.skip_share(ref, k, 0, rows, True) < R.SKIP_CAP, (d, route, rows)


@pytest.mark.parametrize("d, route", W.RANGE_WIDTHS)
def test_the_range_tail_and_small_catalog_cases_are_admissible(d, route):
    """per case as the GPU file tallies it: the ranges of one Tally together, each batch tail with its exclusion rows"""
    tab = lambda c: R.bf16_round(c.table) if route == "bf16" else None
    share = lambda ref, calls: (lambda got: sum(s for s, _ in got) / max(sum(p for _, p in got), 1))(
        [R.check_topk(*R.topk_ref(ref.s, k, lo, hi, pad, x), ref, k, lo, hi, pad, x)[:2] for k, lo, hi, pad, x in calls])
    case = R.base_case(d)
    ref = case.ref(tab(case))
    calls = [(100, lo, hi, True, None) for lo, hi in R.ranges()] + [(100, lo, hi, False, None) for lo, hi in R.ranges() if lo == 0]
    calls.append((100, 257, 557, True, R.exclusion_rows(ref, 257, 557, W.N_ITEMS, d + 1)))
    assert share(ref, calls) < R.SKIP_CAP
    full = (0, W.N_ITEMS + 1)
    for B in W.TAIL_BATCHES:
        case = R.tail_case(d, B)
        ref = case.ref(tab(case))
        assert share(ref, [(100, *full, True, None), (100, *full, True, R.exclusion_rows(ref, *full, W.N_ITEMS, B))]) < R.SKIP_CAP, B
    case = R.one_chunk_case(d)
    ref, n = case.ref(tab(case)), W.ONE_CHUNK_ITEMS
    assert share(ref, [(100, 0, n + 1, True, None), (1024, 0, n + 1, False, None)]) < R.SKIP_CAP


@pytest.mark.parametrize("d, route", W.FALLBACK_CASES)
def test_the_zero_user_cases_are_admissible(d, route):
    cap = W.capacity()
    z = W.zero_user_case(d, cap + 1)
    ref = z.ref(R.bf16_round(z.table) if route == "bf16" else None)
    for k in (100, 1024):
        assert R.skip_share(ref, k, 0, cap + 1, False) < R.SKIP_CAP, (d, route, k)


def test_the_fallback_cases_have_the_lists_the_gpu_file_expects():
    cap = W.capacity()
    c = W.identical_rows_case(8, cap + 1)
    idx, val = R.topk_ref(c.ref().s, 100, 0, cap + 1, True)
    assert (idx == np.arange(1, 101)).all() and (val == val[:, :1]).all()
    z = W.zero_user_case(8, cap + 1)
    idx, val = R.topk_ref(z.ref().s, 100, 0, cap + 1, False)
    assert (idx[1] == np.arange(100)).all() and (val[1] == 0.0).all() and (val[0] != 0.0).all()
    two = W.without_user(z, 1)
    assert two.B == 2 and (two.hidden[1] == z.hidden[2]).all()
