"""CPU: the filtered plan over every call shape tests/test_gpu_topk_allow.py makes, its rule, and the admissibility of its cases.

The plan is asked on the host (srfrd_topk_allow_plan makes no HIP call).  The rule is a bound: every reported plan has groups
of r rows with r k <= capacity, on both streams, and takes no maxima exactly when the range has at most `capacity` rows.  The
workspace query covers every plan's maxima.  Every GPU case is admissible on the reference alone: with the filter folded into
the reference's exclusion rows, the share of (user, slot) pairs the fp64 reference itself leaves to near ties stays under
rank_refs.SKIP_CAP.  No GPU anywhere."""
import numpy as np
import pytest

from tests import rank_refs as R
from tests import topk_allow_refs as A


@pytest.fixture(scope="module")
def calls():
    import __graft_entry__ as g
    g.build()
    return A.allow_calls()


def test_every_planned_launch_fits_the_device_and_the_workspace(calls):
    from srfrd_amd import _lib
    seen = set()
    for d, f, n_items, route, B, k, lo, hi, excl in calls:
        p = A.plan(d, f, n_items, route, B, k, lo, hi, excl)
        path, cap, groups = A.check_plan(p, excl=excl)
        seen.add(path)
        assert cap == A.CAPACITY
        for name, grid, threads, lds in p[0]:
            assert threads in (64, 256, 512, 1024), (name, threads)
            assert 0 <= lds <= 160 * 1024 and grid >= 1, (name, grid, lds)
        r = A.rows_per_group(p, hi - lo)
        assert r * k <= cap, (d, route, k, lo, hi, r)
        assert (path == A.ALL) == (hi - lo <= cap) and (groups == 0) == (path == A.ALL)
        need = _lib.query("srfrd_topk_allow_workspace_bytes", B=B, k=k, n_rows=hi - lo)
        chunks = -(-(hi - lo) // 256)
        assert need >= B * (groups * 4 + 8 + cap * 8 + chunks * 16), (d, route, k, lo, hi)
        select = next(l for l in p[0] if l[0] == "srfrd::wide_select_kernel")
        assert select[1] == B and select[3] == cap * 8
    assert seen == {A.FINE, A.ALL}


@pytest.mark.parametrize("route, d", [("fp32", 50), ("bf16", 50), ("bf16", 64), ("fp32_forced", 50), ("fp32", 60)])
def test_the_plan_rule_is_a_bound(route, d):
    """rows per group * k <= capacity on every reported plan; the strips of 64 / 32 / 16 rows (stream16) and the 8-row groups
    (fp32 stream); no maxima exactly when the range has at most `capacity` rows"""
    import __graft_entry__ as g
    g.build()
    cap = A.CAPACITY
    stream16 = R.is_stream16(d, route)
    for k in A.PLAN_KS:
        for rows in (2, 17, 257, 2601, cap - 1, cap, cap + 1, 20_001, 300_001, 1_000_001):
            for excl in (False, True):
                for B in (17, 300):
                    p = A.plan(d, 0, rows - 1, route, B, k, 0, rows, excl)
                    path, c, groups = A.check_plan(p, excl=excl)
                    assert c == cap
                    assert (path == A.ALL) == (rows <= cap), (k, rows)
                    r = A.rows_per_group(p, rows)
                    assert r * k <= cap, (k, rows, r)
                    stream = next(l for l in p[0] if "collect" in l[0])
                    assert ("collect16" in stream[0]) == stream16
                    if path == A.FINE:
                        assert r == ((64 if k <= 256 else 32 if k <= 512 else 16) if stream16 else 8), (k, rows, r)
                        assert groups == (256 // r) * -(-rows // 256)


def test_launch_names_and_geometry_of_one_plan_per_path():
    import __graft_entry__ as g
    g.build()
    full = (0, A.BIG_ITEMS + 1)
    chunks = -(-(A.BIG_ITEMS + 1) // 256)
    # stream16 over the fp32 table, with exclusion sets: the masked plan's geometry, one user tile per wave
    launches, sizes = A.plan(50, 0, A.BIG_ITEMS, "fp32", A.B, 100, *full, True)
    assert sizes == (A.FINE, A.CAPACITY, 4 * chunks)
    assert [l[0] for l in launches] == ["srfrd::excl_prep_kernel", "srfrd::allow_max16_kernel<true,true>", "srfrd::wide_tau_kernel",
                                        "srfrd::allow_collect16_kernel<true,true>", "srfrd::wide_select_kernel", "srfrd::allow_fallback_kernel"]
    assert launches[1][1:] == launches[3][1:] and launches[1][2] == 1024
    assert launches[2][1:] == (A.B, 256, 0) and launches[4][1:] == (A.B, 1024, A.CAPACITY * 8) and launches[5][1:] == (A.B, 1024, 0)
    masked = R.plan(50, 0, A.BIG_ITEMS, "fp32", 0, A.B, 10, *full, True)
    assert masked[1][0] == "srfrd::topk_max16_kernel<1,true,true>" and masked[1][1:] == launches[1][1:]
    # the same call without sets: the same stream geometry, the unmasked instantiation, no pre-pass
    plain, _ = A.plan(50, 0, A.BIG_ITEMS, "fp32", A.B, 100, *full, False)
    assert [l[0] for l in plain][:2] == ["srfrd::allow_max16_kernel<true,false>", "srfrd::wide_tau_kernel"] and plain[0][1:] == launches[1][1:]
    # the bf16 shadow at k = 1024: 16-row strips
    launches, sizes = A.plan(50, 0, A.BIG_ITEMS, "bf16", A.B, 1024, *full, False)
    assert sizes == (A.FINE, A.CAPACITY, 16 * chunks) and launches[0][0] == "srfrd::allow_max16_kernel<false,false>"
    # the fp32 stream
    launches, sizes = A.plan(64, 0, A.BIG_ITEMS, "fp32", A.B, 1024, *full, False)
    assert sizes == (A.FINE, A.CAPACITY, 32 * chunks)
    assert [l[0] for l in launches] == ["srfrd::allow_max_kernel<false>", "srfrd::wide_tau_kernel", "srfrd::allow_collect_kernel<false>",
                                        "srfrd::wide_select_kernel", "srfrd::allow_fallback_kernel"]
    assert launches[0][2] == 512 and launches[0][1:] == launches[2][1:]
    # no maxima
    launches, sizes = A.plan(50, 0, A.N_ITEMS, "fp32", A.B, 1024, 0, A.N_ITEMS + 1, False)
    assert sizes == (A.ALL, A.CAPACITY, 0)
    assert [l[0] for l in launches] == ["srfrd::wide_tau_kernel", "srfrd::allow_collect16_kernel<true,false>", "srfrd::wide_select_kernel",
                                        "srfrd::allow_fallback_kernel"]


# ---- admissibility ----------------------------------------------------------------------------------------------------------------
def _tab(case, route):
    return R.bf16_round(case.table) if route == "bf16" else None


def _share(ref, calls):
    got = [R.check_topk(*R.topk_ref(ref.s, k, lo, hi, pad, x), ref, k, lo, hi, pad, x)[:2] for k, lo, hi, pad, x in calls]
    return sum(s for s, _ in got) / max(sum(p for _, p in got), 1)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("d, f", A.SWEEP_CASES)
def test_the_sweep_cases_are_admissible_on_the_reference_alone(d, f, bf16):
    case = R.base_case(d, f)
    ref = case.ref(R.bf16_round(case.table) if bf16 else None)
    rows = A.union_rows(A.filter_mask("random_0.5", A.N_ITEMS, d), [0] * A.B)
    assert _share(ref, [(k, 0, A.N_ITEMS + 1, True, rows) for k in A.SWEEP_KS]) < R.SKIP_CAP, (d, f, bf16)


@pytest.mark.parametrize("d, route", R.SHAPE_WIDTHS)
def test_the_threshold_cases_are_admissible(d, route):
    case = R.base_case(d, 0, 1, n_items=A.BIG_ITEMS)
    ref = case.ref(_tab(case, route))
    full = (0, A.BIG_ITEMS + 1)
    for kind in A.FILTERS:
        rows = A.union_rows(A.filter_mask(kind, A.BIG_ITEMS, d), [0] * A.B)
        assert _share(ref, [(k, *full, True, rows) for k in A.BIG_KS]) < R.SKIP_CAP, (d, route, kind)


@pytest.mark.parametrize("d, route", A.RANGE_WIDTHS)
def test_the_alignment_group_and_composition_cases_are_admissible(d, route):
    case = R.base_case(d)
    ref = case.ref(_tab(case, route))
    calls = []
    for edge in A.EDGES:
        rows = A.union_rows(A.edge_mask(edge, A.N_ITEMS), [0] * A.B)
        calls += [(100, lo, hi, True, rows) for lo, hi in R.ranges()]
    assert _share(ref, calls) < R.SKIP_CAP
    group = [b % 3 for b in range(A.B)]
    for n in (A.N_ITEMS, A.BIG_ITEMS):
        case = R.base_case(d, 0, 1 if n == A.BIG_ITEMS else 0, n_items=n)
        ref = case.ref(_tab(case, route))
        full = (0, n + 1)
        rows = A.union_rows(A.group_masks(n), group)
        assert _share(ref, [(100, *full, True, rows)]) < R.SKIP_CAP, n
        x = R.exclusion_rows(ref, *full, n, d)
        both = A.union_rows(A.filter_mask("random_0.5", n, d), [0] * A.B, x)
        assert _share(ref, [(100, *full, True, both), (100, *full, False, both)]) < R.SKIP_CAP, n


@pytest.mark.parametrize("d, f", R.FAKE_CASES)
def test_the_side_term_cases_are_admissible(d, f):
    for n in (A.N_ITEMS, A.BIG_ITEMS):
        case = R.base_case(d, f, 1 if n == A.BIG_ITEMS else 0, n_items=n)
        for bf16 in (False, True):
            ref = case.ref(R.bf16_round(case.table) if bf16 else None)
            both = A.union_rows(A.filter_mask("random_0.5", n, d), [0] * A.B, R.exclusion_rows(ref, 0, n + 1, n, d))
            assert _share(ref, [(100, 0, n + 1, True, both)]) < R.SKIP_CAP, (d, f, n, bf16)


@pytest.mark.parametrize("d, route", A.FALLBACK_CASES)
def test_the_fallback_cases_are_admissible_and_overflow(d, route):
    m = A.fallback_mask(A.BIG_ITEMS)
    assert int(m.sum()) > A.CAPACITY and not m[0] and m[1]
    z = A.zero_user_case(d, A.BIG_ITEMS)
    ref = z.ref(_tab(z, route))
    rows = A.union_rows(m, [0] * z.B)
    for k in (100, 1024):
        assert R.skip_share(ref, k, 0, A.BIG_ITEMS + 1, True, rows) < R.SKIP_CAP, (d, route, k)
        idx, val = R.topk_ref(ref.s, k, 0, A.BIG_ITEMS + 1, True, rows)
        assert (idx[1] == np.nonzero(m)[0][:k]).all() and (val[1] == 0.0).all() and (val[0] != 0.0).all()
    two = A.without_user(z, 1)
    assert two.B == 2 and (two.hidden[1] == z.hidden[2]).all()


def test_the_filters_are_what_the_gpu_file_says():
    n = A.BIG_ITEMS
    assert A.filter_mask("block", n).sum() == 18_000 > A.CAPACITY and A.filter_mask("block300", n).sum() == 300 < 1024
    assert A.filter_mask("all", n).all() and not A.filter_mask("none", n).any()
    assert abs(A.filter_mask("random_0.5", n).mean() - 0.5) < 0.02 and abs(A.filter_mask("random_0.05", n).mean() - 0.05) < 0.01
    assert -(-(n + 1) // 256) == 79 and n + 1 > A.CAPACITY
    for e in A.EDGES:
        m = A.edge_mask(e, A.N_ITEMS)
        assert not m[:e].any() and m[e:e + 4].all()
    g = A.group_masks(A.N_ITEMS)
    assert g.shape == (3, A.N_ITEMS + 1) and len({int(r.sum()) for r in g}) == 3
    rows = A.union_rows(g, [0, 1, 2, 0], [np.array([5]), np.array([], np.int64), np.array([7, 7]), np.array([1])])
    assert len(rows) == 4 and 5 in rows[0] and set(np.nonzero(~g[1])[0]) == set(rows[1].tolist())
