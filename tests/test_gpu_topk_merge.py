"""-m gpu: srfrd::topk_merge_runs, the merge of sorted top-k lists (include/srfrd_hip_merge.h).

Every case of tests/topk_merge_refs.py against merge_runs_ref: ids equal, value bits equal, ``path`` as the case predicts (0:
the runs were merged, 1: the user's candidates were all sorted) - so the unsorted family proves that both code paths ran and
that one user's broken run does not send its neighbours to the full sort.  The (S, B, n) stack and the (B, S n) concatenation
of the same lists through their strides; dirty output buffers; a second call; a captured graph replayed after the inputs were
overwritten in place; both complementary skew libraries, loaded beside the product."""
import numpy as np
import pytest
import torch

from tests import topk_merge_refs as M

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32)


def _dev(a):
    return torch.tensor(a, device="cuda")


def _run(idx, val, k):
    """the op on device tensors -> numpy (idx, val, path)"""
    import srfrd_amd  # noqa: F401  (registers the ops)
    oi, ov, path = torch.ops.srfrd.topk_merge_runs(idx, val, k)
    return oi.cpu().numpy(), ov.cpu().numpy(), path.cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def _check(case):
    want = M.merge_runs_ref(case.idx, case.val, case.k)
    idx, val = _dev(case.idx), _dev(case.val)
    S, B, n = case.idx.shape
    got = _run(idx, val, case.k)
    assert got[0].shape == (B, case.k) and got[0].dtype == np.int64 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (case.name, "ids")
    assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32)), (case.name, "value bits")
    assert np.array_equal(got[2], case.path), (case.name, "path", got[2], case.path)
    # the same lists as a (B, S n) concatenation, read through its strides: no copy is made (the op keeps innermost stride 1)
    cat_i = idx.permute(1, 0, 2).reshape(B, S * n).contiguous()
    cat_v = val.permute(1, 0, 2).reshape(B, S * n).contiguous()
    vi, vv = cat_i.view(B, S, n).permute(1, 0, 2), cat_v.view(B, S, n).permute(1, 0, 2)
    assert vi.data_ptr() == cat_i.data_ptr() and (S == 1 or B == 1 or not vi.is_contiguous())
    other = _run(vi, vv, case.k)
    assert _same(got, other) and np.array_equal(got[2], other[2]), (case.name, "concatenated layout")
    return got


@pytest.mark.parametrize("S, n", M.GRID)
def test_grid_cases_match_the_reference_bit_for_bit(S, n):
    for case in M.grid_cases(S, n):
        _check(case)


def test_special_cases():
    for case in M.special_cases():
        _check(case)


def test_an_unsorted_run_takes_the_full_sort_and_only_its_user():
    for case in M.unsorted_cases():
        got = _check(case)
        assert got[2].tolist() == [0, 1, 0], case.name


def test_the_public_function_a_second_call_and_a_slice_of_a_wider_buffer():
    import srfrd_amd
    case = M.grid_cases(8, 100)[-1]
    want = M.merge_runs_ref(case.idx, case.val, case.k)
    idx, val = _dev(case.idx), _dev(case.val)
    a = srfrd_amd.topk_merge_runs(idx, val, case.k)
    b = srfrd_amd.topk_merge_runs(idx, val, case.k)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert _same((a[0].cpu().numpy(), a[1].cpu().numpy()), want) and not bool(a[2].any())
    # the lists as the leading 100 slots of (S, B, 128) buffers: strides (B 128, 128, 1)
    S, B, n = case.idx.shape
    wide_i = torch.full((S, B, 128), 5, device="cuda", dtype=torch.int64)
    wide_v = torch.full((S, B, 128), 1e9, device="cuda")
    wide_i[:, :, :n], wide_v[:, :, :n] = idx, val
    c = srfrd_amd.topk_merge_runs(wide_i[:, :, :n], wide_v[:, :, :n], case.k)
    assert torch.equal(a[0], c[0]) and torch.equal(_bits(a[1]), _bits(c[1]))
    with pytest.raises(RuntimeError, match="SRFRD_E_UNSUPPORTED"):
        srfrd_amd.topk_merge_runs(torch.zeros(17, 1, 1024, dtype=torch.int64, device="cuda"), torch.zeros(17, 1, 1024, device="cuda"), 10)
    with pytest.raises(RuntimeError, match="SRFRD_E_ARG"):
        srfrd_amd.topk_merge_runs(idx, val, 1025)


def test_every_output_slot_is_written_into_dirty_buffers():
    """the C call itself, on buffers full of other values, path included; NULL path: nothing else changes"""
    from srfrd_amd import _lib
    for case in (M.special_cases()[2], M.unsorted_cases()[0]):              # a user without candidates; a user on the full sort
        S, B, n = case.idx.shape
        idx, val = _dev(case.idx), _dev(case.val)
        want = M.merge_runs_ref(case.idx, case.val, case.k)
        oi = torch.full((B, case.k), 12345, device="cuda", dtype=torch.int64)
        ov = torch.full((B, case.k), 7.0, device="cuda")
        path = torch.full((B + 1,), -9, device="cuda", dtype=torch.int32)
        args = dict(cand_idx=idx, cand_val=val, B=B, n_lists=S, list_len=n, user_stride=n, list_stride=B * n, k=case.k,
                    topk_idx=oi, topk_val=ov)
        _lib.call("srfrd_topk_merge_runs", **args, path=path)
        torch.cuda.synchronize()
        assert _same((oi.cpu().numpy(), ov.cpu().numpy()), want), case.name
        assert path[:B].cpu().numpy().tolist() == case.path.tolist() and int(path[B]) == -9, case.name
        oi.fill_(3)
        ov.fill_(3.0)
        _lib.call("srfrd_topk_merge_runs", **args, path=None)
        torch.cuda.synchronize()
        assert _same((oi.cpu().numpy(), ov.cpu().numpy()), want), case.name


def test_a_captured_call_replays_on_inputs_overwritten_in_place():
    cases = [M.special_cases()[0], M.unsorted_cases()[0]]                    # both (8, 3, 1024), k = 1024: merged, then one user sorted
    assert cases[0].idx.shape == cases[1].idx.shape and cases[0].k == cases[1].k
    k = cases[0].k
    eager = [_run(_dev(c.idx), _dev(c.val), k) for c in cases]
    idx, val = _dev(cases[0].idx), _dev(cases[0].val)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.ops.srfrd.topk_merge_runs(idx, val, k)
    for c, want in list(zip(cases, eager))[::-1] + list(zip(cases, eager)):
        idx.copy_(_dev(c.idx))
        val.copy_(_dev(c.val))
        out[0].fill_(-7)
        out[1].fill_(7.0)
        out[2].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy() for t in out)
        assert _same(got, want) and np.array_equal(got[2], want[2]) and np.array_equal(got[2], c.path), c.name


def _skew_runs():
    out = []
    for case in M.grid_cases(8, 1024)[-1:] + M.grid_cases(3, 65)[-1:] + M.grid_cases(16, 1024)[:1] + M.special_cases()[:1] + M.unsorted_cases():
        out.append(_run(_dev(case.idx), _dev(case.val), case.k))
    return out


@pytest.mark.parametrize("lib", ["even", "odd"])
def test_same_bits_under_skewed_barriers(lib):
    """1024 threads and a barrier per compare-exchange step: each of the two libraries delays the half of the waves the other
    lets run"""
    from tests import skew_cases as S
    want = _skew_runs()
    mask = S.libraries()[lib][2]
    with S.use(lib) as rec:
        assert rec._handle.srfrd_skew_mask(None, None) == mask != 0
        got = _skew_runs()
    assert "srfrd_topk_merge_runs" in rec.called
    for i, (a, b) in enumerate(zip(want, got)):
        assert _same(a, b) and np.array_equal(a[2], b[2]), (lib, i)
