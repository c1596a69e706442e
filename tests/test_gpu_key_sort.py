"""-m gpu: srfrd_sort_keys (include/srfrd_hip_sort.h), the entry point alone, in bits.

Every case of tests/sort_refs.py against ``torch.sort(stable=True)`` on the device and against the numpy reference, into outputs
pre-filled with a sentinel and through a workspace pre-filled with garbage; invalid ids mixed in; two calls on one input; two
inputs through one workspace; the call inside a graph at 1 050 000 keys, replayed on changed input; the skewed-barrier builds.
Equality is of values of int64 throughout: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

from srfrd_amd._lib import call, query
from tests import sort_refs as R

pytestmark = pytest.mark.gpu


def _workspace(n, key_max, fill=0xA5):
    nb = query("srfrd_sort_keys_workspace_bytes", n=n, key_max=key_max)
    assert nb > 0
    return torch.full((nb,), fill, device="cuda", dtype=torch.uint8)       # nothing in it needs zeroing


def _outputs(n):
    return (torch.full((n,), R.SENTINEL, device="cuda", dtype=torch.int64), torch.full((n,), R.SENTINEL, device="cuda", dtype=torch.int64))


def _sort(keys, key_max, ws=None, out=None):
    """one call on a device key list -> (sorted_keys, order) on the CPU, as numpy"""
    n = keys.numel()
    ws = _workspace(n, key_max) if ws is None else ws
    skeys, order = _outputs(n) if out is None else out
    call("srfrd_sort_keys", keys=keys, n=n, key_max=key_max, sorted_keys=skeys, order=order, workspace=ws, ws_bytes=ws.numel())
    torch.cuda.synchronize()
    return skeys.cpu().numpy(), order.cpu().numpy()


def _assert_result(got, want, keys_np, where):
    (skeys, order), (ref_skeys, ref_order) = got, want
    n = keys_np.size
    bad = np.flatnonzero(order != ref_order)
    assert bad.size == 0, f"{where}: order differs at {bad.size} of {n} positions, first {bad[:8].tolist()}: " \
                          f"{order[bad[:8]].tolist()} for {ref_order[bad[:8]].tolist()}"
    bad = np.flatnonzero(skeys != ref_skeys)
    assert bad.size == 0, f"{where}: sorted_keys differs at {bad.size} of {n} positions, first {bad[:8].tolist()}"
    assert not (skeys == R.SENTINEL).any() and not (order == R.SENTINEL).any(), where
    assert np.array_equal(np.sort(order), np.arange(n)), f"{where}: order is no permutation"


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_bits_equal_torch_stable_sort_and_the_reference(case):
    n, key_max, _ = case
    keys_np, ref_skeys, ref_order = R.case(*case)
    keys = torch.from_numpy(keys_np.copy()).cuda()
    got = _sort(keys, key_max)
    assert np.array_equal(keys.cpu().numpy(), keys_np), "the call wrote its input"
    _assert_result(got, (ref_skeys, ref_order), keys_np, "against the reference")
    want = torch.sort(keys, stable=True)               # (eager: over 2^20 keys torch's sort must not be captured, and is not)
    _assert_result(got, (want.values.cpu().numpy(), want.indices.cpu().numpy()), keys_np, "against torch.sort on the device")


def test_the_public_function_allocates_what_is_not_handed_in():
    import srfrd_amd
    n, key_max, content = 3 * R.TILE + 17, 50_000, "once"
    keys_np, ref_skeys, ref_order = R.case(n, key_max, content)
    keys = torch.from_numpy(keys_np.copy()).cuda()
    skeys, order = srfrd_amd.sort_keys(keys, key_max)
    assert np.array_equal(skeys.cpu().numpy(), ref_skeys) and np.array_equal(order.cpu().numpy(), ref_order)
    out, ws = _outputs(n), _workspace(n, key_max)
    back = srfrd_amd.sort_keys(keys.view(-1, 1), key_max, out=out, workspace=ws)
    assert back[0] is out[0] and back[1] is out[1]
    assert np.array_equal(out[0].cpu().numpy(), ref_skeys) and np.array_equal(out[1].cpu().numpy(), ref_order)
    with pytest.raises(ValueError, match="workspace"):
        srfrd_amd.sort_keys(keys, key_max, workspace=ws[:64])
    empty = srfrd_amd.sort_keys(torch.zeros(0, device="cuda", dtype=torch.int64), key_max)
    assert empty[0].numel() == 0 and empty[1].numel() == 0


@pytest.mark.parametrize("shape", R.OUT_OF_RANGE_CASES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_invalid_ids_land_at_the_two_ends_in_input_order(shape):
    n, key_max = shape
    keys_np, ref_skeys, ref_order = R.case(n, key_max, "out_of_range")
    got = _sort(torch.from_numpy(keys_np.copy()).cuda(), key_max)
    _assert_result(got, (ref_skeys, ref_order), keys_np, "invalid ids")
    uu = R.u(got[0], key_max)
    assert (np.diff(uu) >= 0).all() and uu[0] == 0 and uu[-1] == key_max + 2


def test_two_calls_on_one_input_give_the_same_bits():
    n, key_max = 1_050_000, 50_000
    keys_np, ref_skeys, ref_order = R.case(n, key_max, "half_pad")
    keys = torch.from_numpy(keys_np.copy()).cuda()
    ws = _workspace(n, key_max)
    a = _sort(keys, key_max, ws)
    b = _sort(keys, key_max, ws)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _assert_result(b, (ref_skeys, ref_order), keys_np, "second call")


def test_two_inputs_through_one_workspace_are_both_correct():
    """nothing stale is left behind: a long list of three passes, then a shorter one of two, then the long one's other content"""
    n, key_max = 3 * R.TILE + 17, 1_000_000
    ws = _workspace(n, key_max)
    for m, km, content in ((n, key_max, "alternating"), (R.TILE + 1, 50_000, "once"), (n, 254, "half_pad"), (n, 50_000, "once")):
        assert query("srfrd_sort_keys_workspace_bytes", n=m, key_max=km) <= ws.numel()
        keys_np, ref_skeys, ref_order = R.case(m, km, content) if (m, km, content) in R.CASES else R.case(m, km, content, 3)
        got = _sort(torch.from_numpy(keys_np.copy()).cuda(), km, ws)
        _assert_result(got, (ref_skeys, ref_order), keys_np, f"{m}-{km}-{content}")


def test_a_graph_holds_the_sort_of_a_list_over_the_capture_limit():
    """only the new sort is captured (never torch's over the limit: the trainer's host check stays the guard of that)"""
    from srfrd_amd.trainer import SORT_CAPTURE_LIMIT
    n, key_max = 1_050_000, 50_000
    assert n > SORT_CAPTURE_LIMIT
    inputs = [R.case(n, key_max, "half_pad"), R.case(n, key_max, "half_pad", 1), R.case(n, key_max, "half_pad", 2)]
    keys = torch.from_numpy(inputs[2][0].copy()).cuda()
    ws, (skeys, order) = _workspace(n, key_max), _outputs(n)
    args = dict(keys=keys, n=n, key_max=key_max, sorted_keys=skeys, order=order, workspace=ws, ws_bytes=ws.numel())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call("srfrd_sort_keys", **args)                  # (loads the code objects outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("srfrd_sort_keys", **args)
    for i, (keys_np, ref_skeys, ref_order) in enumerate(inputs):
        keys.copy_(torch.from_numpy(keys_np.copy()))
        skeys.fill_(R.SENTINEL)
        order.fill_(R.SENTINEL)
        ws.fill_(0x3C + i)
        g.replay()
        torch.cuda.synchronize()
        _assert_result((skeys.cpu().numpy(), order.cpu().numpy()), (ref_skeys, ref_order), keys_np, f"replay {i}")


@pytest.mark.parametrize("lib", ["even", "odd"])
def test_same_bits_under_skewed_barriers(lib):
    from tests import skew_cases as S
    assert len(R.SKEW_CASES) == 3 and all(c[0] > R.TILE for c in R.SKEW_CASES)
    inputs = [(c, torch.from_numpy(R.case(*c)[0].copy()).cuda()) for c in R.SKEW_CASES]
    product = [_sort(keys, c[1]) for c, keys in inputs]
    mask = S.libraries()[lib][2]
    with S.use(lib) as rec:
        assert rec._handle.srfrd_skew_mask(None, None) == mask != 0
        skewed = [_sort(keys, c[1]) for c, keys in inputs]
    assert {"srfrd_sort_keys", "srfrd_sort_keys_workspace_bytes"} <= rec.called
    for (c, _), a, b in zip(inputs, product, skewed):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (lib, c)
        _assert_result(b, R.case(*c)[1:], R.case(*c)[0], f"{lib} {c}")
