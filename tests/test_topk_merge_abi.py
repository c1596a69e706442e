"""CPU: the merge's sixth header and sixth ctypes table, their exports, refusals and host query, the fake impl, and the routing
of ``ShardedRanker`` on stand-in ops.

include/srfrd_hip_merge.h against ``_lib.MERGE_PARAMS`` / ``_lib.MERGE_SIGNATURES``, disjoint from the other five tables; both
symbols exported by all four libraries; every refusal on dummy pointers (a refused call launches nothing and touches no
memory); ``srfrd_topk_merge_runs_lds_bytes`` over the case list; which ops ``ShardedRanker.topk`` / ``target_rank`` call for
k <= 64, k > 64 and a filter, and what they refuse before any op.  No GPU anywhere."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import topk_allow_refs as A
from tests import topk_merge_refs as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY, MERGE = "srfrd_topk_merge_runs_lds_bytes", "srfrd_topk_merge_runs"
E_ARG, E_UNSUPPORTED = -1, -2


def merge_header():
    """include/srfrd_hip_merge.h -> {name: (return type, [(C type without const, parameter name)])}"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_merge.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"\b(int64_t|int)\s+(srfrd_\w+)\s*\(([^()]*)\)\s*;", src):
        decl = []
        for p in params.split(","):
            m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*", p)
            assert m, (name, p)
            decl.append((m.group(1) + m.group(2), m.group(3)))
        assert name not in out, name
        out[name] = (ret, decl)
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


# ---- header against table -------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_entry_points():
    h = merge_header()
    assert list(h) == [QUERY, MERGE]
    assert h[QUERY] == ("int64_t", [("int", "n_lists"), ("int", "list_len")])
    assert h[MERGE] == ("int", [("int64_t*", "cand_idx"), ("float*", "cand_val"), ("int", "B"), ("int", "n_lists"), ("int", "list_len"),
                                ("int64_t", "user_stride"), ("int64_t", "list_stride"), ("int", "k"), ("int64_t*", "topk_idx"),
                                ("float*", "topk_val"), ("int32_t*", "path"), ("void*", "stream")])


def test_merge_params_and_signatures_are_the_headers():
    from srfrd_amd import _lib
    h = merge_header()
    assert set(_lib.MERGE_PARAMS) == set(h) == set(_lib.MERGE_SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    for name, (ret, decl) in h.items():
        assert _lib.MERGE_PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.MERGE_SIGNATURES[name]
        assert res is scalars[ret] and len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            assert c_type in scalars or c_type.endswith("*"), (name, pname, c_type)
            assert t is (scalars[c_type] if c_type in scalars else C.c_void_p), (name, i, pname, c_type, t)


def test_the_six_tables_are_disjoint_and_the_other_headers_stay_as_they_were():
    from srfrd_amd import _lib
    tables = (_lib.PARAMS, _lib.LAZY_PARAMS, _lib.SORT_PARAMS, _lib.WIDE_PARAMS, _lib.FILTER_PARAMS, _lib.MERGE_PARAMS)
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    assert [len(t) for t in tables] == [61, 1, 2, 3, 6, 2]
    for header in ("srfrd_hip.h", "srfrd_hip_lazy.h", "srfrd_hip_sort.h", "srfrd_hip_topk_wide.h", "srfrd_hip_filter.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "merge_runs" not in text, header
    assert "srfrd_topk_merge" in _lib.PARAMS                     # the narrow merge stays where it was


def test_the_header_states_semantics_refusals_layout_and_the_launch():
    src = open(os.path.join(ROOT, "include", "srfrd_hip_merge.h")).read()
    for words in ("SRFRD_E_ARG before any launch", "SRFRD_E_UNSUPPORTED before any launch", "no memset", "captured", "-1 / -inf",
                  "equal values by ascending id", "-0", "user_stride", "list_stride", "(n_lists, B, list_len)", "concatenation",
                  "A valid id with value -inf is a candidate", "does not deduplicate", "NaN", "Exact for any input", "NULL (not written)",
                  "16 384", "pow2ceil", "No HIP call", "no workspace", "wide_merge_kernel", "1024 threads", "alias"):
        assert words in src, words


def test_the_build_lists_the_new_header_and_adds_no_translation_unit():
    import __graft_entry__ as g
    assert "srfrd_rank_merge.h" in g.HEADERS and any(h.endswith("srfrd_hip_merge.h") for h in g.HEADERS)
    assert not any("merge" in s for s in g.SOURCES)
    rank = open(os.path.join(g.CSRC, "srfrd_rank.hip")).read()
    assert rank.index('#include "srfrd_rank_filter.h"') < rank.index('#include "srfrd_rank_merge.h"')
    text = open(os.path.join(g.CSRC, "srfrd_rank_merge.h")).read()
    assert "__launch_bounds__(kWideBlock) wide_merge_kernel" in text


def test_all_four_libraries_export_the_two_symbols(lib):
    import __graft_entry__ as g
    assert len(g.LIBRARIES) == 4
    for name, (path, _, _) in g.LIBRARIES.items():
        handle = C.CDLL(path)
        for s in (QUERY, MERGE):
            assert hasattr(handle, s), (name, s)


def test_a_handle_typed_from_the_main_table_gets_the_merge_types_late(lib):
    from srfrd_amd import _lib
    import __graft_entry__ as g
    other = C.CDLL(g.LIBRARIES["odd"][0])
    fn = _lib._merge_entry(other, QUERY)
    assert fn.restype is C.c_int64 and tuple(fn.argtypes) == tuple(_lib.MERGE_SIGNATURES[QUERY][1])
    assert fn(8, 1000) == _lib.query(QUERY, n_lists=8, list_len=1000) == 65536
    fn = _lib._merge_entry(other, MERGE)
    assert tuple(fn.argtypes) == tuple(_lib.MERGE_SIGNATURES[MERGE][1])


# ---- the host query and the refusals ----------------------------------------------------------------------------------------------
def test_lds_bytes_over_the_case_list(lib):
    from srfrd_amd import _lib
    q = lambda S, n: _lib.query(QUERY, n_lists=S, list_len=n)
    for S, n in M.GRID:
        assert q(S, n) == M.lds_bytes(S, n) == 8 * M.slots(S, n), (S, n)
    cases = M.special_cases() + M.unsorted_cases()
    for c in cases:
        S, _, n = c.idx.shape
        assert q(S, n) == M.lds_bytes(S, n) > 0, c.name
    assert q(16, 1024) == 128 * 1024 and q(1, 1) == 8 and q(4, 1024) < 48 * 1024 < q(8, 1000)
    for S, n in ((0, 5), (5, 0), (-1, 5), (17, 1024), (16, 1025), (1, M.CAP + 1), (M.CAP + 1, 1), (2 ** 30, 2 ** 30)):
        assert q(S, n) == M.lds_bytes(S, n) == 0, (S, n)
    assert q(M.CAP, 1) == q(1, M.CAP) == 8 * M.CAP


def _merge(**over):
    from srfrd_amd import _lib
    d = C.c_void_p(64)             # never dereferenced: the calls below must fail on the host
    args = dict(cand_idx=d, cand_val=d, B=4, n_lists=8, list_len=100, user_stride=100, list_stride=400, k=100, topk_idx=d,
                topk_val=d, path=None, stream=None)
    args.update(over)
    return _lib.query(MERGE, **args)


def test_every_refusal_holds_without_a_gpu(lib):
    for name, over, code in M.REFUSALS:
        assert _merge(**over) == code, name
    for over in (dict(B=-1), dict(n_lists=-3), dict(list_len=-1), dict(k=-1), dict(list_stride=0), dict(list_stride=-400)):
        assert _merge(**over) == E_ARG, over
    # an argument error is reported before the size is looked at
    assert _merge(n_lists=17, list_len=1024, list_stride=1024, k=0) == E_ARG
    assert _merge(n_lists=17, list_len=1024, list_stride=1023) == E_ARG


# ---- the torch layer ----------------------------------------------------------------------------------------------------------------
def test_fake_impl_gives_shapes_and_dtypes(lib):
    import srfrd_amd
    from srfrd_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "topk_merge_runs" in ops.OPS and "topk_merge" in ops.OPS
    assert "topk_merge_runs" in srfrd_amd.__all__ and callable(srfrd_amd.topk_merge_runs)
    with FakeTensorMode():
        ci = torch.empty(8, 6, 300, dtype=torch.int64, device="meta")
        cv = torch.empty(8, 6, 300, device="meta")
        idx, val, path = torch.ops.srfrd.topk_merge_runs(ci, cv, 1000)
    assert tuple(idx.shape) == (6, 1000) and idx.dtype == torch.int64 and tuple(val.shape) == (6, 1000) and val.dtype == torch.float32
    assert tuple(path.shape) == (6,) and path.dtype == torch.int32
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        srfrd_amd.topk_merge_runs(torch.zeros(2, 1, 3, dtype=torch.int64), torch.zeros(2, 1, 3), 2)


class _StandIn:
    """what srfrd_amd.filters.ItemFilter holds, without the device"""

    def __new__(cls, n_items, n_groups):
        from srfrd_amd.filters import ItemFilter
        f = ItemFilter.__new__(ItemFilter)
        f.n_items, f.n_groups, f.counts = n_items, n_groups, torch.zeros(n_groups, dtype=torch.int64)
        f.words = torch.zeros(n_groups, A.words_of(n_items + 1), dtype=torch.int32)
        return f


@pytest.fixture
def standin(lib, monkeypatch):
    """a CPU model whose ranking inputs are given, and ``torch.ops.srfrd`` replaced by a recorder inside srfrd_amd.ranker"""
    import srfrd_amd
    from srfrd_amd import ranker
    I, B = 100, 3
    m = srfrd_amd.SASRec(I, 20, 50, 0.0, 2, 1, "cpu")
    hidden = torch.zeros(B, 1, 50)
    calls = []

    class Ops:
        def __getattr__(self, name):
            def op(*args):
                calls.append((name, args))
                if "merge" in name:
                    k = args[2]
                    out = [torch.zeros(B, k, dtype=torch.int64), torch.zeros(B, k)]
                    return out + [torch.zeros(B, dtype=torch.int32)] if name == "topk_merge_runs" else out
                if "topk" in name:
                    return [torch.zeros(B, args[5], dtype=torch.int64), torch.zeros(B, args[5])]
                return torch.ones(B, dtype=torch.int32)
            return op

    class Torch:
        class ops:
            srfrd = Ops()
        no_grad, as_tensor, int64, int32, stack, cat, zeros = (torch.no_grad, staticmethod(torch.as_tensor), torch.int64, torch.int32,
                                                               staticmethod(torch.stack), staticmethod(torch.cat), staticmethod(torch.zeros))

    monkeypatch.setattr(m, "_rank_inputs", lambda input_ids, fake_ids, exclude=None: (hidden, None, (None, None, 0)))
    monkeypatch.setattr(ranker, "torch", Torch)
    monkeypatch.setattr(ranker, "topk_merge", lambda ci, cv, k: tuple(Torch.ops.srfrd.topk_merge(ci, cv, k)))
    monkeypatch.setattr(ranker, "topk_merge_runs", lambda ci, cv, k: tuple(Torch.ops.srfrd.topk_merge_runs(ci, cv, k)))
    return m, calls, torch.zeros(B, 20, dtype=torch.int64)


def test_sharded_ranker_routes(standin):
    import srfrd_amd
    m, calls, ids = standin
    r = srfrd_amd.ShardedRanker(m, n_shards=3)
    names = lambda: [c[0] for c in calls]
    r.topk(None, ids, None, k=5)                                     # today's ops, in today's order
    assert names() == ["logits_topk"] * 3 + ["topk_merge"]
    assert [c[1][3:5] for c in calls[:3]] == list(r.shards) and tuple(calls[-1][1][0].shape) == (3, 15)
    del calls[:]
    r.topk(None, ids, None, k=64, exclude="input")
    assert names() == ["logits_topk_excl"] * 3 + ["topk_merge"]
    del calls[:]
    idx, val = r.topk(None, ids, None, k=65)
    assert names() == ["logits_topk_wide"] * 3 + ["topk_merge_runs"] and tuple(idx.shape) == (3, 65)
    assert [c[1][3:6] for c in calls[:3]] == [(lo, hi, 65) for lo, hi in r.shards]
    assert tuple(calls[-1][1][0].shape) == (3, 3, 65) and calls[-1][1][2] == 65          # the (shards, B, k) stack
    one, two = _StandIn(100, 1), _StandIn(100, 2)
    grp = torch.tensor([0, 1, 1])
    for k in (5, 100):
        del calls[:]
        r.topk(None, ids, None, k=k, allow=one)
        assert names() == ["logits_topk_allow"] * 3 + ["topk_merge_runs"], k
        for (_, args), (lo, hi) in zip(calls[:3], r.shards):
            assert args[3:7] == (lo, hi, k, True) and args[-2] is one.words and args[-1] is None     # the whole bitmap, every shard
        del calls[:]
        r.topk(None, ids, None, k=k, allow=two, allow_group=grp, exclude_pad=False)
        assert names() == ["logits_topk_allow"] * 3 + ["topk_merge_runs"]
        assert all(a[6] is False and a[-2] is two.words and torch.equal(a[-1], grp) for _, a in calls[:3])
    del calls[:]
    rank = r.target_rank(None, ids, None, torch.tensor([1, 2, 3]), allow=two, allow_group=grp)
    assert names() == ["target_rank_allow"] * 3 and rank.tolist() == [3, 3, 3]           # the shards' counts add up
    assert all(a[-2] is two.words and torch.equal(a[-1], grp) and a[4:6] == sh for (_, a), sh in zip(calls, r.shards))
    del calls[:]
    r.target_rank(None, ids, None, torch.tensor([1, 2, 3]))
    assert names() == ["target_rank"] * 3
    del calls[:]
    srfrd_amd.ShardedRanker(m, n_shards=1).topk(None, ids, None, k=1024)
    assert names() == ["logits_topk_wide", "topk_merge_runs"]


def test_sharded_ranker_refuses_before_any_op(standin):
    import srfrd_amd
    m, calls, ids = standin
    r = srfrd_amd.ShardedRanker(m, n_shards=3)
    one, three = _StandIn(100, 1), _StandIn(100, 3)
    grp, tg = torch.tensor([0, 2, 1]), torch.tensor([1, 2, 3])
    for call in (lambda **kw: r.topk(None, ids, None, k=10, **kw), lambda **kw: r.topk(None, ids, None, k=100, **kw),
                 lambda **kw: r.target_rank(None, ids, None, tg, **kw)):
        with pytest.raises(ValueError, match="allow_group is required"):
            call(allow=three)
        with pytest.raises(ValueError, match="int64 tensor of shape"):
            call(allow=three, allow_group=torch.tensor([0, 1]))
        with pytest.raises(ValueError, match="built for n_items = 99"):
            call(allow=_StandIn(99, 1))
        with pytest.raises(ValueError, match="ItemFilter"):
            call(allow=torch.ones(101, dtype=torch.bool))
        with pytest.raises(ValueError, match="allow_group needs allow"):
            call(allow_group=grp)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="TOPK_WIDE_MAX"):
            r.topk(None, ids, None, k=k)
        with pytest.raises(ValueError, match="TOPK_WIDE_MAX"):
            r.topk(None, ids, None, k=k, allow=one)
    with pytest.raises(TypeError):
        r.topk(None, ids, None, 10, True, True, None, one)               # keyword-only
    # too many shards for one merge launch: 17 x 1024 and 33 x 512 -> 32 768 slots; the narrow route does not care
    many = srfrd_amd.ShardedRanker(m, n_shards=17)
    with pytest.raises(ValueError, match="16384"):
        many.topk(None, ids, None, k=1024)
    with pytest.raises(ValueError, match="16384"):
        many.topk(None, ids, None, k=513, allow=one)
    with pytest.raises(ValueError, match="16384"):
        srfrd_amd.ShardedRanker(m, n_shards=33).topk_hidden(torch.zeros(3, 50), k=512)
    assert calls == []
    many.topk(None, ids, None, k=512)                                    # 32 x 512 = 16 384: fits
    assert [c[0] for c in calls] == ["logits_topk_wide"] * 17 + ["topk_merge_runs"]
    del calls[:]
    many.topk(None, ids, None, k=64)
    assert [c[0] for c in calls] == ["logits_topk"] * 17 + ["topk_merge"]
