"""CPU: the item filters' fifth header and fifth ctypes table, their exports, refusals and host queries, and the arguments of
``ItemFilter`` / ``model.topk`` / ``model.target_rank``.

include/srfrd_hip_filter.h against ``_lib.FILTER_PARAMS`` / ``_lib.FILTER_SIGNATURES``, disjoint from the other four tables; the
six symbols exported by all four libraries; every refusal of the two calls, the pack and the plan on dummy pointers (a refused
call launches nothing and touches no memory); ``srfrd_item_mask_words``; the fake impls; the routing of ``model.topk`` and
``model.target_rank`` on stand-in ops.  No GPU anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import topk_allow_refs as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS, PACK, PLAN, QUERY, TOPK, RANK = ("srfrd_item_mask_words", "srfrd_item_mask_pack", "srfrd_topk_allow_plan",
                                        "srfrd_topk_allow_workspace_bytes", "srfrd_logits_topk_allow", "srfrd_target_rank_allow")
E_ARG, E_UNSUPPORTED = -1, -2
FILTER_ARGS = ["allow_words", "n_groups", "words_per_group", "allow_group"]


def filter_header():
    """include/srfrd_hip_filter.h -> {name: (return type, [(C type without const, parameter name)])}"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_filter.h")).read()
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
def test_the_header_declares_the_six_entry_points():
    from srfrd_amd import _lib
    h = filter_header()
    assert list(h) == [WORDS, PACK, PLAN, QUERY, TOPK, RANK]
    assert h[WORDS] == ("int64_t", [("int64_t", "n_rows")])
    assert h[QUERY] == ("int64_t", [("int", "B"), ("int", "k"), ("int64_t", "n_rows")])
    assert [n for _, n in h[PACK][1]] == ["mask", "n_groups", "n_rows", "words", "stream"]
    assert [n for _, n in h[PLAN][1]] == list(_lib.WIDE_PARAMS["srfrd_topk_wide_plan"])
    for name in (WORDS, PLAN, QUERY):                                                      # host only
        assert "stream" not in [n for _, n in h[name][1]]
    wide = list(_lib.WIDE_PARAMS["srfrd_logits_topk_wide"])
    assert list(_lib.FILTER_PARAMS[TOPK]) == wide[:-1] + FILTER_ARGS + ["stream"]         # srfrd_logits_topk_wide's + the four
    rank = list(_lib.PARAMS["srfrd_target_rank"])
    assert list(_lib.FILTER_PARAMS[RANK]) == rank[:-1] + FILTER_ARGS + ["stream"]         # srfrd_target_rank's + the four
    assert "cut_k" in rank and "metric_acc" in rank


def test_filter_params_and_signatures_are_the_headers():
    from srfrd_amd import _lib
    h = filter_header()
    assert set(_lib.FILTER_PARAMS) == set(h) == set(_lib.FILTER_SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    for name, (ret, decl) in h.items():
        assert _lib.FILTER_PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.FILTER_SIGNATURES[name]
        assert res is scalars[ret] and len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            assert c_type in scalars or c_type.endswith("*"), (name, pname, c_type)
            want = scalars[c_type] if c_type in scalars else C.POINTER(_lib.Layout) if c_type == "srfrd_layout*" else C.c_void_p
            assert t is want, (name, i, pname, c_type, t)


def test_the_five_tables_are_disjoint_and_the_other_headers_stay_as_they_were():
    from srfrd_amd import _lib
    tables = (_lib.PARAMS, _lib.LAZY_PARAMS, _lib.SORT_PARAMS, _lib.WIDE_PARAMS, _lib.FILTER_PARAMS)
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    assert [len(t) for t in tables] == [61, 1, 2, 3, 6]
    for header in ("srfrd_hip.h", "srfrd_hip_lazy.h", "srfrd_hip_sort.h", "srfrd_hip_topk_wide.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "_allow" not in text and "item_mask" not in text, header


def test_the_header_states_semantics_refusals_workspace_and_launches():
    src = open(os.path.join(ROOT, "include", "srfrd_hip_filter.h")).read()
    for words in ("SRFRD_E_ARG before any launch", "SRFRD_E_UNSUPPORTED before any launch", "no memset", "captured", "-1 / -inf",
                  "equal values by ascending id", "allow_group", "clamped", "NULL: every user reads row 0", "words_per_group <",
                  "n_groups < 1", "ws_bytes", "Exact for any input", "SRFRD_EXCL_CAP", "table_bf16", "SRFRD_TOPK_FP32", "exclude_pad",
                  "fallback", "No HIP call", "no HIP call", "k r <= capacity", "SRFRD_WIDE_ALL", "ranked even when the filter disallows it", "cut_k", "metric_acc",
                  "last word", "no atomics"):
        assert words in src, words


def test_all_four_libraries_export_the_six_symbols(lib):
    import __graft_entry__ as g
    for name, (path, _, _) in g.LIBRARIES.items():
        handle = C.CDLL(path)
        for s in (WORDS, PACK, PLAN, QUERY, TOPK, RANK):
            assert hasattr(handle, s), (name, s)


def test_a_handle_typed_from_the_main_table_gets_the_filter_types_late(lib):
    from srfrd_amd import _lib
    import __graft_entry__ as g
    other = C.CDLL(g.LIBRARIES["odd"][0])
    fn = _lib._filter_entry(other, QUERY)
    assert fn.restype is C.c_int64 and tuple(fn.argtypes) == tuple(_lib.FILTER_SIGNATURES[QUERY][1])
    assert fn(4, 100, 2601) == _lib.query(QUERY, B=4, k=100, n_rows=2601) > 0


# ---- host queries -------------------------------------------------------------------------------------------------------------------
def test_item_mask_words(lib):
    from srfrd_amd import _lib
    q = lambda n: _lib.query(WORDS, n_rows=n)
    assert [q(n) for n in (1, 31, 32, 33, 2601)] == [2, 2, 2, 3, 83]
    assert q(0) == 0 and q(-5) == 0
    for n in (1, 31, 32, 33, 64, 65, 2601, 20_001):
        assert q(n) == A.words_of(n) and 32 * (q(n) - 1) >= n            # every id has its bit before the zero last word


def test_the_numpy_packing_is_the_header_layout():
    g = np.random.RandomState(0)
    for n in A.PACK_ROWS:
        m = g.random_sample((3, n)) < 0.5
        w = A.pack_ref(m)
        assert w.shape == (3, A.words_of(n)) and w.dtype == np.uint32 and (w[:, -1] == 0).all()
        for gi in range(3):
            for i in range(n):
                assert ((int(w[gi, i >> 5]) >> (i & 31)) & 1) == int(m[gi, i]), (n, gi, i)
            assert sum(bin(int(x)).count("1") for x in w[gi]) == int(m[gi].sum())       # no bit at or past n


def test_workspace_query_is_zero_exactly_where_its_values_refuse(lib):
    from srfrd_amd import _lib
    q = lambda B, k, n: _lib.query(QUERY, B=B, k=k, n_rows=n)
    assert q(0, 100, 101) == 0 and q(-1, 100, 101) == 0 and q(4, 0, 101) == 0 and q(4, 1025, 101) == 0 and q(4, 100, 0) == 0
    for B, k, n in ((1, 1, 1), (4, 100, 101), (17, 1024, 2601), (512, 1024, 1_000_001), (3, 64, 16_385)):
        assert q(B, k, n) >= B * A.CAPACITY * 8 + B * 8 + B * 32 * -(-n // 256) * 4, (B, k, n)
    assert q(512, 1024, 1_000_001) < 1 << 29              # 256 MB of maxima and 64 MB of lists: a fraction of the 2 GB of logits


# ---- refusals, on the host --------------------------------------------------------------------------------------------------------
def _dummy(n=64):
    return C.c_void_p(n)           # never dereferenced: the calls below must fail on the host


def _topk(layout, **over):
    from srfrd_amd import _lib
    d = _dummy()
    args = dict(lay=layout, item_table=d, dense=d, hidden=d, B=4, L=1, item_lo=0, item_hi=101, exclude_pad=1, user_label=None, k=100,
                excl_ptr=None, excl_items=None, max_row=0, topk_idx=d, topk_val=d, workspace=d, ws_bytes=1 << 40,
                excl_workspace=None, allow_words=d, n_groups=1, words_per_group=5, allow_group=None, stream=None)
    args.update(over)
    return _lib.query(TOPK, **args)


def _rank(layout, **over):
    from srfrd_amd import _lib
    d = _dummy()
    args = dict(lay=layout, item_table=d, dense=d, hidden=d, B=4, L=1, item_lo=0, item_hi=101, exclude_pad=1, user_label=None,
                targets=d, excl_ptr=None, excl_items=None, max_row=0, cut_k=10, rank=d, metric_acc=None, workspace=d,
                allow_words=d, n_groups=1, words_per_group=5, allow_group=None, stream=None)
    args.update(over)
    return _lib.query(RANK, **args)


def test_every_refusal_holds_without_a_gpu(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    assert _lib.query(WORDS, n_rows=101) == 5
    shared = (dict(B=0), dict(B=-2), dict(L=0), dict(item_lo=-1), dict(item_hi=0), dict(item_lo=50, item_hi=50), dict(item_hi=102),
              dict(allow_words=None), dict(n_groups=0), dict(n_groups=-1), dict(words_per_group=4), dict(words_per_group=0))
    for name in ("lay", "item_table", "dense", "hidden", "topk_idx", "topk_val", "workspace"):
        assert _topk(lay, **{name: None}) == E_ARG, name
    for over in shared + (dict(k=0), dict(k=-1), dict(k=1025), dict(ws_bytes=0)):
        assert _topk(lay, **over) == E_ARG, over
    need = _lib.query(QUERY, B=4, k=100, n_rows=101)
    assert need > 0 and _topk(lay, ws_bytes=need - 1) == E_ARG
    for name in ("lay", "item_table", "dense", "hidden", "targets", "rank", "workspace"):
        assert _rank(lay, **{name: None}) == E_ARG, name
    for over in shared + (dict(cut_k=0), dict(cut_k=-3)):
        assert _rank(lay, **over) == E_ARG, over
    x = dict(excl_ptr=_dummy(), excl_items=_dummy(), max_row=8, excl_workspace=_dummy())
    assert _topk(lay, **{**x, "excl_items": None}) == E_ARG
    assert _topk(lay, **{**x, "excl_workspace": None}) == E_ARG
    assert _topk(lay, **{**x, "max_row": -1}) == E_ARG
    assert _topk(lay, **{**x, "max_row": _lib.EXCL_CAP + 1}) == E_UNSUPPORTED
    xr = dict(excl_ptr=_dummy(), excl_items=_dummy(), max_row=8)
    assert _rank(lay, **{**xr, "excl_items": None}) == E_ARG and _rank(lay, **{**xr, "max_row": -1}) == E_ARG
    assert _rank(lay, **{**xr, "max_row": _lib.EXCL_CAP + 1}) == E_UNSUPPORTED
    srfrn = _lib.make_layout("SRFRN", 100, 20, 45, 5, 3, 2, 1)
    assert _topk(srfrn, user_label=None) == E_ARG and _rank(srfrn, user_label=None) == E_ARG
    big = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    big.D = 65
    assert _topk(big) == E_UNSUPPORTED and _rank(big) == E_UNSUPPORTED
    # the pack
    d = _dummy()
    pack = lambda **o: _lib.query(PACK, **{**dict(mask=d, n_groups=1, n_rows=101, words=d, stream=None), **o})
    for over in (dict(mask=None), dict(words=None), dict(n_groups=0), dict(n_rows=0), dict(n_rows=-1)):
        assert pack(**over) == E_ARG, over
    assert pack(n_rows=(1 << 31) - 1024) == E_UNSUPPORTED


def test_the_plan_refuses_what_the_call_refuses(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    ok = _lib.topk_allow_plan(lay, 4, 100, 0, 101)
    assert not isinstance(ok, int) and ok[1] == (A.ALL, A.CAPACITY, 0)
    for over in (dict(B=0), dict(k=0), dict(k=1025), dict(item_lo=-1), dict(item_hi=0), dict(item_hi=102), dict(n_cu=0)):
        args = dict(B=4, k=100, item_lo=0, item_hi=101, n_cu=256)
        args.update(over)
        assert _lib.topk_allow_plan(lay, **args) == E_ARG, over
    base = dict(B=4, k=100, item_lo=0, item_hi=101, excl=0, switches=0, n_cu=256, names=None, name_len=0, geom=None, sizes=None)
    assert _lib.query(PLAN, lay=None, max_launches=8, **base) == E_ARG
    assert _lib.query(PLAN, lay=lay, max_launches=-1, **base) == E_ARG
    assert _lib.query(PLAN, lay=lay, max_launches=0, **base) == len(ok[0])          # names, geom and sizes may be NULL
    big = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    big.D = 65
    assert _lib.topk_allow_plan(big, 4, 100, 0, 101) == E_UNSUPPORTED


# ---- the torch layer ----------------------------------------------------------------------------------------------------------------
def test_fake_impls_give_shapes_and_dtypes(lib):
    import srfrd_amd
    from srfrd_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "logits_topk_allow" in ops.OPS and "target_rank_allow" in ops.OPS
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    key = ops.register_model(m)
    with FakeTensorMode():
        h = torch.empty(6, 1, 50, device="meta")
        words = torch.empty(2, 5, dtype=torch.int32, device="meta")
        grp = torch.empty(6, dtype=torch.int64, device="meta")
        xp = torch.empty(7, dtype=torch.int64, device="meta")
        xi = torch.empty(11, dtype=torch.int32, device="meta")
        tg = torch.empty(6, dtype=torch.int64, device="meta")
        idx, val = torch.ops.srfrd.logits_topk_allow(h, None, key, 0, 101, 300, True, xp, xi, 3, words, grp)
        idx2, _ = torch.ops.srfrd.logits_topk_allow(h, None, key, 0, 101, 10, True, None, None, 0, words, None)
        rank = torch.ops.srfrd.target_rank_allow(h, None, tg, key, 0, 101, True, None, None, 0, words, None)
    assert tuple(idx.shape) == (6, 300) and idx.dtype == torch.int64 and tuple(val.shape) == (6, 300) and val.dtype == torch.float32
    assert tuple(idx2.shape) == (6, 10) and tuple(rank.shape) == (6,) and rank.dtype == torch.int32


class _StandIn:
    """what srfrd_amd.filters.ItemFilter holds, without the device: the argument checks of the model methods need no GPU"""

    def __new__(cls, n_items, n_groups):
        from srfrd_amd.filters import ItemFilter
        f = ItemFilter.__new__(ItemFilter)
        f.n_items, f.n_groups, f.counts = n_items, n_groups, torch.zeros(n_groups, dtype=torch.int64)
        f.words = torch.zeros(n_groups, A.words_of(n_items + 1), dtype=torch.int32)
        return f


def test_item_filter_refuses_a_mask_of_another_catalog():
    import srfrd_amd
    for shape in ((100,), (2, 102), (2, 3, 101), (0, 101)):
        with pytest.raises(ValueError, match="n_items \\+ 1"):
            srfrd_amd.ItemFilter(torch.ones(shape, dtype=torch.bool), 100, "cpu")
    with pytest.raises(ValueError, match="bool or integer"):
        srfrd_amd.ItemFilter(torch.ones(101), 100, "cpu")
    with pytest.raises(ValueError, match="ROCm GPU"):             # nothing is launched on host memory
        srfrd_amd.ItemFilter(torch.ones(101, dtype=torch.bool), 100, "cpu")
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    with pytest.raises(ValueError, match="n_items \\+ 1"):
        m.item_filter(torch.ones(100, dtype=torch.bool))


def test_model_methods_route_and_refuse(lib, monkeypatch):
    import srfrd_amd
    from srfrd_amd import modules
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    hidden = torch.zeros(3, 1, 50)
    calls = []

    class Ops:
        def __getattr__(self, name):
            def op(*args):
                calls.append((name, args))
                return [torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, 1)] if "topk" in name else torch.zeros(3, dtype=torch.int32)
            return op

    class Torch:
        class ops:
            srfrd = Ops()
        no_grad, as_tensor, int64 = torch.no_grad, staticmethod(torch.as_tensor), torch.int64

    monkeypatch.setattr(m, "_rank_inputs", lambda input_ids, fake_ids, exclude=None: (hidden, None, (None, None, 0)))
    monkeypatch.setattr(modules, "torch", Torch)
    ids, tg = torch.zeros(3, 20, dtype=torch.int64), torch.tensor([1, 2, 3])
    one, three = _StandIn(100, 1), _StandIn(100, 3)
    grp = torch.tensor([0, 2, 1])
    for k in (1, 64, 65, 1024):                                      # with a filter every k goes to the filtered op
        m.topk(None, ids, None, k=k, allow=one)
        name, args = calls[-1]
        assert name == "logits_topk_allow" and args[3:7] == (0, 101, k, True) and args[-2] is one.words and args[-1] is None
    m.topk(None, ids, None, k=10, allow=three, allow_group=grp, item_range=(3, 90), exclude_pad=False)
    name, args = calls[-1]
    assert name == "logits_topk_allow" and args[3:7] == (3, 90, 10, False) and args[-2] is three.words and torch.equal(args[-1], grp)
    m.target_rank(None, ids, None, tg, allow=three, allow_group=grp)
    name, args = calls[-1]
    assert name == "target_rank_allow" and args[-2] is three.words and torch.equal(args[-1], grp)
    m.target_rank(None, ids, None, tg, allow=one)
    assert calls[-1][0] == "target_rank_allow" and calls[-1][1][-1] is None
    n = len(calls)
    m.topk(None, ids, None, k=10)                                    # without one, today's ops
    m.target_rank(None, ids, None, tg)
    assert [c[0] for c in calls[n:]] == ["logits_topk", "target_rank"]
    n = len(calls)
    for call in (lambda **kw: m.topk(None, ids, None, k=10, **kw), lambda **kw: m.target_rank(None, ids, None, tg, **kw)):
        with pytest.raises(ValueError, match="allow_group is required"):
            call(allow=three)
        with pytest.raises(ValueError, match="int64 tensor of shape"):
            call(allow=three, allow_group=torch.tensor([0, 1]))
        with pytest.raises(ValueError, match="int64 tensor of shape"):
            call(allow=three, allow_group=torch.tensor([0, 1, 2], dtype=torch.int32))
        with pytest.raises(ValueError, match="int64 tensor of shape"):
            call(allow=one, allow_group=torch.zeros(3, 1, dtype=torch.int64))
        with pytest.raises(ValueError, match="built for n_items = 99"):
            call(allow=_StandIn(99, 1))
        with pytest.raises(ValueError, match="ItemFilter"):
            call(allow=torch.ones(101, dtype=torch.bool))
        with pytest.raises(ValueError, match="allow_group needs allow"):
            call(allow_group=grp)
    with pytest.raises(ValueError, match="TOPK_WIDE_MAX"):
        m.topk(None, ids, None, k=1025, allow=one)
    assert len(calls) == n
    with pytest.raises(TypeError):
        m.topk(None, ids, None, 10, True, None, None, one)          # keyword-only
