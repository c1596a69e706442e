"""CPU: the wide top-k's fourth header and fourth ctypes table, its exports, refusals and workspace query, and the routing of
``model.topk``.

include/srfrd_hip_topk_wide.h against ``_lib.WIDE_PARAMS`` / ``_lib.WIDE_SIGNATURES``, disjoint from the other three tables; the
three symbols exported by all four libraries; every refusal of ``srfrd_logits_topk_wide`` and ``srfrd_topk_wide_plan`` on dummy
pointers (a refused call launches nothing and touches no memory); the workspace query, 0 exactly where its values make the call
refuse; the fake impl; ``model.topk`` choosing its op by k on stand-in ops.  No GPU anywhere."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN, QUERY, ENTRY = "srfrd_topk_wide_plan", "srfrd_topk_wide_workspace_bytes", "srfrd_logits_topk_wide"
E_ARG, E_UNSUPPORTED = -1, -2


def wide_header():
    """include/srfrd_hip_topk_wide.h -> {name: (return type, [(C type without const, parameter name)])}"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_topk_wide.h")).read()
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
def test_the_header_declares_the_three_entry_points():
    h = wide_header()
    assert list(h) == [PLAN, QUERY, ENTRY]
    assert h[QUERY] == ("int64_t", [("int", "B"), ("int", "k"), ("int64_t", "n_rows")])
    assert [n for _, n in h[PLAN][1]] == ["lay", "B", "k", "item_lo", "item_hi", "excl", "switches", "n_cu", "max_launches", "names",
                                          "name_len", "geom", "sizes"]
    assert "stream" not in [n for _, n in h[PLAN][1]] + [n for _, n in h[QUERY][1]]          # host only
    from srfrd_amd import _lib
    narrow = list(_lib.PARAMS["srfrd_logits_topk_excl"])
    at = narrow.index("excl_workspace")
    assert list(_lib.WIDE_PARAMS[ENTRY]) == narrow[:at] + ["ws_bytes"] + narrow[at:]       # srfrd_logits_topk_excl's + ws_bytes
    src = open(os.path.join(ROOT, "include", "srfrd_hip_topk_wide.h")).read()
    assert re.search(r"#define\s+SRFRD_TOPK_WIDE_MAX\s+1024\b", src) and _lib.TOPK_WIDE_MAX == 1024
    import srfrd_amd
    assert srfrd_amd.TOPK_WIDE_MAX == 1024


def test_wide_params_and_signatures_are_the_headers():
    from srfrd_amd import _lib
    h = wide_header()
    assert set(_lib.WIDE_PARAMS) == set(h) == set(_lib.WIDE_SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    for name, (ret, decl) in h.items():
        assert _lib.WIDE_PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.WIDE_SIGNATURES[name]
        assert res is scalars[ret] and len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            assert c_type in scalars or c_type.endswith("*"), (name, pname, c_type)
            want = scalars[c_type] if c_type in scalars else C.POINTER(_lib.Layout) if c_type == "srfrd_layout*" else C.c_void_p
            assert t is want, (name, i, pname, c_type, t)


def test_the_four_tables_are_disjoint_and_the_other_headers_stay_as_they_were():
    from srfrd_amd import _lib
    tables = (_lib.PARAMS, _lib.LAZY_PARAMS, _lib.SORT_PARAMS, _lib.WIDE_PARAMS)
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    assert [len(t) for t in tables] == [61, 1, 2, 3]
    for header in ("srfrd_hip.h", "srfrd_hip_lazy.h", "srfrd_hip_sort.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "topk_wide" not in text, header


def test_the_header_states_semantics_refusals_workspace_and_launches():
    src = open(os.path.join(ROOT, "include", "srfrd_hip_topk_wide.h")).read()
    for words in ("SRFRD_E_ARG before any launch", "SRFRD_E_UNSUPPORTED before any launch", "no memset", "captured", "-1 / -inf",
                  "equal values by ascending id", "excl_ptr == NULL", "ws_bytes", "every score tied", "SRFRD_EXCL_CAP",
                  "table_bf16", "SRFRD_TOPK_FP32", "exclude_pad", "fallback", "no HIP call"):
        assert words in src, words


def test_all_four_libraries_export_the_three_symbols(lib):
    import __graft_entry__ as g
    for name, (path, _, _) in g.LIBRARIES.items():
        handle = C.CDLL(path)
        for s in (PLAN, QUERY, ENTRY):
            assert hasattr(handle, s), (name, s)


def test_a_handle_typed_from_the_main_table_gets_the_wide_types_late(lib):
    from srfrd_amd import _lib
    import __graft_entry__ as g
    other = C.CDLL(g.LIBRARIES["even"][0])
    fn = _lib._wide_entry(other, QUERY)
    assert fn.restype is C.c_int64 and tuple(fn.argtypes) == tuple(_lib.WIDE_SIGNATURES[QUERY][1])
    assert fn(4, 100, 2601) == _lib.query(QUERY, B=4, k=100, n_rows=2601) > 0


# ---- refusals, on the host --------------------------------------------------------------------------------------------------------
def _dummy(n=64):
    return C.c_void_p(n)           # never dereferenced: the calls below must fail on the host


def _call(layout, **over):
    from srfrd_amd import _lib
    d = _dummy()
    args = dict(lay=layout, item_table=d, dense=d, hidden=d, B=4, L=1, item_lo=0, item_hi=101, exclude_pad=1, user_label=None, k=100,
                excl_ptr=None, excl_items=None, max_row=0, topk_idx=d, topk_val=d, workspace=d, ws_bytes=1 << 40,
                excl_workspace=None, stream=None)
    args.update(over)
    return _lib.query(ENTRY, **args)


def test_every_refusal_holds_without_a_gpu(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    for name in ("lay", "item_table", "dense", "hidden", "topk_idx", "topk_val", "workspace"):
        assert _call(lay, **{name: None}) == E_ARG, name
    for over in (dict(B=0), dict(B=-2), dict(L=0), dict(k=0), dict(k=-1), dict(k=1025), dict(item_lo=-1), dict(item_hi=0),
                 dict(item_lo=50, item_hi=50), dict(item_hi=102), dict(ws_bytes=0)):
        assert _call(lay, **over) == E_ARG, over
    need = _lib.query(QUERY, B=4, k=100, n_rows=101)
    assert need > 0 and _call(lay, ws_bytes=need - 1) == E_ARG
    x = dict(excl_ptr=_dummy(), excl_items=_dummy(), max_row=8, excl_workspace=_dummy())
    assert _call(lay, **{**x, "excl_items": None}) == E_ARG
    assert _call(lay, **{**x, "excl_workspace": None}) == E_ARG
    assert _call(lay, **{**x, "max_row": -1}) == E_ARG
    assert _call(lay, **{**x, "max_row": _lib.EXCL_CAP + 1}) == E_UNSUPPORTED
    srfrn = _lib.make_layout("SRFRN", 100, 20, 45, 5, 3, 2, 1)
    assert _call(srfrn, user_label=None) == E_ARG
    # the narrow entry points keep their limit
    d = _dummy()
    assert lib.srfrd_logits_topk(C.byref(lay), d, d, d, 4, 1, 0, 101, 1, None, 65, d, d, d, None) == E_ARG


def test_the_plan_refuses_what_the_call_refuses(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    ok = _lib.topk_wide_plan(lay, 4, 100, 0, 101)
    assert not isinstance(ok, int) and ok[1][1] >= 101
    for over in (dict(B=0), dict(k=0), dict(k=1025), dict(item_lo=-1), dict(item_hi=0), dict(item_hi=102), dict(n_cu=0)):
        args = dict(B=4, k=100, item_lo=0, item_hi=101, n_cu=256)
        args.update(over)
        assert _lib.topk_wide_plan(lay, **args) == E_ARG, over
    assert _lib.query(PLAN, lay=None, B=4, k=100, item_lo=0, item_hi=101, excl=0, switches=0, n_cu=256, max_launches=8, names=None,
                      name_len=0, geom=None, sizes=None) == E_ARG
    assert _lib.query(PLAN, lay=lay, B=4, k=100, item_lo=0, item_hi=101, excl=0, switches=0, n_cu=256, max_launches=0, names=None,
                      name_len=0, geom=None, sizes=None) == len(ok[0])          # names, geom and sizes may be NULL
    big = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    big.D = 65                                            # what the narrow plan refuses, the wide plan refuses
    assert _lib.topk_wide_plan(big, 4, 100, 0, 101) == E_UNSUPPORTED == _lib.rank_plan(big, _lib.RANK_TOPK, 4, 10, 0, 101)


def test_workspace_query_is_zero_exactly_where_its_values_refuse(lib):
    from srfrd_amd import _lib
    q = lambda B, k, n: _lib.query(QUERY, B=B, k=k, n_rows=n)
    assert q(0, 100, 101) == 0 and q(-1, 100, 101) == 0 and q(4, 0, 101) == 0 and q(4, 1025, 101) == 0 and q(4, 100, 0) == 0
    for B, k, n in ((1, 1, 1), (4, 100, 101), (17, 1024, 2601), (512, 1024, 1_000_001), (3, 64, 16_385)):
        got = q(B, k, n)
        assert got >= B * 16_384 * 8 + B * 8, (B, k, n)       # B candidate lists, thresholds and cursors
    assert q(512, 1024, 1_000_001) < 1 << 30              # a fraction of the 2 GB the materialised logits take


def test_fake_impl_gives_shapes_and_dtypes(lib):
    import srfrd_amd
    from srfrd_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    key = ops.register_model(m)
    with FakeTensorMode():
        h = torch.empty(6, 1, 50, device="meta")
        xp = torch.empty(7, dtype=torch.int64, device="meta")
        xi = torch.empty(11, dtype=torch.int32, device="meta")
        idx, val = torch.ops.srfrd.logits_topk_wide(h, None, key, 0, 101, 300, True, xp, xi, 3)
        idx2, _ = torch.ops.srfrd.logits_topk_wide(h, None, key, 0, 101, 100, True, None, None, 0)
    assert tuple(idx.shape) == (6, 300) and idx.dtype == torch.int64
    assert tuple(val.shape) == (6, 300) and val.dtype == torch.float32
    assert tuple(idx2.shape) == (6, 100)


# ---- model.topk ---------------------------------------------------------------------------------------------------------------------
def test_model_topk_routes_by_k_and_names_the_limit(lib, monkeypatch):
    import srfrd_amd
    from srfrd_amd import modules
    m = srfrd_amd.SASRec(100, 20, 50, 0.0, 2, 1, "cpu")
    hidden = torch.zeros(3, 1, 50)
    calls = []

    class Ops:
        def __getattr__(self, name):
            def op(h, ulab, key, lo, hi, k, pad, *excl):
                calls.append((name, lo, hi, k, pad, excl))
                return [torch.zeros(3, k, dtype=torch.int64), torch.zeros(3, k)]
            return op

    class Torch:
        class ops:
            srfrd = Ops()
        no_grad = torch.no_grad

    xp, xi = torch.tensor([0, 1, 1, 2]), torch.tensor([5, 6], dtype=torch.int32)
    monkeypatch.setattr(m, "_rank_inputs", lambda input_ids, fake_ids, exclude=None: (hidden, None, (None, None, 0) if exclude is None
                                                                                      else (xp, xi, 1)))
    monkeypatch.setattr(modules, "torch", Torch)
    ids = torch.zeros(3, 20, dtype=torch.int64)
    m.topk(None, ids, None, k=64)
    m.topk(None, ids, None, k=64, exclude="input")
    m.topk(None, ids, None, k=65)
    m.topk(None, ids, None, k=1024, exclude="input", item_range=(3, 90), exclude_pad=False)
    assert calls == [("logits_topk", 0, 101, 64, True, ()), ("logits_topk_excl", 0, 101, 64, True, (xp, xi, 1)),
                     ("logits_topk_wide", 0, 101, 65, True, (None, None, 0)), ("logits_topk_wide", 3, 90, 1024, False, (xp, xi, 1))]
    for k in (0, -1, 1025, 5000):
        with pytest.raises(ValueError, match="srfrd_amd.TOPK_WIDE_MAX"):
            m.topk(None, ids, None, k=k)
    assert len(calls) == 4
