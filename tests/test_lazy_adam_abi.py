"""CPU: the lazy-Adam entry point's second header and second ctypes table, its refusals, and the trainer option's host side.

include/srfrd_hip_lazy.h against ``_lib.LAZY_PARAMS`` / ``_lib.LAZY_SIGNATURES`` (a parser of this file's own), disjoint from the
main table; the symbol exported by all four libraries; ``_lib.call`` by name into a recording stand-in; every refusal of
``srfrd_table_reduce_adam`` on dummy pointers (a refused call launches nothing and touches no memory); every refusal of
``trainer._lazy_config``; ``step_program``'s present results unchanged beside the lazy form.  No GPU anywhere."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "srfrd_table_reduce_adam"
E_ARG = -1


def lazy_header():
    """include/srfrd_hip_lazy.h -> {name: (return type, [(C type without const, parameter name)])}"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_lazy.h")).read()
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


# ---- header against table -------------------------------------------------------------------------------------------------------
def test_the_lazy_header_declares_the_one_entry_point_as_the_issue_spells_it():
    h = lazy_header()
    assert list(h) == [ENTRY]
    assert h[ENTRY] == ("int", [("int64_t*", "sorted_keys"), ("int64_t*", "order"), ("float*", "table_contrib"), ("int64_t", "n"),
                                ("int", "d_item"), ("int64_t", "n_rows"), ("float*", "table"), ("float*", "m"), ("float*", "v"),
                                ("double", "beta1"), ("double", "beta2"), ("double", "eps"), ("uint32_t*", "state"),
                                ("float*", "stats"), ("uint16_t*", "table_bf16"), ("void*", "stream")])


def test_lazy_params_and_signatures_are_the_lazy_headers():
    from srfrd_amd import _lib
    h = lazy_header()
    assert set(_lib.LAZY_PARAMS) == set(h) == set(_lib.LAZY_SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}
    for name, (ret, decl) in h.items():
        assert _lib.LAZY_PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.LAZY_SIGNATURES[name]
        assert res is scalars[ret], name
        assert len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            want = scalars[c_type] if c_type in scalars else C.c_void_p
            assert c_type in scalars or c_type.endswith("*"), (name, pname, c_type)
            assert t is want, (name, i, pname, c_type, t)


def test_the_two_tables_are_disjoint_and_the_main_header_stays_without_it():
    from srfrd_amd import _lib
    assert not set(_lib.LAZY_PARAMS) & set(_lib.PARAMS)
    assert not set(_lib.LAZY_SIGNATURES) & set(_lib.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    assert ENTRY not in main and "srfrd_hip_lazy" not in main


def test_the_lazy_header_says_who_advances_state_and_what_is_refused():
    """the main header's comment standard: semantics, refusals, who advances `state`"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_lazy.h")).read()
    comment = src.split("int srfrd_table_reduce_adam(")[0]
    for words in ("SRFRD_E_ARG before any launch", "NOT advanced", "n == 0 returns 0", "never\n * dereferenced", "key 0"):
        assert words in comment, words


# ---- exports --------------------------------------------------------------------------------------------------------------------
def test_all_four_libraries_export_the_symbol():
    import __graft_entry__ as g
    g.build()
    assert set(g.LIBRARIES) == {"product", "skew", "even", "odd"}
    for name, (path, _, _) in g.LIBRARIES.items():
        assert os.path.exists(path), path
        assert hasattr(C.CDLL(path), ENTRY), f"{ENTRY} is not exported by the {name} library"
    assert "srfrd_optim.hip" in g.SPLIT_SOURCES           # (compiled under each mask: the kernel is every library's own)


# ---- marshalling ----------------------------------------------------------------------------------------------------------------
class Stand:
    """a stand-in for the library handle: every entry point returns ``rc`` and its call is kept"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if not name.startswith("srfrd_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.rc)[1]


def _distinct_args():
    args, want = {}, []
    for i, (c_type, pname) in enumerate(lazy_header()[ENTRY][1]):
        if c_type.endswith("*"):
            if i % 5 == 3:
                v, w = None, ("is", None)
            elif i % 5 == 4:
                v = 0x1000 + 16 * i
                w = ("eq", v)
            else:
                v = torch.zeros(4 + i)
                w = ("eq", v.data_ptr())
        elif c_type == "double":
            v = 0.5 + i
            w = ("eq", v)
        else:
            v = 100 + i
            w = ("eq", v)
        args[pname] = v
        want.append(w)
    return args, want


def _assert_placed(got, want):
    assert len(got) == len(want)
    for i, (g, (how, w)) in enumerate(zip(got, want)):
        if how == "is":
            assert g is w, i
        else:
            assert type(g) in (int, float) and g == w, (i, g, w)


def test_call_by_name_places_every_value(monkeypatch):
    from srfrd_amd import _lib
    stand = Stand()
    monkeypatch.setattr(_lib, "_lib", stand)
    args, want = _distinct_args()
    assert sum(isinstance(v, torch.Tensor) for v in args.values()) >= 5 and any(v is None for v in args.values())
    _lib.call(ENTRY, **dict(reversed(list(args.items()))))
    assert [n for n, _ in stand.calls] == [ENTRY]
    _assert_placed(stand.calls[0][1], want)
    assert _lib.query(ENTRY, **args) == 0 and len(stand.calls) == 2
    _assert_placed(stand.calls[1][1], want)
    # a missing or an unknown name raises before the library is touched
    victim = list(args)[len(args) // 2]
    with pytest.raises(TypeError, match=rf"{ENTRY}: missing \['{victim}'\], unknown \[\]"):
        _lib.call(ENTRY, **{k: v for k, v in args.items() if k != victim})
    with pytest.raises(TypeError, match=r"missing \[\], unknown \['no_such_parameter'\]"):
        _lib.query(ENTRY, **args, no_such_parameter=1)
    assert len(stand.calls) == 2
    # a code raises through `call`, naming the entry point
    monkeypatch.setattr(_lib, "_lib", Stand(E_ARG))
    with pytest.raises(RuntimeError, match=f"{ENTRY}: .*SRFRD_E_ARG"):
        _lib.call(ENTRY, **args)
    assert _lib.query(ENTRY, **args) == E_ARG


def test_a_handle_bound_from_the_main_table_alone_gets_the_lazy_types_at_the_call():
    """what tests/skew_cases.load hands out: the main table's symbols typed, this one not - an address would travel as a C int"""
    import __graft_entry__ as g
    from srfrd_amd import _lib
    g.build()
    handle = C.CDLL(g.LIBRARIES["even"][0])
    assert getattr(handle, ENTRY).argtypes is None
    fn = _lib._lazy_entry(handle, ENTRY)
    assert fn.restype is C.c_int and tuple(fn.argtypes) == tuple(_lib.LAZY_SIGNATURES[ENTRY][1])
    assert _lib._lazy_entry(handle, ENTRY) is fn


# ---- the entry point's refusals ---------------------------------------------------------------------------------------------------
def _good():
    """arguments the entry point would accept - on dummy addresses: only refused calls are made with them"""
    p = {k: 0x10000 + 0x1000 * i for i, k in enumerate(("sorted_keys", "order", "table_contrib", "table", "m", "v", "state", "stats",
                                                        "table_bf16"))}
    return dict(p, n=12, d_item=50, n_rows=100, beta1=0.9, beta2=0.98, eps=1e-8, stream=0)


REFUSED = ([(k, None) for k in ("sorted_keys", "order", "table_contrib", "table", "m", "v", "state")]
           + [("n", -1), ("d_item", 0), ("d_item", -3), ("d_item", 65), ("n_rows", 0), ("n_rows", -5)])


@pytest.mark.parametrize("name,value", REFUSED, ids=[f"{k}={v}" for k, v in REFUSED])
def test_entry_point_refuses_with_its_code(name, value):
    import __graft_entry__ as g
    from srfrd_amd import _lib
    g.build()
    assert _lib.query(ENTRY, **dict(_good(), **{name: value})) == E_ARG


def test_entry_point_launches_nothing_for_an_empty_key_list():
    import __graft_entry__ as g
    from srfrd_amd import _lib
    g.build()
    assert _lib.query(ENTRY, **dict(_good(), n=0)) == 0
    assert _lib.query(ENTRY, **dict(_good(), n=0, stats=None, table_bf16=None)) == 0
    assert _lib.query(ENTRY, **dict(_good(), n=0, table=None)) == E_ARG        # (the refusals come first)


# ---- _lazy_config ---------------------------------------------------------------------------------------------------------------
def test_lazy_config_accepts_the_defaults_and_reads_the_option():
    from srfrd_amd.trainer import _lazy_config
    assert _lazy_config(True) is True and _lazy_config(False) is False
    # with the option off nothing is looked at
    assert _lazy_config(False, loss="softmax", shadow_gather=True, l2_emb=0.1, weight_decay=0.1, max_grad_norm=1.0) is False


LAZY_REFUSED = {"loss": dict(loss="softmax"), "loss_token": dict(loss="gbce"), "loss_sampled": dict(loss="sampled_softmax"),
                "shadow_gather": dict(shadow_gather=True), "l2_emb": dict(l2_emb=1e-3), "weight_decay": dict(weight_decay=0.01),
                "max_grad_norm": dict(max_grad_norm=1.0), "max_grad_norm_inf": dict(max_grad_norm=float("inf"))}


@pytest.mark.parametrize("case", LAZY_REFUSED)
def test_lazy_config_refuses(case):
    from srfrd_amd.trainer import _lazy_config
    kw = LAZY_REFUSED[case]
    with pytest.raises(ValueError, match="lazy_table") as e:
        _lazy_config(True, **kw)
    assert next(iter(kw)) in str(e.value)            # ... and the argument it collides with


def test_lazy_config_refuses_an_active_exchange(monkeypatch):
    from srfrd_amd import trainer
    monkeypatch.setattr(trainer, "exchange_active", lambda group=None: True)          # (what a group of two, or a forced one, answers)
    with pytest.raises(ValueError, match="lazy_table.*single rank"):
        trainer._lazy_config(True)
    assert trainer._lazy_config(False) is False


def test_the_trainer_refuses_before_anything_is_allocated():
    """FusedTrainer(lazy_table=True, ...) raises from _lazy_config ahead of every use of the model (None here)"""
    import srfrd_amd
    for kw in (dict(loss="softmax"), dict(l2_emb=0.5), dict(weight_decay=0.1), dict(max_grad_norm=2.0), dict(shadow_gather=True)):
        with pytest.raises(ValueError, match="lazy_table"):
            srfrd_amd.FusedTrainer(None, 4, 8, lazy_table=True, **kw)


# ---- step_program ----------------------------------------------------------------------------------------------------------------
def test_step_program_keeps_its_results_and_adds_the_lazy_form():
    from srfrd_amd.trainer import FusedTrainer, step_program
    G, E, X = "graph", "eager", "collective"
    assert step_program("single") == step_program("single", False) == step_program("single", False, False) == \
        [(G, True, ("_enqueue_compute_update",))]
    assert step_program("single", True) == [(G, True, ("_enqueue_ce_compute",)), (E, False, ("_sort_keys",)),
                                            (G, False, ("_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))]
    assert step_program("allreduce") == [(G, True, ("_enqueue_compute",)), (X, False, ("_all_reduce_grad",)),
                                         (G, False, ("_enqueue_update",))]
    assert step_program("sharded") == [(G, True, ("_enqueue_fwd",)), (X, False, ("_start_stats_reduce",)), (G, True, ("_enqueue_bwd",)),
                                       (X, False, ("_scatter_grad",)), (G, False, ("_enqueue_shard_update",)),
                                       (X, False, ("_gather_params",)), (G, False, ("_enqueue_shard_finish",))]
    lazy = step_program("single", lazy=True)
    assert lazy == [(G, True, ("_enqueue_lazy_step",))]
    assert all(callable(getattr(FusedTrainer, name)) for _, _, calls in lazy for name in calls)
    for mode, token in (("allreduce", False), ("sharded", False), ("single", True)):
        with pytest.raises(ValueError, match="lazy_table"):
            step_program(mode, token, lazy=True)


def test_the_lazy_step_is_compute_then_the_dense_update():
    """the lazy program's one stage on recording stubs: the single-rank compute of the slot, then the dense-only Adam tail"""
    from srfrd_amd.trainer import FusedTrainer

    class T:
        _enqueue_lazy_step = FusedTrainer._enqueue_lazy_step

        def __init__(self):
            self.log = []

        def __getattr__(self, name):
            if not name.startswith("_enqueue_"):
                raise AttributeError(name)
            return lambda *a: self.log.append((name,) + a)

    t = T()
    t._enqueue_lazy_step(1)
    assert t.log == [("_enqueue_step_compute", 1), ("_enqueue_lazy_update",)]
