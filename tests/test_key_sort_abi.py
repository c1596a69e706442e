"""CPU: the device key sort's third header and third ctypes table, its refusals, its reference, and the trainer option's host side.

include/srfrd_hip_sort.h against ``_lib.SORT_PARAMS`` / ``_lib.SORT_SIGNATURES`` (the parser of tests/test_lazy_adam_abi.py's
kind), disjoint from the other two tables; the symbols exported by all four libraries; ``_lib.call`` / ``query`` by name; every
refusal of ``srfrd_sort_keys`` on dummy pointers (a refused call launches nothing and touches no memory); the workspace query over
every shape tests/test_gpu_key_sort.py uses; ``sort_refs.reference`` against ``torch.sort(stable=True)`` on the CPU, which makes it
admissible as the GPU file's yardstick; the cover of the case list; ``sort_plan`` / ``step_program`` / ``_sort_keys`` under the
option, on stand-ins.  No GPU anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import sort_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, QUERY = "srfrd_sort_keys", "srfrd_sort_keys_workspace_bytes"
E_ARG = -1
INT_MAX = 2 ** 31 - 1


def sort_header():
    """include/srfrd_hip_sort.h -> {name: (return type, [(C type without const, parameter name)])}"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip_sort.h")).read()
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


def _built():
    import __graft_entry__ as g
    g.build()
    return g


# ---- header against table -------------------------------------------------------------------------------------------------------
def test_the_sort_header_declares_the_two_entry_points_as_the_issue_spells_them():
    h = sort_header()
    assert list(h) == [QUERY, ENTRY]
    assert h[QUERY] == ("int64_t", [("int64_t", "n"), ("int64_t", "key_max")])
    assert h[ENTRY] == ("int", [("int64_t*", "keys"), ("int64_t", "n"), ("int64_t", "key_max"), ("int64_t*", "sorted_keys"),
                                ("int64_t*", "order"), ("void*", "workspace"), ("int64_t", "ws_bytes"), ("void*", "stream")])


def test_sort_params_and_signatures_are_the_sort_headers():
    from srfrd_amd import _lib
    h = sort_header()
    assert set(_lib.SORT_PARAMS) == set(h) == set(_lib.SORT_SIGNATURES)
    scalars = {"int": C.c_int, "int64_t": C.c_int64}
    for name, (ret, decl) in h.items():
        assert _lib.SORT_PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.SORT_SIGNATURES[name]
        assert res is scalars[ret], name
        assert len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            assert c_type in scalars or c_type.endswith("*"), (name, pname, c_type)
            assert t is (scalars[c_type] if c_type in scalars else C.c_void_p), (name, i, pname, c_type, t)


def test_the_three_tables_are_disjoint_and_the_other_headers_stay_without_it():
    from srfrd_amd import _lib
    for other in (_lib.PARAMS, _lib.LAZY_PARAMS, _lib.SIGNATURES, _lib.LAZY_SIGNATURES):
        assert not set(_lib.SORT_PARAMS) & set(other)
    assert len(_lib.PARAMS) == 61 and len(_lib.LAZY_PARAMS) == 1
    for header in ("srfrd_hip.h", "srfrd_hip_lazy.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "srfrd_sort_keys" not in text and "srfrd_hip_sort" not in text, header


def test_the_sort_header_states_the_contract_and_the_refusals():
    src = open(os.path.join(ROOT, "include", "srfrd_hip_sort.h")).read()
    comment = src.split("int srfrd_sort_keys(")[0]
    for words in ("SRFRD_E_ARG before any launch", "n == 0 returns 0", "permutation of [0, n)", "non-decreasing", "(stable)",
                  "sorted_keys[j] == keys[order[j]]", "16-byte", "key_max + 2", "no memset", "never waits for another workgroup",
                  "equal to each other", "2^31 - 3"):
        assert words in comment, words


# ---- exports, and the kernels' place in the build -------------------------------------------------------------------------------
def test_all_four_libraries_export_the_symbols():
    g = _built()
    assert set(g.LIBRARIES) == {"product", "skew", "even", "odd"}
    for name, (path, _, _) in g.LIBRARIES.items():
        handle = C.CDLL(path)
        for sym in (ENTRY, QUERY):
            assert hasattr(handle, sym), f"{sym} is not exported by the {name} library"


def test_the_kernels_are_a_header_of_the_optimizer_unit_with_its_widths():
    """no new translation unit; a header name the width scan splices in; launch widths the unit is pinned to; the project's barrier"""
    import __graft_entry__ as g
    from tests import skew_cases as S
    assert "srfrd_keysort.h" in g.HEADERS and not any("keysort" in s for s in g.SOURCES)
    optim = open(os.path.join(S.CSRC, "srfrd_optim.hip")).read()
    assert re.findall(r'#include "(srfrd_[a-z_]+\.h)"', optim) == ["srfrd_dev.h", "srfrd_keysort.h"]
    assert optim.index('#include "srfrd_dev.h"') < optim.index('#include "srfrd_keysort.h"')      # (the skewed __syncthreads is defined first)
    text = open(os.path.join(S.CSRC, "srfrd_keysort.h")).read()
    widths = re.findall(r"__launch_bounds__\(([^,)]+)", text)
    assert len(widths) == 3 and set(widths) == {"256"}
    assert S.launch_widths("srfrd_optim.hip") == {64, 256, 512}
    assert S.constants(text)["kSortTile"] == R.TILE
    code = re.sub(r"//[^\n]*", "", text)
    assert "__syncthreads()" in code and "s_barrier" not in code
    for word in ("atomic", "hipMemset", "hipMalloc", "while (", "__threadfence", "cooperative"):      # ranks from ballots and scans; no wait
        assert word not in code, word


# ---- marshalling ----------------------------------------------------------------------------------------------------------------
class Stand:
    """a stand-in for the library handle: every entry point returns ``rc`` and its call is kept"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if not name.startswith("srfrd_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.rc)[1]


def test_call_and_query_by_name_place_every_value(monkeypatch):
    from srfrd_amd import _lib
    stand = Stand()
    monkeypatch.setattr(_lib, "_lib", stand)
    keys, skeys, order = torch.zeros(5, dtype=torch.int64), torch.zeros(6, dtype=torch.int64), torch.zeros(7, dtype=torch.int64)
    args = dict(keys=keys, n=101, key_max=102, sorted_keys=skeys, order=order, workspace=0x4000, ws_bytes=103, stream=0x77)
    _lib.call(ENTRY, **dict(reversed(list(args.items()))))
    assert stand.calls == [(ENTRY, (keys.data_ptr(), 101, 102, skeys.data_ptr(), order.data_ptr(), 0x4000, 103, 0x77))]
    assert _lib.query(QUERY, key_max=9, n=8) == 0 and stand.calls[1] == (QUERY, (8, 9))
    with pytest.raises(TypeError, match=rf"{ENTRY}: missing \['order'\], unknown \[\]"):
        _lib.call(ENTRY, **{k: v for k, v in args.items() if k != "order"})
    with pytest.raises(TypeError, match=r"missing \[\], unknown \['no_such_parameter'\]"):
        _lib.query(QUERY, n=1, key_max=1, no_such_parameter=1)
    assert len(stand.calls) == 2
    monkeypatch.setattr(_lib, "_lib", Stand(E_ARG))
    with pytest.raises(RuntimeError, match=f"{ENTRY}: .*SRFRD_E_ARG"):
        _lib.call(ENTRY, **args)
    assert _lib.query(ENTRY, **args) == E_ARG


def test_a_handle_bound_from_the_main_table_alone_gets_the_sort_types_at_the_call(monkeypatch):
    """what tests/skew_cases.load hands out: the main table's symbols typed, these not - an address would travel as a C int"""
    g = _built()
    from srfrd_amd import _lib
    handle = C.CDLL(g.LIBRARIES["odd"][0])
    assert getattr(handle, ENTRY).argtypes is None and getattr(handle, QUERY).argtypes is None
    monkeypatch.setattr(_lib, "_lib", handle)
    big = _lib.query(QUERY, n=INT_MAX, key_max=R.KM_TOP)          # (an int64 answer: a C int would truncate it)
    assert big > 2 ** 33
    assert handle.srfrd_sort_keys_workspace_bytes.restype is C.c_int64
    assert _lib.query(ENTRY, **dict(_good(), keys=None)) == E_ARG
    assert tuple(handle.srfrd_sort_keys.argtypes) == tuple(_lib.SORT_SIGNATURES[ENTRY][1])
    assert _lib._sort_entry(handle, ENTRY) is handle.srfrd_sort_keys


# ---- the entry point's refusals ---------------------------------------------------------------------------------------------------
def _good(n=12, key_max=50_000):
    """arguments the entry point would accept - on dummy addresses: only refused calls (and n == 0) are made with them"""
    from srfrd_amd import _lib
    _built()
    return dict(keys=0x10000, n=n, key_max=key_max, sorted_keys=0x20000, order=0x30000, workspace=0x40000,
                ws_bytes=_lib.query(QUERY, n=n, key_max=key_max), stream=0)


REFUSED = ([(k, None) for k in ("keys", "sorted_keys", "order", "workspace")]
           + [("n", -1), ("n", INT_MAX + 1), ("key_max", -1), ("key_max", 2 ** 31 - 2), ("key_max", 2 ** 40),
              ("ws_bytes", "one less"), ("ws_bytes", 0), ("ws_bytes", -1), ("workspace", 0x40008), ("workspace", 0x40001),
              ("sorted_keys", 0x10000), ("order", 0x10000), ("order", 0x20000)])


@pytest.mark.parametrize("name,value", REFUSED, ids=[f"{k}={v}" for k, v in REFUSED])
def test_entry_point_refuses_with_its_code(name, value):
    from srfrd_amd import _lib
    good = _good()
    if value == "one less":
        value = good["ws_bytes"] - 1
    assert _lib.query(ENTRY, **dict(good, **{name: value})) == E_ARG


def test_entry_point_launches_nothing_for_an_empty_key_list():
    from srfrd_amd import _lib
    assert _lib.query(ENTRY, **_good(n=0)) == 0
    assert _lib.query(ENTRY, **dict(_good(n=0), order=None)) == E_ARG        # (the refusals come first)
    assert _lib.query(ENTRY, **dict(_good(n=0), workspace=0x40004)) == E_ARG


def test_the_largest_accepted_arguments_are_not_refused_by_the_query():
    from srfrd_amd import _lib
    _built()
    assert _lib.query(QUERY, n=INT_MAX, key_max=R.KM_TOP) > 0 and _lib.query(QUERY, n=0, key_max=0) > 0
    for n, km in ((-1, 5), (INT_MAX + 1, 5), (5, -1), (5, R.KM_TOP + 1)):
        assert _lib.query(QUERY, n=n, key_max=km) == 0, (n, km)


def test_workspace_query_is_positive_and_monotone_over_every_shape_the_gpu_tests_use():
    from srfrd_amd import _lib
    _built()
    ns = sorted(set(R.N_LIST) | {c[0] for c in R.OUT_OF_RANGE_CASES} | {0, 1_689_600})
    kms = sorted(set(R.KEY_MAX_LIST) | {c[1] for c in R.OUT_OF_RANGE_CASES})
    table = [[_lib.query(QUERY, n=n, key_max=km) for km in kms] for n in ns]
    for i, row in enumerate(table):
        assert all(b > 0 and b % 16 == 0 for b in row), (ns[i], row)
        assert all(a <= b for a, b in zip(row, row[1:])), (ns[i], row)                  # non-decreasing in key_max
        if i:
            assert all(a <= b for a, b in zip(table[i - 1], row)), (ns[i - 1], ns[i])      # ... and in n
    # two 8-byte pairs per key, no more than a few histogram words per tile on top
    assert 16 * 1_689_600 <= table[-1][-1] <= 17 * 1_689_600


# ---- the reference, and the case list ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_reference_is_torch_stable_sort_on_every_in_range_case(case):
    keys, skeys, order = R.case(*case)
    assert keys.min() >= 0 and keys.max() <= case[1]
    want = torch.sort(torch.from_numpy(keys.copy()), stable=True)
    assert np.array_equal(skeys, want.values.numpy()) and np.array_equal(order, want.indices.numpy())


def test_reference_puts_invalid_ids_at_the_two_ends_in_input_order():
    keys = np.array([7, -1, 2 ** 62, 0, 11, -(2 ** 40), 10, 3, 12], dtype=np.int64)
    assert R.u(keys, 10).tolist() == [8, 0, 12, 1, 12, 0, 11, 4, 12]
    skeys, order = R.reference(keys, 10)
    assert order.tolist() == [1, 5, 3, 7, 0, 6, 2, 4, 8]
    assert skeys.tolist() == [-1, -(2 ** 40), 0, 3, 7, 10, 2 ** 62, 11, 12]
    for n, km in R.OUT_OF_RANGE_CASES:
        k = R.make_out_of_range(n, km)
        bad = (k < 0) | (k > km)
        assert 0.03 * n < bad.sum() < 0.2 * n and {-1, -(1 << 40), km + 1, 1 << 62} <= set(k[bad].tolist())


def test_the_case_list_covers_every_n_and_every_key_max_twice():
    assert R.N_LIST == (1, 2, 63, 64, 65, 255, 256, 257, R.TILE - 1, R.TILE, R.TILE + 1, 3 * R.TILE + 17, 1_050_000)
    assert R.KEY_MAX_LIST == (0, 1, 5, 253, 254, 255, 65_533, 65_534, 50_000, 1_000_000, 2 ** 31 - 3)
    assert len(R.CONTENTS) == 8 and len(set(R.CASES)) == len(R.CASES)
    for n in R.N_LIST:
        assert len({c for m, _, c in R.CASES if m == n}) >= 2, n
    for km in R.KEY_MAX_LIST:
        assert len({c for _, k, c in R.CASES if k == km}) >= 2, km
    for content in R.CONTENTS:
        assert sum(c == content for _, _, c in R.CASES) >= 2, content
    assert {(n, km) for n, km, _ in R.CASES} <= {(n, km) for n in R.N_LIST for km in R.KEY_MAX_LIST}
    # the pass count changes where key_max + 2 crosses 2^8 and 2^16
    passes = {km: -(-int(km + 2).bit_length() // 8) for km in R.KEY_MAX_LIST}
    assert (passes[253], passes[254], passes[65_533], passes[65_534], passes[50_000], passes[1_000_000], passes[R.KM_TOP]) == \
        (1, 2, 2, 3, 2, 3, 4)
    assert [c[0] for c in R.SKEW_CASES] == [R.TILE + 1, R.TILE + 1, 3 * R.TILE + 17]
    # what the contents claim
    d = R.make(256, 255, "descending")
    assert (np.diff(d) < 0).all()
    o = R.make(R.TILE - 1, 65_534, "once")
    assert len(set(o.tolist())) == o.size
    h = R.make(1_050_000, 1_000_000, "hot")
    assert 0.88 < (h == np.bincount(h).argmax()).mean() < 0.92
    p = R.make(1_050_000, 50_000, "half_pad")
    assert 0.49 < (p == 0).mean() < 0.51
    assert len(set(R.make(255, 253, "alternating").tolist())) == 2


# ---- sort_plan / step_program under the option ------------------------------------------------------------------------------------
LENGTHS = (0, 2 ** 20, 2 ** 20 + 1, 1_689_600)


@pytest.mark.parametrize("mode", ["single", "allreduce", "sharded"])
def test_sort_plan_captures_the_device_sort_at_every_length(mode):
    from srfrd_amd.trainer import SORT_CAPTURE_LIMIT, sort_plan
    assert SORT_CAPTURE_LIMIT == 2 ** 20
    for n in LENGTHS:
        for use_graph in (True, False):
            assert sort_plan(mode, n, use_graph, device_sort=True) == (False, use_graph, None)
            assert sort_plan(mode, n, use_graph, True) == (False, use_graph, None)
    # without it: today's answers, positionally and by keyword
    for n in LENGTHS:
        over = n > SORT_CAPTURE_LIMIT
        for args, kw in (((mode, n), {}), ((mode, n, True), {}), ((mode, n, True, False), {}), ((mode, n), dict(device_sort=False))):
            eager_sort, use_graph, reason = sort_plan(*args, **kw)
            if mode == "single":
                assert (eager_sort, use_graph, reason) == (over, True, None)
            else:
                assert (eager_sort, use_graph) == (False, not over) and (reason is None) == (not over)


def test_step_program_runs_the_token_step_as_one_stage_under_the_device_sort():
    from srfrd_amd.trainer import FusedTrainer, step_program
    G, E, X = "graph", "eager", "collective"
    token = step_program("single", token=True, device_sort=True)
    assert token == [(G, True, ("_enqueue_ce_compute", "_sort_keys", "_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))]
    assert token == step_program("single", True, False, False, True)
    assert all(callable(getattr(FusedTrainer, name)) for name in token[0][2])
    # every other program under the option: the form without an eager sort
    assert step_program("single", lazy=True, device_sort=True) == [(G, True, ("_enqueue_lazy_step",))]
    assert step_program("single", device_sort=True) == [(G, True, ("_enqueue_compute_update",))]
    for mode in ("allreduce", "sharded"):
        assert step_program(mode, device_sort=True) == step_program(mode)
    with pytest.raises(ValueError, match="device_sort"):
        step_program("single", eager_sort=True, device_sort=True)
    with pytest.raises(ValueError, match="lazy_table"):
        step_program("single", token=True, lazy=True, device_sort=True)
    # without it: today's programs
    for kw in ({}, dict(device_sort=False)):
        assert step_program("single", **kw) == [(G, True, ("_enqueue_compute_update",))]
        assert step_program("single", True, **kw) == [(G, True, ("_enqueue_ce_compute",)), (E, False, ("_sort_keys",)),
                                                      (G, False, ("_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))]
        assert step_program("single", False, True, **kw) == [(G, True, ("_enqueue_lazy_step",))]
        assert step_program("single", False, False, True, **kw) == [
            (G, True, ("_enqueue_to_keys",)), (E, False, ("_sort_keys",)), (G, False, ("_enqueue_reduce", "_enqueue_update"))]
        assert step_program("single", False, True, True, **kw) == [
            (G, True, ("_enqueue_to_keys",)), (E, False, ("_sort_keys",)), (G, False, ("_enqueue_reduce", "_enqueue_lazy_update"))]
        assert step_program("allreduce", **kw) == [(G, True, ("_enqueue_compute",)), (X, False, ("_all_reduce_grad",)),
                                                   (G, False, ("_enqueue_update",))]
        assert [k for k, _, _ in step_program("sharded", **kw)] == [G, X, G, X, G, X, G]


def test_the_walk_hands_the_slot_to_the_pieces_that_read_one():
    """the one-stage token program on recording stubs: the compute gets the slot, the four pieces behind it none"""
    from srfrd_amd.trainer import SLOT_FREE, FusedTrainer, step_program

    class T:
        _walk, _enqueue_step = FusedTrainer._walk, FusedTrainer._enqueue_step

        def __init__(self, program):
            self.log, self._program = [], program

        def __getattr__(self, name):
            if not (name.startswith("_enqueue_") or name == "_sort_keys"):
                raise AttributeError(name)
            return lambda *a: self.log.append((name,) + a)

    t = T(step_program("single", token=True, device_sort=True))
    t._enqueue_step(1)
    assert t.log == [("_enqueue_ce_compute", 1), ("_sort_keys",), ("_enqueue_table_reduce",), ("_enqueue_ce_dense",),
                     ("_enqueue_update",)]
    # no per-slot stage of a program without the option names such a piece: its walks are what they were
    for args in (("single",), ("single", True), ("single", False, True), ("single", False, False, True), ("allreduce",), ("sharded",)):
        for _, per_slot, calls in step_program(*args):
            assert not (per_slot and set(calls) & SLOT_FREE), (args, calls)


# ---- _sort_keys -------------------------------------------------------------------------------------------------------------------
class _Lay:
    n_items = 4321


class _Sorter:
    def __init__(self, keys, sort_ws=None):
        from srfrd_amd.trainer import FusedTrainer
        self._sort = FusedTrainer._sort_keys
        self.keys = torch.tensor(keys, dtype=torch.int64)
        self.skeys, self.order = torch.full_like(self.keys, -1), torch.full_like(self.keys, -1)
        self.lay = _Lay()
        if sort_ws is not None:
            self.sort_ws = sort_ws


def test_sort_keys_takes_the_device_branch_where_the_trainer_has_a_workspace(monkeypatch):
    from srfrd_amd import _lib, trainer
    stand = Stand()
    monkeypatch.setattr(_lib, "_lib", stand)
    monkeypatch.setattr(_lib, "stream", lambda: 0x55)
    monkeypatch.setattr(trainer, "SORT_CAPTURE_LIMIT", 2)          # (over the limit: the torch branch would ask, and refuse)
    asked = []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: asked.append(1) or True)
    ws = torch.zeros(96, dtype=torch.uint8)
    s = _Sorter([3, 1, 3, 0, 1], sort_ws=ws)
    s._sort(s)
    assert stand.calls == [(ENTRY, (s.keys.data_ptr(), 5, _Lay.n_items, s.skeys.data_ptr(), s.order.data_ptr(), ws.data_ptr(), 96,
                                    0x55))]
    assert not asked and s.skeys.tolist() == [-1] * 5          # (the stand-in sorted nothing, and neither did torch)
    # without a workspace: today's sort, the host check ahead of it
    t = _Sorter([3, 1, 3, 0, 1])
    with pytest.raises(RuntimeError, match="5 keys.*must not be captured"):
        t._sort(t)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    t._sort(t)
    assert len(stand.calls) == 1 and t.skeys.tolist() == [0, 1, 1, 3, 3] and t.order.tolist() == [3, 1, 4, 0, 2]
    t.sort_ws = None                                           # (a trainer that asked for "torch", or sorts nothing)
    t.skeys.fill_(-1)
    t._sort(t)
    assert len(stand.calls) == 1 and t.skeys.tolist() == [0, 1, 1, 3, 3]


def test_the_trainer_refuses_an_unknown_key_sort_before_the_model_is_touched():
    import srfrd_amd
    from srfrd_amd.trainer import KEY_SORTS
    assert KEY_SORTS == ("torch", "device")
    for bad in ("x", "rocprim", None, True):
        with pytest.raises(ValueError, match="key_sort"):
            srfrd_amd.FusedTrainer(None, 4, 8, key_sort=bad)
    with pytest.raises(ValueError, match="lazy_table"):          # a valid value: the next refusal in line is reached
        srfrd_amd.FusedTrainer(None, 4, 8, key_sort="device", lazy_table=True, loss="softmax")


def test_key_sort_is_no_part_of_the_checkpoint():
    import inspect
    from srfrd_amd.trainer import FusedTrainer
    for fn in (FusedTrainer.state_dict, FusedTrainer._loss_signature, FusedTrainer.load_state_dict):
        assert "key_sort" not in inspect.getsource(fn) and "sort_ws" not in inspect.getsource(fn)


def test_sort_keys_function_refuses_what_is_not_a_device_key_list():
    import srfrd_amd
    with pytest.raises(ValueError, match="contiguous int64 device tensor"):
        srfrd_amd.sort_keys(torch.zeros(4, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="contiguous int64 device tensor"):
        srfrd_amd.sort_keys(torch.zeros(4, dtype=torch.int32), 5)
