"""CPU: the Python layer calls the C ABI by parameter name, and the table it does so by is held to include/srfrd_hip.h.

Three parts.  The HEADER against ``_lib.PARAMS`` / ``_lib.SIGNATURES``: names, order, C types and return type of every
declaration, read by a parser of this file's own.  PLACEMENT: ``_lib.call`` by name into a recording stand-in for the library
puts every value at the position the header gives that name.  The BUILDERS of the argument heads that several call sites share
(``_lib.encoder_head``, ``ops.rank_head``), driven with CPU tensors.  No GPU and no kernel launch anywhere."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER_ENTRIES = ("srfrd_encoder_fwd", "srfrd_encoder_bwd", "srfrd_encoder_fwd_sched", "srfrd_encoder_bwd_sched",
                   "srfrd_encoder_train_sched", "srfrd_encoder_train_ranked")
PLACED = ("srfrd_encoder_fwd", "srfrd_encoder_bwd_sched", "srfrd_encoder_train_ranked", "srfrd_encoder_fwd_last",
          "srfrd_logits_topk_excl", "srfrd_target_rank", "srfrd_adamw_pack_step", "srfrd_tneg_bwd")


def header():
    """include/srfrd_hip.h -> {name: (return type, [(C type, parameter name)])}: comments stripped, one regular expression per
    declaration; a type keeps its ``*`` and loses ``const``"""
    src = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
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


def ctype_of(c_type, lib):
    """the ctypes type(s) SIGNATURES may hold for a C type of the header: a scalar's own; the two structures' pointer types;
    any other pointer c_void_p - or, for the host out-parameters the helpers of _lib fill by reference, the typed pointer"""
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}
    if c_type in scalars:
        return (scalars[c_type],)
    assert c_type.endswith("*"), c_type
    structs = {"srfrd_layout*": lib.Layout, "srfrd_optim_opts*": lib.OptimOpts}
    if c_type in structs:
        return (C.POINTER(structs[c_type]),)
    typed = {"int64_t*": C.c_int64, "int32_t*": C.c_int32}
    return (C.c_void_p,) + ((C.POINTER(typed[c_type]),) if c_type in typed else ())


def test_header_parser_reads_every_declaration():
    h = header()
    assert len(h) == 61
    assert h["srfrd_sched_ints"] == ("int64_t", [("int", "B")])
    assert h["srfrd_step_begin_sched"][1] == [("uint32_t*", "state"), ("srfrd_optim_opts*", "opts"), ("void*", "stream")]


def test_params_and_signatures_are_the_headers():
    from srfrd_amd import _lib
    h = header()
    assert set(_lib.PARAMS) == set(h) == set(_lib.SIGNATURES)
    for name, (ret, decl) in h.items():
        assert _lib.PARAMS[name] == tuple(n for _, n in decl), name
        res, types = _lib.SIGNATURES[name]
        assert res is {"int": C.c_int, "int64_t": C.c_int64}[ret], name
        assert len(types) == len(decl), name
        for i, ((c_type, pname), t) in enumerate(zip(decl, types)):
            assert any(t is ok for ok in ctype_of(c_type, _lib)), (name, i, pname, c_type, t)


def test_the_six_encoder_entries_share_the_head():
    from srfrd_amd import _lib
    h = header()
    heads = {tuple(n for _, n in h[e][1][:22]) for e in ENCODER_ENTRIES}
    assert len(heads) == 1
    head = heads.pop()
    assert head[0] == "lay" and head[-1] == "save_aux" and _lib.ENCODER_HEAD == head
    for e in ENCODER_ENTRIES:
        assert _lib.PARAMS[e][:22] == head


# ---- placement ---------------------------------------------------------------------------------------------------------------
class Stand:
    """a stand-in for the library handle: every entry point returns ``rc`` and its call is kept"""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if not name.startswith("srfrd_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.rc)[1]


@pytest.fixture
def stand(monkeypatch):
    from srfrd_amd import _lib
    s = Stand()
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def distinct_args(name):
    """one distinct value per parameter of the header's declaration -> ({name: value}, [what must arrive at position i])"""
    from srfrd_amd import _lib
    args, want = {}, []
    for i, (c_type, pname) in enumerate(header()[name][1]):
        if c_type == "srfrd_layout*":
            v = _lib.Layout()
            w = ("struct", C.addressof(v))
        elif c_type == "srfrd_optim_opts*":
            v = _lib.OptimOpts()
            w = ("struct", C.addressof(v))
        elif c_type.endswith("*"):
            if i % 5 == 3:                       # some pointers are absent,
                v, w = None, ("is", None)
            elif i % 5 == 4:                     # some are an address worked out by the caller,
                v = 0x1000 + 16 * i
                w = ("eq", v)
            else:                                # the others a tensor of their own
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


def assert_placed(got, want, name):
    assert len(got) == len(want), name
    for i, (g, (how, w)) in enumerate(zip(got, want)):
        if how == "is":
            assert g is w, (name, i)
        elif how == "struct":
            assert C.addressof(g._obj) == w, (name, i)
        else:
            assert type(g) in (int, float) and g == w, (name, i, g, w)


@pytest.mark.parametrize("name", PLACED)
def test_every_name_lands_at_the_headers_position(name, stand):
    from srfrd_amd import _lib
    args, want = distinct_args(name)
    tensors = [v.data_ptr() for v in args.values() if isinstance(v, torch.Tensor)]
    assert len(set(tensors)) == len(tensors) > 0
    # given in reverse: the order of the keywords means nothing
    _lib.call(name, **dict(reversed(list(args.items()))))
    assert [n for n, _ in stand.calls] == [name]
    assert_placed(stand.calls[0][1], want, name)
    assert _lib.query(name, **args) == 0 and len(stand.calls) == 2
    assert_placed(stand.calls[1][1], want, name)


@pytest.mark.parametrize("name", PLACED)
def test_missing_and_unknown_names_raise_before_the_library(name, stand):
    from srfrd_amd import _lib
    args, _ = distinct_args(name)
    victim = list(args)[len(args) // 2]
    with pytest.raises(TypeError, match=rf"{name}: missing \['{victim}'\], unknown \[\]"):
        _lib.call(name, **{k: v for k, v in args.items() if k != victim})
    with pytest.raises(TypeError, match=r"missing \[\], unknown \['no_such_parameter'\]"):
        _lib.call(name, **args, no_such_parameter=1)
    with pytest.raises(TypeError, match="no_such_parameter"):
        _lib.query(name, **args, no_such_parameter=1)
    assert stand.calls == []


def test_function_is_resolved_on_the_handle_at_every_call(stand):
    from srfrd_amd import _lib
    args, want = distinct_args("srfrd_adamw_pack_step")
    _lib.call("srfrd_adamw_pack_step", **args)
    seen = []
    stand.srfrd_adamw_pack_step = lambda *a: (seen.append(a), 0)[1]      # (as bench.time_kernels wraps an entry point)
    _lib.call("srfrd_adamw_pack_step", **args)
    assert len(stand.calls) == 1 and len(seen) == 1
    assert_placed(seen[0], want, "srfrd_adamw_pack_step")


def test_nonzero_return_raises_naming_the_entry(monkeypatch):
    from srfrd_amd import _lib
    args, _ = distinct_args("srfrd_tneg_bwd")
    for rc, what in ((-1, "SRFRD_E_ARG"), (-2, "SRFRD_E_UNSUPPORTED"), (700, "hipError_t 700")):
        monkeypatch.setattr(_lib, "_lib", Stand(rc))
        with pytest.raises(RuntimeError, match=f"srfrd_tneg_bwd: .*{what}"):
            _lib.call("srfrd_tneg_bwd", **args)
        assert _lib.query("srfrd_tneg_bwd", **args) == rc


# ---- builders ----------------------------------------------------------------------------------------------------------------
def test_encoder_head_builder():
    from srfrd_amd import _lib
    lay = _lib.Layout()
    flat, table16, packed = torch.zeros(64), torch.zeros(8, dtype=torch.int16), torch.zeros(16)
    ids = [torch.zeros(2, 3, dtype=torch.int64) for _ in range(6)]
    out = [torch.zeros(5 + i) for i in range(6)]
    pair = (lay, _lib.ptr(table16))                      # what a model's _table_args() gives with the bf16 shadow in use
    head = _lib.encoder_head(pair, flat, 12, packed, ids, 2, 3, 0.25, 7, out, seed=0x1_2345_6789)
    assert tuple(head) == tuple(n for _, n in header()["srfrd_encoder_fwd"][1][:22])
    assert head["lay"] is lay and head["item_table"] is pair[1] and head["item_table"].value == table16.data_ptr()
    assert head["dense"] == flat.data_ptr() + 4 * 12 == _lib.dense_ptr(flat, 12)
    assert head["packed"] is packed
    for k, t in zip(("input_ids", "fake_ids", "pos_ids", "pos_fake", "neg_ids", "neg_fake"), ids):
        assert head[k] is t
    assert (head["B"], head["L"], head["dropout_p"], head["seq_index0"]) == (2, 3, 0.25, 7)
    assert head["seed"] == 0x2345_6789 and head["seed_dev"] is None
    for k, t in zip(("hidden", "pos_logits", "neg_logits", "save_x", "save_h1", "save_aux"), out):
        assert head[k] is t
    # the seed as a device word; absent target planes take their logits with them
    word = flat.data_ptr() + 8
    head = _lib.encoder_head(pair, flat, 12, packed, [ids[0], ids[1], None, None, None, None], 2, 3, 0.0, 0, out, seed_dev=word)
    assert head["seed"] == 0 and head["seed_dev"] == word
    for k in ("pos_ids", "pos_fake", "neg_ids", "neg_fake", "pos_logits", "neg_logits"):
        assert head[k] is None
    assert head["hidden"] is out[0] and head["save_aux"] is out[5]
    head = _lib.encoder_head(pair, flat, 12, packed, [ids[0], None, ids[2], None, None, None], 2, 3, 0.0, 0, out)
    assert head["pos_logits"] is out[1] and head["neg_logits"] is None


def test_encoder_head_goes_through_call(stand):
    """the head, composed with an entry point's own arguments, is a whole call: nothing missing, nothing unknown"""
    from srfrd_amd import _lib
    ids = [torch.zeros(2, 3, dtype=torch.int64) for _ in range(6)]
    out = [torch.zeros(5 + i) for i in range(6)]
    flat = torch.zeros(64)
    head = _lib.encoder_head((_lib.Layout(), flat), flat, 12, torch.zeros(16), ids, 2, 3, 0.5, 0, out, seed=9)
    _lib.call("srfrd_encoder_fwd", **head, loss_part=None, scratch=None, scratch_floats=0, dbg=None, dbg_seq=0, stream=0)
    got = stand.calls[0][1]
    names = _lib.PARAMS["srfrd_encoder_fwd"]
    assert got[names.index("item_table")] == flat.data_ptr() and got[names.index("dense")] == flat.data_ptr() + 48
    assert [got[names.index(k)] for k in ("input_ids", "pos_ids", "neg_fake")] == [ids[0].data_ptr(), ids[2].data_ptr(), ids[5].data_ptr()]
    assert got[names.index("save_aux")] == out[5].data_ptr() and got[-1] == 0


def test_rank_head_builder():
    from srfrd_amd import _lib, ops
    h = header()
    lay = _lib.Layout()
    flat, table16 = torch.zeros(64), torch.zeros(8, dtype=torch.int16)
    hidden, ulab = torch.zeros(3, 1, 10), torch.zeros(3, dtype=torch.int64)
    xp, xi = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int32)
    pair = (lay, _lib.ptr(table16))
    m = types.SimpleNamespace(_table_args=lambda: pair, _flat=flat, n_table_pad=12)      # what the builder reads of a model
    shared = ops.rank_head(m, hidden, ulab)
    assert shared == dict(lay=lay, item_table=pair[1], dense=flat.data_ptr() + 48, hidden=hidden, B=3, L=1, user_label=ulab)
    assert shared["hidden"] is hidden and shared["user_label"] is ulab and shared["lay"] is lay
    own = {"srfrd_predict_logits": {"cand", "n_cand", "cand_stride", "logits"},
           "srfrd_logits_topk": {"k", "topk_idx", "topk_val", "workspace"},
           "srfrd_logits_topk_excl": {"k", "topk_idx", "topk_val", "workspace", "excl_workspace"},
           "srfrd_target_rank": {"targets", "cut_k", "rank", "metric_acc", "workspace"}}
    heads = {"srfrd_predict_logits": shared,
             "srfrd_logits_topk": ops.rank_head(m, hidden, None, item_range=(2, 9), exclude_pad=True),
             "srfrd_logits_topk_excl": ops.rank_head(m, hidden, ulab, item_range=(2, 9), exclude_pad=False, excl=(xp, xi, 7)),
             "srfrd_target_rank": ops.rank_head(m, hidden, ulab, item_range=(0, 5), exclude_pad=True, excl=(None, None, 0))}
    for entry, head in heads.items():       # its keys are the header's: with the entry's own arguments and the stream, all of them
        assert set(head) | own[entry] | {"stream"} == {n for _, n in h[entry][1]}, entry
        assert not set(head) & own[entry]
    topk = heads["srfrd_logits_topk"]
    assert (topk["item_lo"], topk["item_hi"], topk["exclude_pad"], topk["user_label"]) == (2, 9, 1, None)
    ex = heads["srfrd_logits_topk_excl"]
    assert ex["excl_ptr"] is xp and ex["excl_items"] is xi and ex["max_row"] == 7 and ex["exclude_pad"] == 0
    tr = heads["srfrd_target_rank"]
    assert tr["excl_ptr"] is None and tr["excl_items"] is None and tr["max_row"] == 0
