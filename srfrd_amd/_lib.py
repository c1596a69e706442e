"""ctypes binding of libsrfrd_hip.so (the C ABI declared in include/srfrd_hip.h and, the lazy-Adam entry point,
include/srfrd_hip_lazy.h; the device key sort, include/srfrd_hip_sort.h; the wide top-k, include/srfrd_hip_topk_wide.h; the
item filters, include/srfrd_hip_filter.h; the merge of sorted lists, include/srfrd_hip_merge.h).

There is no CPU fallback: if the library is missing this module raises, and every op above it fails loudly.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRFRD_LIB_PATH") or os.path.join(_HERE, "lib", "libsrfrd_hip.so")

MAX_BLOCKS = 8
MAX_D = 64
LAYOUT_MASK_PAD_KEYS = 1        # SRFRD_LAYOUT_MASK_PAD_KEYS: srfrd_layout.flags, the leading pads leave the attention keys
EXCL_CAP = 4096                 # SRFRD_EXCL_CAP: most ids one row of an exclusion set may hold
TOPK_WIDE_MAX = 1024            # SRFRD_TOPK_WIDE_MAX: largest k of srfrd_logits_topk_wide (include/srfrd_hip_topk_wide.h)
KINDS = {"SASRec": 0, "SRFR": 1, "SRFRN": 2, "SRFU_B": 3, "SRFU_F": 4, "SRFU_R": 5}
_ERR = {-1: "SRFRD_E_ARG (bad argument)", -2: "SRFRD_E_UNSUPPORTED (configuration outside the fused kernels: "
        "hidden width > 64, hidden width not divisible by num_heads, a debug tap of a kernel without taps, or a caller-provided "
        "scratch buffer too small for this sequence length)", -3: "SRFRD_E_DEVICE"}


class BlockOff(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("ln1_w", "ln1_b", "in_w", "in_b", "out_w", "out_b", "ln2_w", "ln2_b",
                                         "c1_w", "c1_b", "c2_w", "c2_b")]


class Layout(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("kind", "n_items", "max_len", "d_item", "d_fake", "D", "d_out", "n_labels",
                                          "n_blocks", "n_heads", "side_rows", "side_cols", "table_bf16", "flags")]
                + [("off_pos", C.c_int64), ("off_side", C.c_int64), ("blk", BlockOff * MAX_BLOCKS),
                   ("off_lc_w", C.c_int64), ("off_lc_b", C.c_int64), ("off_ll_w", C.c_int64), ("off_ll_b", C.c_int64),
                   ("n_dense", C.c_int64), ("n_table", C.c_int64)])


class OptimOpts(C.Structure):
    """srfrd_optim_opts: base rate and betas, decoupled weight decay, and the learning-rate schedule of include/srfrd_hip.h"""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("weight_decay", C.c_double),
                ("final_ratio", C.c_double), ("warmup_steps", C.c_int64), ("total_steps", C.c_int64), ("schedule", C.c_int32),
                ("reserved", C.c_int32)]


SCHEDULES = {"constant": 0, "linear": 1, "cosine": 2}      # SRFRD_SCHED_*
GRAD_NORM_PARTIALS = 1024                                  # SRFRD_GRAD_NORM_PARTIALS: doubles of srfrd_grad_norm's workspace
GRAD_NORM_SHARE = 4096                                     # SRFRD_GRAD_NORM_SHARE

_P = C.c_void_p
_i, _i64, _u32, _d = C.c_int, C.c_int64, C.c_uint32, C.c_double
_LP = C.POINTER(Layout)
_OP = C.POINTER(OptimOpts)
_TYPES = {"i": _i, "q": _i64, "u": _u32, "d": _d, "p": _P, "lay": _LP, "opt": _OP, "pq": C.POINTER(_i64), "pi": C.POINTER(C.c_int32)}

# what the six encoder entry points that run a whole forward or backward begin with (`encoder_head` builds its values)
_ENC_HEAD = ("lay:lay item_table dense packed input_ids fake_ids pos_ids pos_fake neg_ids neg_fake B:i L:i dropout_p:d seed:u "
             "seed_dev seq_index0:q hidden pos_logits neg_logits save_x save_h1 save_aux")
# THE table of the C ABI: every symbol include/srfrd_hip.h declares, its parameters in the header's order and spelling, each
# `name:type` with the types of _TYPES (a bare name: a pointer passed as void*), the return type in front.
# tests/test_call_names.py holds it to the header; SIGNATURES and PARAMS derive from it.
_ABI = f"""
i srfrd_layout_init(lay:lay kind:i n_items:i max_len:i d_item:i d_fake:i n_labels:i n_blocks:i n_heads:i)
i srfrd_lds_bytes(lay:lay L:i fwd_bytes:pq bwd_bytes:pq)
i srfrd_scratch_floats(lay:lay B:i L:i fwd_floats:pq bwd_floats:pq)
i srfrd_bwd_grid(lay:lay B:i L:i)
i srfrd_debug_shape(lay:lay L:i slot_floats:pq n_slots:pi)
q srfrd_packed_floats(lay:lay)
i srfrd_pack_weights(lay:lay dense packed state lr:d beta1:d beta2:d stream)
i srfrd_encoder_fwd({_ENC_HEAD} loss_part scratch scratch_floats:q dbg dbg_seq:i stream)
i srfrd_encoder_fwd_last(lay:lay item_table dense packed input_ids fake_ids B:i L:i hidden_last scratch scratch_floats:q stream)
i srfrd_encoder_bwd({_ENC_HEAD} d_hidden d_pos d_neg fused_bce:i grad_table table_contrib grad_slabs scratch scratch_floats:q
    dbg dbg_seq:i stream)
q srfrd_sched_ints(B:i)
i srfrd_seq_order(input_ids B:i L:i pair_stride:i sched stream)
i srfrd_encoder_plan(lay:lay B:i L:i mode:i switches:i n_cu:i scratch_floats:q fwd_name bwd_name name_len:i grids)
i srfrd_encoder_fwd_sched({_ENC_HEAD} loss_part scratch scratch_floats:q sched sched_mode:i stream)
i srfrd_encoder_bwd_sched({_ENC_HEAD} d_hidden d_pos d_neg fused_bce:i grad_table table_contrib grad_slabs scratch
    scratch_floats:q sched sched_mode:i stream)
i srfrd_encoder_plan_train(lay:lay B:i L:i mode:i switches:i n_cu:i scratch_floats:q name name_len:i grid)
q srfrd_train_scratch_floats(lay:lay B:i L:i)
i srfrd_encoder_train_sched({_ENC_HEAD} loss_part d_hidden d_pos d_neg fused_bce:i grad_table table_contrib grad_slabs scratch
    scratch_floats:q sched sched_mode:i stream)
i srfrd_encoder_train_ranked({_ENC_HEAD} loss_part fused_bce:i grad_table table_contrib grad_slabs pair_stride:i stream)
i srfrd_table_reduce(sorted_keys order table_contrib n:q d_item:i grad_table stream)
q srfrd_aux_floats(lay:lay B:i L:i)
i srfrd_reduce_dense(grad_slabs n_slabs:i n_dense:q grad_dense loss_part B:i stats loss_out stream)
i srfrd_loss_stats(loss_part B:i stats loss_out stream)
i srfrd_step_begin(state lr:d beta1:d beta2:d stream)
i srfrd_adam_step(param grad m v n:q i0:q i1:q n_zero:q beta1:d beta2:d eps:d state stats table_bf16 n_table:q stream)
i srfrd_adam_pack_step(lay:lay param grad m v n:q n_table_pad:q n_zero:q lr:d beta1:d beta2:d eps:d state stats packed
    table_bf16 stream)
i srfrd_step_begin_sched(state opts:opt stream)
i srfrd_grad_norm(grad n:q stats max_norm:d partial out stream)
i srfrd_adamw_step(param grad m v n:q i0:q i1:q n_zero:q beta1:d beta2:d eps:d state stats clip table_bf16 n_table:q stream)
i srfrd_adamw_pack_step(lay:lay param grad m v n:q n_table_pad:q n_zero:q opts:opt eps:d state stats clip packed table_bf16
    stream)
i srfrd_table_to_bf16(src n:q out stream)
i srfrd_loss_finalize(stats loss_out stream)
i srfrd_skew_mask(out_dev stream)
i srfrd_l2_norms(param seg_off seg_len n_seg:i n_table_pad:q l2_emb:d partial l2buf dense_scale stream)
i srfrd_l2_apply(grad param i0:q i1:q n_table_pad:q l2buf dense_scale stats stream)
i srfrd_user_labels(kind:i fake_ids B:i L:i labels stream)
i srfrd_check_ids(item_a item_b item_c fake_a fake_b fake_c n:q n_items:q fake_hi:q err_word stream)
i srfrd_predict_logits(lay:lay item_table dense hidden B:i L:i cand n_cand:i cand_stride:q user_label logits stream)
q srfrd_topk_workspace_bytes(B:i k:i n_rows:q)
i srfrd_logits_topk(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label k:i topk_idx topk_val
    workspace stream)
i srfrd_topk_merge(cand_idx cand_val B:i n_cand:i k:i topk_idx topk_val stream)
q srfrd_excl_workspace_bytes(B:i max_row:i n_rows:q)
i srfrd_logits_topk_excl(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label k:i excl_ptr
    excl_items max_row:i topk_idx topk_val workspace excl_workspace stream)
i srfrd_target_rank(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label targets excl_ptr
    excl_items max_row:i cut_k:i rank metric_acc workspace stream)
i srfrd_rank_plan(lay:lay op:i B:i k:i item_lo:q item_hi:q excl:i switches:i n_cu:i max_launches:i names name_len:i geom)
i srfrd_eval_rank(logits B:i n_cand:i rank metric_acc stream)
i srfrd_sample_batch(user_ptr items reviews usernum:i itemnum:i B:i L:i seed:u batch_index:u out_user out_packed stream)
q srfrd_xent_workspace_floats(lay:lay B:i L:i)
i srfrd_xent_fwd(lay:lay table hidden targets B:i L:i token_loss lse stats workspace ws_floats:q stream)
i srfrd_xent_bwd(lay:lay table hidden targets lse d_token_loss B:i L:i d_hidden grad_table accumulate:i workspace ws_floats:q
    stream)
q srfrd_sxent_workspace_floats(lay:lay B:i L:i K:i)
i srfrd_sxent_fwd(lay:lay table hidden targets negatives log_q K:i remove_hits:i B:i L:i token_loss lse stats workspace
    ws_floats:q stream)
i srfrd_sxent_bwd(lay:lay table hidden targets negatives log_q K:i remove_hits:i lse d_token_loss B:i L:i d_hidden table_contrib
    contrib_keys workspace ws_floats:q stream)
i srfrd_shared_negatives(state n_items:i K:i alias_prob alias_idx item_log_q out_ids out_log_q stream)
i srfrd_token_negatives(user_ptr items usernum:i n_items:i max_hist:i users targets B:i L:i K:i seed:u batch_index:u state
    alias_prob alias_idx item_log_q user_log_keep exclude_history:i out_ids out_log_q stream)
q srfrd_tneg_workspace_floats(lay:lay B:i L:i K:i)
i srfrd_tneg_fwd(lay:lay table hidden targets negatives log_q K:i objective:i beta:d remove_hits:i B:i L:i token_loss lse stats
    workspace ws_floats:q stream)
i srfrd_tneg_bwd(lay:lay table hidden targets negatives log_q K:i objective:i beta:d remove_hits:i lse d_token_loss B:i L:i
    d_hidden contrib_coef contrib_keys workspace ws_floats:q stream)
i srfrd_table_reduce_rank1(sorted_keys order contrib_coef hidden d_out:i rows_per_token:i n:q d_item:i grad_table workspace
    ws_floats:q stream)
q srfrd_table_reduce_mixed_workspace_floats(n:q d_item:i)
i srfrd_table_reduce_mixed(sorted_keys order n:q rows n_rows:q contrib_coef hidden d_out:i rows_per_token:i d_item:i grad_table
    workspace ws_floats:q stream)
"""
# The second table: what include/srfrd_hip_lazy.h declares, in the same notation (tests/test_lazy_adam_abi.py holds it to that
# header; LAZY_SIGNATURES and LAZY_PARAMS derive from it).  `query` / `call` consult it after the main one.
_LAZY_ABI = """
i srfrd_table_reduce_adam(sorted_keys order table_contrib n:q d_item:i n_rows:q table m v beta1:d beta2:d eps:d state stats
    table_bf16 stream)
"""
# The third table: what include/srfrd_hip_sort.h declares (tests/test_key_sort_abi.py holds it to that header; SORT_SIGNATURES and
# SORT_PARAMS derive from it).  `query` / `call` consult it after the other two.
_SORT_ABI = """
q srfrd_sort_keys_workspace_bytes(n:q key_max:q)
i srfrd_sort_keys(keys n:q key_max:q sorted_keys order workspace ws_bytes:q stream)
"""
# The fourth table: what include/srfrd_hip_topk_wide.h declares (tests/test_topk_wide_abi.py holds it to that header;
# WIDE_SIGNATURES and WIDE_PARAMS derive from it).  `query` / `call` consult it after the other three.
_WIDE_ABI = """
i srfrd_topk_wide_plan(lay:lay B:i k:i item_lo:q item_hi:q excl:i switches:i n_cu:i max_launches:i names name_len:i geom sizes)
q srfrd_topk_wide_workspace_bytes(B:i k:i n_rows:q)
i srfrd_logits_topk_wide(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label k:i excl_ptr
    excl_items max_row:i topk_idx topk_val workspace ws_bytes:q excl_workspace stream)
"""
# The fifth table: what include/srfrd_hip_filter.h declares (tests/test_topk_allow_abi.py holds it to that header;
# FILTER_SIGNATURES and FILTER_PARAMS derive from it).  `query` / `call` consult it after the other four.
_FILTER_ABI = """
q srfrd_item_mask_words(n_rows:q)
i srfrd_item_mask_pack(mask n_groups:i n_rows:q words stream)
i srfrd_topk_allow_plan(lay:lay B:i k:i item_lo:q item_hi:q excl:i switches:i n_cu:i max_launches:i names name_len:i geom sizes)
q srfrd_topk_allow_workspace_bytes(B:i k:i n_rows:q)
i srfrd_logits_topk_allow(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label k:i excl_ptr
    excl_items max_row:i topk_idx topk_val workspace ws_bytes:q excl_workspace allow_words n_groups:i words_per_group:q allow_group
    stream)
i srfrd_target_rank_allow(lay:lay item_table dense hidden B:i L:i item_lo:q item_hi:q exclude_pad:i user_label targets excl_ptr
    excl_items max_row:i cut_k:i rank metric_acc workspace allow_words n_groups:i words_per_group:q allow_group stream)
"""
# The sixth table: what include/srfrd_hip_merge.h declares (tests/test_topk_merge_abi.py holds it to that header; MERGE_SIGNATURES
# and MERGE_PARAMS derive from it).  `query` / `call` consult it after the other five.
_MERGE_ABI = """
q srfrd_topk_merge_runs_lds_bytes(n_lists:i list_len:i)
i srfrd_topk_merge_runs(cand_idx cand_val B:i n_lists:i list_len:i user_stride:q list_stride:q k:i topk_idx topk_val path stream)
"""


def _parse(params):
    pairs = [(p + ":p").split(":")[:2] for p in params.split()]
    return [_TYPES[t] for _, t in pairs], tuple(n for n, _ in pairs)


def _parse_abi(text):
    return {name: (_TYPES[res], *_parse(params)) for res, name, params in re.findall(r"(\w) (srfrd_\w+)\(([^)]*)\)", text)}


_PARSED = _parse_abi(_ABI)
SIGNATURES = {name: (res, types) for name, (res, types, _) in _PARSED.items()}      # name -> (restype, argtypes)
PARAMS = {name: names for name, (_, _, names) in _PARSED.items()}                   # name -> parameter names, in order
_LAZY_PARSED = _parse_abi(_LAZY_ABI)
LAZY_SIGNATURES = {name: (res, types) for name, (res, types, _) in _LAZY_PARSED.items()}
LAZY_PARAMS = {name: names for name, (_, _, names) in _LAZY_PARSED.items()}
_SORT_PARSED = _parse_abi(_SORT_ABI)
SORT_SIGNATURES = {name: (res, types) for name, (res, types, _) in _SORT_PARSED.items()}
SORT_PARAMS = {name: names for name, (_, _, names) in _SORT_PARSED.items()}
_WIDE_PARSED = _parse_abi(_WIDE_ABI)
WIDE_SIGNATURES = {name: (res, types) for name, (res, types, _) in _WIDE_PARSED.items()}
WIDE_PARAMS = {name: names for name, (_, _, names) in _WIDE_PARSED.items()}
_FILTER_PARSED = _parse_abi(_FILTER_ABI)
FILTER_SIGNATURES = {name: (res, types) for name, (res, types, _) in _FILTER_PARSED.items()}
FILTER_PARAMS = {name: names for name, (_, _, names) in _FILTER_PARSED.items()}
_MERGE_PARSED = _parse_abi(_MERGE_ABI)
MERGE_SIGNATURES = {name: (res, types) for name, (res, types, _) in _MERGE_PARSED.items()}
MERGE_PARAMS = {name: names for name, (_, _, names) in _MERGE_PARSED.items()}
ENCODER_HEAD = _parse(_ENC_HEAD)[1]
# name -> (its names as a set, the fetch of a dict's values in parameter order, the positions that hold a pointer)
_MARSHAL = {name: (frozenset(names), operator.itemgetter(*names) if len(names) > 1 else (lambda a, n=names[0]: (a[n],)),
                   tuple(i for i, t in enumerate(types) if t not in (_i, _i64, _u32, _d)))
            for name, (_, types, names) in {**_PARSED, **_LAZY_PARSED, **_SORT_PARSED, **_WIDE_PARSED,
                                               **_FILTER_PARSED, **_MERGE_PARSED}.items()}

_lib = None


def lib():
    """The loaded library (loads on first use; raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the SRFRD HIP kernels are not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **LAZY_SIGNATURES, **SORT_SIGNATURES, **WIDE_SIGNATURES,
                                  **FILTER_SIGNATURES, **MERGE_SIGNATURES}.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def _late_entry(handle, name, table):
    """entry point ``name`` of ``table`` (the second to the sixth) on ``handle``.  A handle that was bound from SIGNATURES alone
    (another build of the library, loaded beside the product's) gets the types here: an unbound ctypes function would take an
    address as a C int"""
    fn = getattr(handle, name)
    if getattr(fn, "argtypes", ()) is None:          # (a ctypes function nobody has typed yet)
        fn.restype, fn.argtypes = table[name]
    return fn


def _lazy_entry(handle, name):
    return _late_entry(handle, name, LAZY_SIGNATURES)


def _sort_entry(handle, name):
    return _late_entry(handle, name, SORT_SIGNATURES)


def _wide_entry(handle, name):
    return _late_entry(handle, name, WIDE_SIGNATURES)


def _filter_entry(handle, name):
    return _late_entry(handle, name, FILTER_SIGNATURES)


def _merge_entry(handle, name):
    return _late_entry(handle, name, MERGE_SIGNATURES)


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError(f"{what}: {_ERR.get(rc, rc)}")
    raise RuntimeError(f"{what}: hipError_t {rc}")


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    """the current torch stream, as the launchers' `stream` argument"""
    return torch.cuda.current_stream().cuda_stream


def dense_ptr(flat, n_table_pad):
    """address of the dense part of a flat [table | pad | dense] vector (parameters, gradient or moments)"""
    return flat.data_ptr() + 4 * n_table_pad


def query(name, /, **args):
    """The C entry point ``name`` with its parameters BY NAME (PARAMS, then LAZY_PARAMS, SORT_PARAMS, WIDE_PARAMS, FILTER_PARAMS and MERGE_PARAMS: the headers'; all of them, except that ``stream`` defaults
    to the current torch stream) -> its raw return value.  In a pointer's place a tensor passes its ``data_ptr()``, None is
    NULL, a ctypes structure goes by reference, anything else (an address as an int, a ctypes buffer) as it is.  A missing or
    unknown name raises TypeError before the library is touched; the function is looked up on the handle at every call."""
    known, fetch, pointers = _MARSHAL[name]
    if "stream" in known and "stream" not in args:
        args["stream"] = stream()
    if args.keys() != known:
        raise TypeError(f"{name}: missing {sorted(known - args.keys())}, unknown {sorted(args.keys() - known)}")
    argv = list(fetch(args))
    for i in pointers:
        v = argv[i]
        if isinstance(v, torch.Tensor):
            argv[i] = v.data_ptr()
        elif isinstance(v, C.Structure):
            argv[i] = C.byref(v)
    if name in SIGNATURES:
        return getattr(lib(), name)(*argv)
    table = next(t for t in (LAZY_SIGNATURES, SORT_SIGNATURES, WIDE_SIGNATURES, FILTER_SIGNATURES, MERGE_SIGNATURES) if name in t)
    return _late_entry(lib(), name, table)(*argv)


def call(name, /, **args):
    """``query`` for a launcher: a non-zero return raises (``check``)."""
    check(query(name, **args), name)


def encoder_head(table_args, flat, n_table_pad, packed, ids, B, L, dropout_p, seq0, out, seed=0, seed_dev=None):
    """The named values every encoder entry point begins with (ENCODER_HEAD): a model's ``_table_args()`` pair, flat vector and
    packed weights, the six id planes (None where absent; an absent target plane takes its logits with it), the dropout seed
    (host value) or ``seed_dev`` (address of its device word), the first global sequence, ``out``: the forward's six outputs."""
    out = (out[0], out[1] if ids[2] is not None else None, out[2] if ids[4] is not None else None, *out[3:])
    return dict(zip(ENCODER_HEAD, (*table_args, dense_ptr(flat, n_table_pad), packed, *ids, B, L, float(dropout_p),
                                   int(seed) & 0xFFFFFFFF, seed_dev, int(seq0), *out)))


def make_layout(kind: str, n_items: int, max_len: int, d_item: int, d_fake: int = 0, n_labels: int = 0,
                n_blocks: int = 2, n_heads: int = 1) -> Layout:
    lay = Layout()
    call("srfrd_layout_init", lay=lay, kind=KINDS[kind], n_items=n_items, max_len=max_len, d_item=d_item, d_fake=d_fake,
         n_labels=n_labels, n_blocks=n_blocks, n_heads=n_heads)
    return lay


def lds_bytes(lay: Layout, L: int):
    f, b = _i64(0), _i64(0)
    call("srfrd_lds_bytes", lay=lay, L=L, fwd_bytes=C.byref(f), bwd_bytes=C.byref(b))
    return f.value, b.value


def scratch_floats(lay: Layout, B: int, L: int):
    f, b = _i64(0), _i64(0)
    call("srfrd_scratch_floats", lay=lay, B=B, L=L, fwd_floats=C.byref(f), bwd_floats=C.byref(b))
    return f.value, b.value


# srfrd_encoder_plan mode bits (SRFRD_PLAN_*) and switch bits (SRFRD_SW_*, keyed by the environment variable of that name)
PLAN_POS, PLAN_NEG, PLAN_CKPT, PLAN_LOSS, PLAN_DROPOUT, PLAN_FUSED_BCE, PLAN_TAPS = 1, 2, 4, 8, 16, 32, 64
SWITCHES = {"SRFRD_GENERIC": 1, "SRFRD_NO_RAGGED": 2, "SRFRD_RAGGED_FULL_ROWS": 4, "SRFRD_NO_SLOTS50": 8, "SRFRD_NO_SLOTS": 16,
            "SRFRD_NO_ROWS": 32, "SRFRD_ROWS_ALWAYS": 64}


def encoder_plan(lay: Layout, B: int, L: int, mode: int, switches: int = 0, n_cu: int = 256, scratch_floats: int = 0):
    """srfrd_encoder_plan (no GPU needed) -> ((forward kernel, grid), (backward kernel, grid)); a direction the encoder
    refuses with SRFRD_E_UNSUPPORTED reads ("", -2)."""
    fwd, bwd, grids = C.create_string_buffer(128), C.create_string_buffer(128), (C.c_int32 * 2)()
    call("srfrd_encoder_plan", lay=lay, B=B, L=L, mode=mode, switches=switches, n_cu=n_cu, scratch_floats=scratch_floats,
         fwd_name=fwd, bwd_name=bwd, name_len=128, grids=grids)
    return (fwd.value.decode(), grids[0]), (bwd.value.decode(), grids[1])


def encoder_plan_train(lay: Layout, B: int, L: int, mode: int, switches: int = 0, n_cu: int = 256, scratch_floats: int = 0):
    """srfrd_encoder_plan_train (no GPU needed) -> (train kernel, grid): what srfrd_encoder_train_sched launches, or ("", -2)
    where it refuses with SRFRD_E_UNSUPPORTED."""
    name, grid = C.create_string_buffer(128), C.c_int32(0)
    call("srfrd_encoder_plan_train", lay=lay, B=B, L=L, mode=mode, switches=switches, n_cu=n_cu, scratch_floats=scratch_floats,
         name=name, name_len=128, grid=C.byref(grid))
    return name.value.decode(), grid.value


def env_switches() -> int:
    """the SRFRD_SW_* bits the launchers read from the environment right now (a switch counts when its variable is set)"""
    return sum(bit for name, bit in SWITCHES.items() if name in os.environ)


# objectives of srfrd_tneg_fwd / _bwd (SRFRD_TNEG_*) and the segment length of srfrd_table_reduce_rank1 (SRFRD_TNEG_SPLIT_ROWS)
TNEG_OBJECTIVES = {"softmax": 0, "gbce": 1}
TNEG_SPLIT_ROWS = 256
# srfrd_token_negatives: draws per slot (SRFRD_TNEG_TRIES) and the longest history its LDS set holds (SRFRD_TNEG_MAX_HIST)
TNEG_TRIES = 32
TNEG_MAX_HIST = 16384

# srfrd_rank_plan ops (SRFRD_RANK_*) and the ranking's switch bit (SRFRD_SW_TOPK_FP32: the environment variable SRFRD_TOPK_FP32)
RANK_TOPK, RANK_TARGET, RANK_TARGET_METRIC = 0, 1, 2
SW_TOPK_FP32 = 128


def rank_plan(lay: Layout, op: int, B: int, k: int, item_lo: int, item_hi: int, excl: bool = False, switches: int = 0,
              n_cu: int = 256):
    """srfrd_rank_plan (no GPU needed) -> [(kernel, workgroups, threads, dynamic LDS bytes)] in launch order, or the
    negative code the call refuses with (SRFRD_E_UNSUPPORTED, SRFRD_E_ARG)."""
    n, w = 8, 96
    names, geom = C.create_string_buffer(n * w), (C.c_int32 * (3 * n))()
    rc = query("srfrd_rank_plan", lay=lay, op=op, B=B, k=k, item_lo=item_lo, item_hi=item_hi, excl=int(excl), switches=switches,
               n_cu=n_cu, max_launches=n, names=names, name_len=w, geom=geom)
    if rc < 0:
        return rc
    return [(names.raw[i * w:(i + 1) * w].split(b"\0")[0].decode(), geom[3 * i], geom[3 * i + 1], geom[3 * i + 2])
            for i in range(rc)]


# paths of a wide top-k plan (SRFRD_WIDE_*)
WIDE_FINE, WIDE_CHUNK, WIDE_ALL = 0, 1, 2


def topk_wide_plan(lay: Layout, B: int, k: int, item_lo: int, item_hi: int, excl: bool = False, switches: int = 0,
                   n_cu: int = 256):
    """srfrd_topk_wide_plan (no GPU needed) -> ([(kernel, workgroups, threads, dynamic LDS bytes)] in launch order,
    (path, candidate capacity per user, group maxima per user)), or the negative code the call refuses with."""
    n, w = 8, 96
    names, geom, sizes = C.create_string_buffer(n * w), (C.c_int32 * (3 * n))(), (C.c_int32 * 3)()
    rc = query("srfrd_topk_wide_plan", lay=lay, B=B, k=k, item_lo=item_lo, item_hi=item_hi, excl=int(excl), switches=switches,
               n_cu=n_cu, max_launches=n, names=names, name_len=w, geom=geom, sizes=sizes)
    if rc < 0:
        return rc
    return ([(names.raw[i * w:(i + 1) * w].split(b"\0")[0].decode(), geom[3 * i], geom[3 * i + 1], geom[3 * i + 2])
             for i in range(rc)], tuple(sizes))


def topk_allow_plan(lay: Layout, B: int, k: int, item_lo: int, item_hi: int, excl: bool = False, switches: int = 0,
                    n_cu: int = 256):
    """srfrd_topk_allow_plan (no GPU needed), in the form of ``topk_wide_plan``: ([(kernel, workgroups, threads, dynamic LDS
    bytes)] in launch order, (path, candidate capacity per user, group maxima per user)), or the negative code the call
    refuses with."""
    n, w = 8, 96
    names, geom, sizes = C.create_string_buffer(n * w), (C.c_int32 * (3 * n))(), (C.c_int32 * 3)()
    rc = query("srfrd_topk_allow_plan", lay=lay, B=B, k=k, item_lo=item_lo, item_hi=item_hi, excl=int(excl), switches=switches,
               n_cu=n_cu, max_launches=n, names=names, name_len=w, geom=geom, sizes=sizes)
    if rc < 0:
        return rc
    return ([(names.raw[i * w:(i + 1) * w].split(b"\0")[0].decode(), geom[3 * i], geom[3 * i + 1], geom[3 * i + 2])
             for i in range(rc)], tuple(sizes))
