"""ctypes binding of libsrfrd_hip.so (the C ABI declared in include/srfrd_hip.h).

There is no CPU fallback: if the library is missing this module raises, and every op above it fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRFRD_LIB_PATH") or os.path.join(_HERE, "lib", "libsrfrd_hip.so")

MAX_BLOCKS = 8
MAX_D = 64
LAYOUT_MASK_PAD_KEYS = 1        # SRFRD_LAYOUT_MASK_PAD_KEYS: srfrd_layout.flags, the leading pads leave the attention keys
EXCL_CAP = 4096                 # SRFRD_EXCL_CAP: most ids one row of an exclusion set may hold
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

# name -> (restype, argtypes); must list every symbol include/srfrd_hip.h declares (tests/test_abi.py checks it)
SIGNATURES = {
    "srfrd_layout_init": (_i, [_LP, _i, _i, _i, _i, _i, _i, _i, _i]),
    "srfrd_lds_bytes": (_i, [_LP, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "srfrd_scratch_floats": (_i, [_LP, _i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "srfrd_bwd_grid": (_i, [_LP, _i, _i]),
    "srfrd_debug_shape": (_i, [_LP, _i, C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "srfrd_packed_floats": (_i64, [_LP]),
    "srfrd_pack_weights": (_i, [_LP, _P, _P, _P, _d, _d, _d, _P]),
    "srfrd_encoder_fwd": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                               _P, _P, _P, _P, _P, _P, _P, _P, _i64, _P, _i, _P]),
    "srfrd_encoder_fwd_last": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _P, _P, _i64, _P]),
    "srfrd_encoder_bwd": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                               _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _P, _P, _i64, _P, _i, _P]),
    "srfrd_sched_ints": (_i64, [_i]),
    "srfrd_seq_order": (_i, [_P, _i, _i, _i, _P, _P]),
    "srfrd_encoder_plan": (_i, [_LP, _i, _i, _i, _i, _i, _i64, _P, _P, _i, _P]),
    "srfrd_encoder_fwd_sched": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                                     _P, _P, _P, _P, _P, _P, _P, _P, _i64, _P, _i, _P]),
    "srfrd_encoder_bwd_sched": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                                     _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _P, _P, _i64, _P, _i, _P]),
    "srfrd_encoder_plan_train": (_i, [_LP, _i, _i, _i, _i, _i, _i64, _P, _i, _P]),
    "srfrd_train_scratch_floats": (_i64, [_LP, _i, _i]),
    "srfrd_encoder_train_sched": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                                       _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _P, _P, _i64, _P, _i, _P]),
    "srfrd_encoder_train_ranked": (_i, [_LP, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _d, _u32, _P, _i64,
                                        _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _P, _i, _P]),
    "srfrd_table_reduce": (_i, [_P, _P, _P, _i64, _i, _P, _P]),
    "srfrd_aux_floats": (_i64, [_LP, _i, _i]),
    "srfrd_reduce_dense": (_i, [_P, _i, _i64, _P, _P, _i, _P, _P, _P]),
    "srfrd_loss_stats": (_i, [_P, _i, _P, _P, _P]),
    "srfrd_step_begin": (_i, [_P, _d, _d, _d, _P]),
    "srfrd_adam_step": (_i, [_P, _P, _P, _P, _i64, _i64, _i64, _i64, _d, _d, _d, _P, _P, _P, _i64, _P]),
    "srfrd_adam_pack_step": (_i, [_LP, _P, _P, _P, _P, _i64, _i64, _i64, _d, _d, _d, _d, _P, _P, _P, _P, _P]),
    "srfrd_step_begin_sched": (_i, [_P, _OP, _P]),
    "srfrd_grad_norm": (_i, [_P, _i64, _P, _d, _P, _P, _P]),
    "srfrd_adamw_step": (_i, [_P, _P, _P, _P, _i64, _i64, _i64, _i64, _d, _d, _d, _P, _P, _P, _P, _i64, _P]),
    "srfrd_adamw_pack_step": (_i, [_LP, _P, _P, _P, _P, _i64, _i64, _i64, _OP, _d, _P, _P, _P, _P, _P, _P]),
    "srfrd_table_to_bf16": (_i, [_P, _i64, _P, _P]),
    "srfrd_loss_finalize": (_i, [_P, _P, _P]),
    "srfrd_skew_mask": (_i, [_P, _P]),
    "srfrd_l2_norms": (_i, [_P, _P, _P, _i, _i64, _d, _P, _P, _P, _P]),
    "srfrd_l2_apply": (_i, [_P, _P, _i64, _i64, _i64, _P, _P, _P, _P]),
    "srfrd_user_labels": (_i, [_i, _P, _i, _i, _P, _P]),
    "srfrd_check_ids": (_i, [_P, _P, _P, _P, _P, _P, _i64, _i64, _i64, _P, _P]),
    "srfrd_predict_logits": (_i, [_LP, _P, _P, _P, _i, _i, _P, _i, _i64, _P, _P, _P]),
    "srfrd_topk_workspace_bytes": (_i64, [_i, _i, _i64]),
    "srfrd_logits_topk": (_i, [_LP, _P, _P, _P, _i, _i, _i64, _i64, _i, _P, _i, _P, _P, _P, _P]),
    "srfrd_topk_merge": (_i, [_P, _P, _i, _i, _i, _P, _P, _P]),
    "srfrd_excl_workspace_bytes": (_i64, [_i, _i, _i64]),
    "srfrd_logits_topk_excl": (_i, [_LP, _P, _P, _P, _i, _i, _i64, _i64, _i, _P, _i, _P, _P, _i, _P, _P, _P, _P, _P]),
    "srfrd_target_rank": (_i, [_LP, _P, _P, _P, _i, _i, _i64, _i64, _i, _P, _P, _P, _P, _i, _i, _P, _P, _P, _P]),
    "srfrd_rank_plan": (_i, [_LP, _i, _i, _i, _i64, _i64, _i, _i, _i, _i, _P, _i, _P]),
    "srfrd_eval_rank": (_i, [_P, _i, _i, _P, _P, _P]),
    "srfrd_sample_batch": (_i, [_P, _P, _P, _i, _i, _i, _i, _u32, _u32, _P, _P, _P]),
    "srfrd_xent_workspace_floats": (_i64, [_LP, _i, _i]),
    "srfrd_xent_fwd": (_i, [_LP, _P, _P, _P, _i, _i, _P, _P, _P, _P, _i64, _P]),
    "srfrd_xent_bwd": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _P, _P, _i, _P, _i64, _P]),
    "srfrd_sxent_workspace_floats": (_i64, [_LP, _i, _i, _i]),
    "srfrd_sxent_fwd": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _i, _i, _P, _P, _P, _P, _i64, _P]),
    "srfrd_sxent_bwd": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _P, _P, _i, _i, _P, _P, _P, _P, _i64, _P]),
    "srfrd_shared_negatives": (_i, [_P, _i, _i, _P, _P, _P, _P, _P, _P]),
    "srfrd_token_negatives": (_i, [_P, _P, _i, _i, _i, _P, _P, _i, _i, _i, _u32, _u32, _P, _P, _P, _P, _P, _i, _P, _P, _P]),
    "srfrd_tneg_workspace_floats": (_i64, [_LP, _i, _i, _i]),
    "srfrd_tneg_fwd": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _d, _i, _i, _i, _P, _P, _P, _P, _i64, _P]),
    "srfrd_tneg_bwd": (_i, [_LP, _P, _P, _P, _P, _P, _i, _i, _d, _i, _P, _P, _i, _i, _P, _P, _P, _P, _i64, _P]),
    "srfrd_table_reduce_rank1": (_i, [_P, _P, _P, _P, _i, _i, _i64, _i, _P, _P, _i64, _P]),
    "srfrd_table_reduce_mixed_workspace_floats": (_i64, [_i64, _i]),
    "srfrd_table_reduce_mixed": (_i, [_P, _P, _i64, _P, _i64, _P, _P, _i, _i, _i, _P, _P, _i64, _P]),
}

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
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError(f"{what}: {_ERR.get(rc, rc)}")
    raise RuntimeError(f"{what}: hipError_t {rc}")


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def make_layout(kind: str, n_items: int, max_len: int, d_item: int, d_fake: int = 0, n_labels: int = 0,
                n_blocks: int = 2, n_heads: int = 1) -> Layout:
    lay = Layout()
    check(lib().srfrd_layout_init(C.byref(lay), KINDS[kind], n_items, max_len, d_item, d_fake, n_labels, n_blocks,
                                  n_heads), "srfrd_layout_init")
    return lay


def lds_bytes(lay: Layout, L: int):
    f, b = _i64(0), _i64(0)
    check(lib().srfrd_lds_bytes(C.byref(lay), L, C.byref(f), C.byref(b)), "srfrd_lds_bytes")
    return f.value, b.value


def scratch_floats(lay: Layout, B: int, L: int):
    f, b = _i64(0), _i64(0)
    check(lib().srfrd_scratch_floats(C.byref(lay), B, L, C.byref(f), C.byref(b)), "srfrd_scratch_floats")
    return f.value, b.value


# srfrd_encoder_plan mode bits (SRFRD_PLAN_*) and switch bits (SRFRD_SW_*, keyed by the environment variable of that name)
PLAN_POS, PLAN_NEG, PLAN_CKPT, PLAN_LOSS, PLAN_DROPOUT, PLAN_FUSED_BCE, PLAN_TAPS = 1, 2, 4, 8, 16, 32, 64
SWITCHES = {"SRFRD_GENERIC": 1, "SRFRD_NO_RAGGED": 2, "SRFRD_RAGGED_FULL_ROWS": 4, "SRFRD_NO_SLOTS50": 8, "SRFRD_NO_SLOTS": 16,
            "SRFRD_NO_ROWS": 32, "SRFRD_ROWS_ALWAYS": 64}


def encoder_plan(lay: Layout, B: int, L: int, mode: int, switches: int = 0, n_cu: int = 256, scratch_floats: int = 0):
    """srfrd_encoder_plan (no GPU needed) -> ((forward kernel, grid), (backward kernel, grid)); a direction the encoder
    refuses with SRFRD_E_UNSUPPORTED reads ("", -2)."""
    fwd, bwd, grids = C.create_string_buffer(128), C.create_string_buffer(128), (C.c_int32 * 2)()
    check(lib().srfrd_encoder_plan(C.byref(lay), B, L, mode, switches, n_cu, scratch_floats, fwd, bwd, 128, grids),
          "srfrd_encoder_plan")
    return (fwd.value.decode(), grids[0]), (bwd.value.decode(), grids[1])


def encoder_plan_train(lay: Layout, B: int, L: int, mode: int, switches: int = 0, n_cu: int = 256, scratch_floats: int = 0):
    """srfrd_encoder_plan_train (no GPU needed) -> (train kernel, grid): what srfrd_encoder_train_sched launches, or ("", -2)
    where it refuses with SRFRD_E_UNSUPPORTED."""
    name, grid = C.create_string_buffer(128), C.c_int32(0)
    check(lib().srfrd_encoder_plan_train(C.byref(lay), B, L, mode, switches, n_cu, scratch_floats, name, 128, C.byref(grid)),
          "srfrd_encoder_plan_train")
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
    rc = lib().srfrd_rank_plan(C.byref(lay), op, B, k, item_lo, item_hi, int(excl), switches, n_cu, n, names, w, geom)
    if rc < 0:
        return rc
    return [(names.raw[i * w:(i + 1) * w].split(b"\0")[0].decode(), geom[3 * i], geom[3 * i + 1], geom[3 * i + 2])
            for i in range(rc)]
