"""CPU-only: the C-ABI shared library loads and exports every symbol include/srfrd_hip.h declares; the ctypes
signature table covers exactly that set; host-side (no-GPU) entry points behave."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(srfrd_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/srfrd_hip.h but not exported"
    assert sorted(_lib.SIGNATURES) == syms, "ctypes signature table and header disagree"


def test_layout_matches_state_dict_sizes():
    from srfrd_amd import _lib
    lay = _lib.make_layout("SRFR", 1000, 20, 45, 5, 0, 2, 1)
    assert lay.n_table + lay.n_dense == 79345
    lay = _lib.make_layout("SRFRN", 1000, 20, 45, 5, 0, 2, 1)
    assert lay.n_table + lay.n_dense == 77060
    lay = _lib.make_layout("SASRec", 1000, 20, 50, 0, 0, 2, 1)
    assert lay.n_table + lay.n_dense == 82150
    assert lay.D == 50 and lay.d_out == 50 and lay.off_lc_w == -1
    with pytest.raises(RuntimeError):
        _lib.make_layout("SRFU_B", 1000, 20, 50, 0, 0, 2, 1)      # SRFU needs n_labels


def test_lds_capability_query():
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 50000, 200, 50, 0, 0, 2, 1)
    f50, b50 = _lib.lds_bytes(lay, 50)
    assert 0 < f50 <= 160 * 1024 and 0 < b50 <= 160 * 1024
    f100, b100 = _lib.lds_bytes(lay, 100)
    assert f100 > 0 and b100 == 0                         # (first-generation layouts: the slot / chunk backward kernels report through srfrd_scratch_floats)
    assert _lib.lds_bytes(lay, 200) == (0, 0)
    assert _lib.scratch_floats(lay, 512, 50) == (0, 0)             # LDS-resident
    f200, b200 = _lib.scratch_floats(lay, 512, 200)                 # long-sequence build: global scratch per workgroup
    assert f200 > 0 and b200 > 0 and _lib.scratch_floats(lay, 512, 100)[1] > 0
    assert _lib.lib().srfrd_bwd_grid(C.byref(lay), 7, 50) == 7
    assert _lib.lib().srfrd_packed_floats(C.byref(lay)) == (2 * 6 + 1) * 2 * 4096


def test_argument_errors_are_codes_not_crashes():
    from srfrd_amd import _lib
    lib = _lib.lib()
    assert lib.srfrd_layout_init(None, 0, 10, 10, 10, 0, 0, 1, 1) == -1
    assert lib.srfrd_eval_rank(None, 4, 4, None, None, None) == -1
    assert lib.srfrd_topk_workspace_bytes(0, 10, 100) == 0
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    assert lib.srfrd_encoder_fwd(C.byref(lay), *([None] * 9), 4, 20, 0.0, 0, None, 0, *([None] * 8), 0, None, 0, None) == -1
    assert lib.srfrd_aux_floats(C.byref(lay), 4, 20) == 2 * 4 * (5 * 20 * 50 + 20 * 32)


def test_depth_outside_1_to_8_is_refused():
    """The backward kernels prefetch block n_blocks - 1's checkpoints in front of their loop: with no block that is a read in
    front of the allocation.  So depth 0 is refused where the layout is made and where a model is constructed - never run."""
    import srfrd_amd
    from srfrd_amd import _lib
    lib = _lib.lib()
    lay = _lib.Layout()
    assert _lib.MAX_BLOCKS == 8
    for nb in (0, -1, 9):
        assert lib.srfrd_layout_init(C.byref(lay), 0, 100, 20, 50, 0, 0, nb, 1) == -1, nb
        with pytest.raises(RuntimeError):
            _lib.make_layout("SASRec", 100, 20, 50, 0, 0, n_blocks=nb)
    for nb in (1, 8):
        assert _lib.make_layout("SASRec", 100, 20, 50, 0, 0, n_blocks=nb).n_blocks == nb
    make = {"SASRec": lambda nb: srfrd_amd.SASRec(100, 20, 50, 0.0, nb, 1, "cpu"),
            "SRFR": lambda nb: srfrd_amd.SRFR(100, 20, 45, 5, 0.0, nb, 1, "cpu"),
            "SRFRN": lambda nb: srfrd_amd.SRFRN(100, 20, 45, 5, 0.0, nb, 1, "cpu"),
            "SRFU_B": lambda nb: srfrd_amd.SRFU_B(100, 20, 50, 3, 0.0, nb, 1, "cpu"),
            "SRFU_F": lambda nb: srfrd_amd.SRFU_F(100, 20, 50, 3, 0.0, nb, 1, "cpu"),
            "SRFU_R": lambda nb: srfrd_amd.SRFU_R(100, 20, 50, 3, 0.0, nb, 1, "cpu")}
    for kind, ctor in make.items():
        for nb in (0, 9, -1):
            with pytest.raises(ValueError, match="num_blocks"):         # at construction, not at the first layout
                ctor(nb)
        assert ctor(1).layout.n_blocks == 1 and ctor(8).layout.n_blocks == 8, kind


def test_torch_library_ops_are_registered():
    """the launchers are dispatcher-visible custom ops (namespace srfrd::), not opaque ctypes calls; each has a
    fake implementation (shape propagation) and the encoder forward a registered backward."""
    import torch
    import srfrd_amd  # noqa: F401
    from srfrd_amd import ops
    for name in ops.OPS:
        op = getattr(torch.ops.srfrd, name)
        assert op.default._schema.name == f"srfrd::{name}"
    sch = str(torch.ops.srfrd.encoder_fwd.default._schema)
    assert "Tensor[] params" in sch and "-> Tensor[]" in sch
    # no CPU kernel is registered: calling on CPU tensors must fail loudly, never fall back
    import pytest
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.srfrd.eval_rank(torch.zeros(2, 5))
