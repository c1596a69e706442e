"""CPU-only: the optimizer and gradient-reduction entry points (srfrd_amd/csrc/srfrd_optim.hip) refuse every malformed call
their header documents before anything is launched, and launch nothing for an empty range: none of these calls may reach a
GPU (the pointers are never dereferenced)."""
import ctypes as C

import pytest

E_ARG, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: the calls below must return on the host


def _adam(lib, n=16, i0=0, i1=16, param=_d(), state=_d()):
    d = _d()
    return lib.srfrd_adam_step(param, d, d, d, n, i0, i1, 0, 0.9, 0.98, 1e-8, state, None, None, 0, None)


def test_adam_step_refuses_bad_slices(lib):
    assert _adam(lib, i0=2, i1=8) == E_ARG                  # i0 not a multiple of 4
    assert _adam(lib, i0=8, i1=4) == E_ARG                  # i1 < i0
    assert _adam(lib, i0=0, i1=17) == E_ARG                 # i1 > n
    assert _adam(lib, i0=-4, i1=8) == E_ARG
    assert _adam(lib, n=0, i0=0, i1=0) == E_ARG
    assert _adam(lib, param=None) == E_ARG
    assert _adam(lib, state=None) == E_ARG


def test_adam_step_launches_nothing_for_an_empty_slice(lib):
    # shard_bounds gives the ranks past the end of a short vector the empty slice [n, n), n not always a multiple of 4
    from srfrd_amd import shard_bounds
    assert shard_bounds(5, 3, 2) == (5, 5)
    assert _adam(lib, n=5, i0=5, i1=5) == 0
    assert _adam(lib, n=16, i0=8, i1=8) == 0
    assert _adam(lib, n=5, i0=6, i1=6) == E_ARG              # (still inside [0, n])


def _pack(lib, lay, n, n_table_pad, packed=_d()):
    d = _d()
    return lib.srfrd_adam_pack_step(C.byref(lay), d, d, d, d, n, n_table_pad, n_table_pad, 1e-3, 0.9, 0.98, 1e-8, d, None,
                                    packed, None, None)


def test_adam_pack_step_refuses_bad_layouts(lib):
    from srfrd_amd import _lib
    lay = _lib.make_layout("SASRec", 100, 20, 50, 0, 0, 2, 1)
    ntp = (lay.n_table + 3) // 4 * 4
    n = (ntp + lay.n_dense + 3) // 4 * 4
    assert _pack(lib, lay, n, ntp - 2) == E_ARG              # misaligned n_table_pad
    assert _pack(lib, lay, n, -4) == E_ARG
    assert _pack(lib, lay, ntp + lay.n_dense - 1, ntp) == E_ARG   # n_table_pad + n_dense > n
    assert _pack(lib, lay, 0, 0) == E_ARG
    assert _pack(lib, lay, n, ntp, packed=None) == E_ARG
    wide = _lib.make_layout("SASRec", 100, 20, 80, 0, 0, 2, 1)   # D = 80 > SRFRD_MAX_D
    ntp = (wide.n_table + 3) // 4 * 4
    assert _pack(lib, wide, (ntp + wide.n_dense + 3) // 4 * 4, ntp) == E_UNSUPPORTED


def test_reductions_refuse_bad_counts(lib):
    d = _d()
    assert lib.srfrd_reduce_dense(d, 0, 64, d, None, 1, None, None, None) == E_ARG
    assert lib.srfrd_reduce_dense(d, -3, 64, d, None, 1, None, None, None) == E_ARG
    assert lib.srfrd_reduce_dense(d, 4, 0, d, None, 1, None, None, None) == E_ARG
    assert lib.srfrd_reduce_dense(d, 4, 64, d, d, 8, None, None, None) == E_ARG      # loss_part without stats
    assert lib.srfrd_reduce_dense(d, 4, 64, d, None, 8, d, None, None) == E_ARG      # stats without loss_part
    assert lib.srfrd_reduce_dense(None, 4, 64, d, None, 1, None, None, None) == E_ARG
    assert lib.srfrd_loss_stats(d, 0, d, None, None) == E_ARG
    assert lib.srfrd_loss_stats(d, 8, None, None, None) == E_ARG
    assert lib.srfrd_loss_finalize(None, d, None) == E_ARG
    assert lib.srfrd_loss_finalize(d, None, None) == E_ARG
    assert lib.srfrd_step_begin(None, 1e-3, 0.9, 0.98, None) == E_ARG
    assert lib.srfrd_table_to_bf16(d, 0, d, None) == E_ARG
    assert lib.srfrd_table_to_bf16(d, 8, None, None) == E_ARG


def test_table_reduce_refuses_rows_wider_than_a_wave(lib):
    d = _d()
    assert lib.srfrd_table_reduce(d, d, d, 10, 65, d, None) == E_ARG
    assert lib.srfrd_table_reduce(d, d, d, 10, 0, d, None) == E_ARG
    assert lib.srfrd_table_reduce(d, d, d, 0, 50, d, None) == E_ARG
    assert lib.srfrd_table_reduce(d, None, d, 10, 50, d, None) == E_ARG


def test_l2_entry_points_refuse_bad_segments_and_slices(lib):
    d = _d()
    for n_seg in (0, -1, 129):
        assert lib.srfrd_l2_norms(d, d, d, n_seg, 0, 1e-3, d, d, d, None) == E_ARG
    assert lib.srfrd_l2_norms(d, d, d, 4, -4, 1e-3, d, d, d, None) == E_ARG
    assert lib.srfrd_l2_norms(d, d, d, 4, 0, 1e-3, d, d, None, None) == E_ARG
    assert lib.srfrd_l2_apply(d, d, 8, 4, 0, d, d, None, None) == E_ARG              # i1 < i0
    assert lib.srfrd_l2_apply(d, d, -1, 4, 0, d, d, None, None) == E_ARG
    assert lib.srfrd_l2_apply(None, d, 0, 4, 0, d, d, None, None) == E_ARG
    assert lib.srfrd_l2_apply(d, d, 7, 7, 0, d, d, None, None) == 0                   # empty: nothing launched
