"""CPU-only: srfrd_token_negatives (K negatives per position, drawn outside the user's history) is declared, exported and
typed; what it refuses is refused before anything touches a GPU; srfrd_amd.history_log_keep agrees with a brute-force fp64
loop; the numpy restatement of the stream (tests/token_neg_refs.py) has, on its own, the sampler's properties on the inputs
the GPU tests use; DeviceSampler's new arguments are checked before the device."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import token_neg_refs as R

E_ARG, E_UNSUPPORTED = -1, -2
PTRS = ("user_ptr", "items", "users", "targets", "state", "alias_prob", "alias_idx", "item_log_q", "user_log_keep", "out_ids",
        "out_log_q")
OPTIONAL = ("state", "alias_prob", "alias_idx", "item_log_q", "user_log_keep", "out_log_q")
SEED = 20240611                      # the seed of every property test below (and of the GPU tests' inputs)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from srfrd_amd import _lib
    return _lib.lib()


def _d(n=64):
    return C.c_void_p(n)           # never dereferenced: every call below must return before a launch


def _call(lib, usernum=10, n_items=100, max_hist=40, B=4, L=20, K=10, exclude=1, **null):
    a = {k: (None if k in null else _d()) for k in PTRS}
    return lib.srfrd_token_negatives(a["user_ptr"], a["items"], usernum, n_items, max_hist, a["users"], a["targets"], B, L, K, 1, 2,
                                     a["state"], a["alias_prob"], a["alias_idx"], a["item_log_q"], a["user_log_keep"], exclude,
                                     a["out_ids"], a["out_log_q"], None)


def test_symbol_declared_exported_and_typed(lib):
    from srfrd_amd import _lib
    from tests.test_abi import ROOT, header_symbols
    s = "srfrd_token_negatives"
    assert s in header_symbols() and s in _lib.SIGNATURES and hasattr(C.CDLL(_lib.LIB_PATH), s)
    res, args = _lib.SIGNATURES[s]
    assert res is C.c_int and len(args) == 21
    assert args[10] is C.c_uint32 and args[11] is C.c_uint32                 # seed, batch_index
    hdr = open(os.path.join(ROOT, "include", "srfrd_hip.h")).read()
    assert f"#define SRFRD_TNEG_TRIES {_lib.TNEG_TRIES}\n" in hdr and _lib.TNEG_TRIES == R.TRIES == 32
    assert f"#define SRFRD_TNEG_MAX_HIST {_lib.TNEG_MAX_HIST}\n" in hdr and _lib.TNEG_MAX_HIST == 16384
    rng = open(os.path.join(ROOT, "srfrd_amd", "csrc", "srfrd_rng.h")).read()
    assert f"SITE_TNEG = 0x{R.SITE_TNEG:08X}u" in rng


def test_refusals_before_any_launch(lib):
    from srfrd_amd import _lib
    for k in PTRS:
        if k not in OPTIONAL:
            assert _call(lib, **{k: 1}) == E_ARG, k
    for name in ("B", "L", "K", "usernum", "n_items"):
        for v in (0, -1):
            assert _call(lib, **{name: v}) == E_ARG, (name, v)
    assert _call(lib, B=1 << 15, L=1 << 8, K=255) == E_ARG                   # B L (1 + K) = 2^31
    assert _call(lib, B=1 << 15, L=1 << 8, K=1 << 20) == E_ARG               # ... and far beyond it (no int overflow)
    assert _call(lib, alias_prob=1) == E_ARG and _call(lib, alias_idx=1) == E_ARG
    assert _call(lib, item_log_q=1) == E_ARG                                 # an alias table without item_log_q
    assert _call(lib, max_hist=-1) == E_ARG and _call(lib, max_hist=-1, exclude=0) == E_ARG
    assert _call(lib, max_hist=_lib.TNEG_MAX_HIST + 1) == E_UNSUPPORTED
    assert _call(lib, max_hist=1 << 30) == E_UNSUPPORTED


def test_history_log_keep_against_brute_force():
    import srfrd_amd
    n_items = 12
    hist = [[], [3], [1, 2, 2, 1, 5, 5, 5], list(range(1, 13)) + [4, 4], [7, 8, 9, 7], [12, 12]]      # one item; duplicates; all mass
    data = R.interaction_data(hist, n_items)
    rng = np.random.RandomState(3)
    w = rng.rand(n_items)
    w[[1, 6]] = 0.0                                                          # items 2 and 7 carry no mass
    q = w / w.sum()
    for qq in (None, q):
        got = srfrd_amd.history_log_keep(data, qq)
        assert got.dtype == np.float32 and got.shape == (len(hist),)
        for u, h in enumerate(hist):
            mass = 0.0
            for it in sorted(set(h)):
                mass += (1.0 / n_items) if qq is None else float(qq[it - 1])
            if len(set(h)) == n_items:
                assert got[u] == -np.inf
            else:
                assert got[u] == pytest.approx(math.log(1.0 - mass), rel=1e-6, abs=1e-7), (u, qq is None)
        assert got[0] == 0.0
    assert srfrd_amd.history_log_keep(data, None)[2] == np.float32(math.log(1.0 - 3 / 12))
    # all the MASS, not all the items: the history holds every item of positive weight
    q2 = np.zeros(n_items)
    q2[[0, 1, 4]] = [0.1, 0.2, 0.7]
    assert srfrd_amd.history_log_keep(data, q2)[2] == -np.inf
    with pytest.raises(ValueError):
        srfrd_amd.history_log_keep(data, np.ones(n_items + 1) / (n_items + 1))


def test_restatement_never_emits_a_history_item_and_never_runs_dry():
    """200 items, histories of at most 30 % of them (60 distinct), seed 20240611, batch indices 0..3: 10 rows x 20 x 16 x 4
    draws, uniform and by popularity"""
    hist, ptr, items, usernum, users, targets = R.standard_case()
    assert R.distinct_fraction(hist, 200) <= 0.30
    from srfrd_amd.sampler import alias_table, negative_q
    q = negative_q(200, R.counts_with_zeros(200))
    prob, idx = alias_table(q)
    for alias in (False, True):
        for index in range(4):
            kw = dict(alias_prob=prob, alias_idx=idx, item_log_q=np.zeros(201, np.float32)) if alias else {}
            ids, _, tries = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 16, SEED, index, **kw)
            assert ((ids == 0) == np.repeat((targets == 0)[:, :, None], 16, axis=2)).all()
            assert ids.min() >= 0 and ids.max() <= 200 and tries.max() <= R.TRIES
            for b, u in enumerate(users):
                own = set(hist[min(int(u), usernum)])
                assert not own & set(ids[b].ravel().tolist())
            if alias:
                assert not (q[ids[ids > 0] - 1] == 0).any()                  # an item of weight 0 is never drawn


def test_restatement_whole_catalog_history_gives_zeros():
    hist = R.users_tiny()
    ptr, items, usernum = R.csr(hist)
    users = np.array([1, 2, 3], np.int64)
    targets = R.make_targets(hist, usernum, users, 6, SEED)
    ids, log_q, tries = R.token_negatives_ref(ptr, items, usernum, 8, 9, users, targets, 9, SEED, 0,
                                              user_log_keep=np.array([0, math.log(1 / 8), -np.inf, math.log(6 / 8)], np.float32))
    live = targets != 0
    assert set(np.unique(ids[0][live[0]]).tolist()) <= {0, 8} and (ids[0] == 8).any()
    assert (ids[1] == 0).all() and (log_q[1] == 0).all() and (tries[1][live[1]] == R.TRIES + 1).all()
    assert not set(ids[2].ravel().tolist()) & {2, 6}
    assert np.isfinite(log_q).all()
    assert (log_q[0][ids[0] == 8] == np.float32(np.float32(math.log(9 / 8)) - np.float32(math.log(1 / 8)))).all()
    # without exclusion the first draw is kept: nothing is 0 at a live position, history items do appear
    free, _, t2 = R.token_negatives_ref(ptr, items, usernum, 8, 9, users, targets, 9, SEED, 0, exclude_history=False)
    assert (free[live] > 0).all() and (t2[live] == 1).all() and (free[1] != 0).any()


def test_restatement_depends_on_state_word_index_and_seed():
    hist, ptr, items, usernum, users, targets = R.standard_case(L=7)
    a = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 0, state2=1)[0]
    b = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 0, state2=2)[0]
    a2 = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 0, state2=1)[0]
    none = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 0)[0]
    zero = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 0, state2=0)[0]
    other_index = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED, 1, state2=1)[0]
    other_seed = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 5, SEED + 1, 0, state2=1)[0]
    assert (a == a2).all() and (none == zero).all()
    live = np.repeat((targets != 0)[:, :, None], 5, axis=2)
    for x in (b, none, other_index, other_seed):
        assert (a[live] != x[live]).mean() > 0.9
    # rows 8 and 9 share user 8 (id 99 is clamped) but not the row index: different draws
    assert (a[8] != a[9]).any()


def test_restatement_is_uniform_over_the_free_items():
    """chi-square of 10 rows x 20 x 64 draws of one user (60 of 200 items held) over the 140 free items: 139 degrees of
    freedom, mean 139, sd 16.7; the bound 139 + 5 sd = 223 fails a correct stream once in ~10^6 seeds"""
    hist = R.users_long()
    ptr, items, usernum = R.csr(hist)
    users = np.full(10, 6, np.int64)
    targets = np.full((10, 20), hist[6][0], np.int64)
    ids, _, _ = R.token_negatives_ref(ptr, items, usernum, 200, 600, users, targets, 64, SEED, 0)
    cnt = np.bincount(ids.ravel(), minlength=201)
    free = np.setdiff1d(np.arange(1, 201), hist[6])
    assert cnt.sum() == cnt[free].sum() == 10 * 20 * 64
    exp = cnt.sum() / free.size
    chi2 = float(((cnt[free] - exp) ** 2 / exp).sum())
    assert chi2 < 223.0, chi2


def test_device_sampler_checks_new_arguments_before_the_device():
    import srfrd_amd
    from srfrd_amd import _lib
    data = R.interaction_data(R.users_short(), 200)
    with pytest.raises(ValueError, match="shape"):
        srfrd_amd.DeviceSampler(data, 4, 20, device="cpu", num_negatives=6, neg_counts=np.ones(200))
    with pytest.raises(ValueError):
        srfrd_amd.DeviceSampler(data, 4, 20, device="cpu", num_negatives=-1)
    long_hist = [[], list(np.arange(_lib.TNEG_MAX_HIST + 1) % 150 + 1), [1, 2]]
    big = R.interaction_data(long_hist, 200)
    with pytest.raises(ValueError, match="exclude_history=False"):
        srfrd_amd.DeviceSampler(big, 4, 20, device="cpu", num_negatives=6)
    # valid arguments get as far as the device check, as without them (there is no CPU fallback)
    for kw in (dict(), dict(num_negatives=6), dict(num_negatives=6, neg_counts=np.ones(201)),
               dict(num_negatives=0, neg_counts=np.ones(7))):              # K = 0: the other new arguments are not looked at
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            srfrd_amd.DeviceSampler(data, 4, 20, device="cpu", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        srfrd_amd.DeviceSampler(big, 4, 20, device="cpu", num_negatives=6, exclude_history=False)
