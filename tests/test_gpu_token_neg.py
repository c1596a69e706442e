"""-m gpu: srfrd_token_negatives (K negatives per position outside the row user's history) and DeviceSampler(num_negatives=K).
Ids and the bits of log_q are compared for equality with the numpy restatement of the stream (tests/token_neg_refs.py) at
every shape, distribution, max_hist and optional argument; the sampler's properties (no history item, zeros only at dead
positions, ids in range) are checked without the restatement on the inputs tests/test_token_neg_abi.py proved free of
exhausted slots (seed 20240611); launches are deterministic and replay in a captured graph with a fresh state word."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import token_neg_refs as R

pytestmark = pytest.mark.gpu
SEED = 20240611
# (B, L, K): 257 makes a row's slot count no multiple of the 256 threads, 208 is the longest LDS-resident sequence length
SHAPES = [(1, 1, 1), (3, 7, 5), (5, 50, 16), (4, 20, 257), (2, 208, 3)]
# rows' user ids per shape: 0 and ids above usernum are clamped; every user of the set appears somewhere
USERS = {(1, 1, 1): [4], (3, 7, 5): [0, 1, 2], (5, 50, 16): [3, 4, 5, 1, 99], (4, 20, 257): [2, 4, 3, 1 << 40], (2, 208, 3): [5, 3]}
USERS_LONG = {(1, 1, 1): [7], (3, 7, 5): [6, 7, 8], (5, 50, 16): [8, 0, 7, 6, 99], (4, 20, 257): [7, 4, 8, 3], (2, 208, 3): [8, 7]}


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda().contiguous()


class Case:
    """one set of device inputs and the matching host arrays"""

    def __init__(self, hist, n_items, users, L, alias=False, dead_row=None, seed=SEED):
        from srfrd_amd.sampler import alias_table, negative_q
        self.hist, self.n_items, self.L = hist, n_items, L
        self.ptr, self.items, self.usernum = R.csr(hist)
        self.users = np.asarray(users, np.int64)
        self.targets = R.make_targets(hist, self.usernum, self.users, L, seed, dead_row=dead_row)
        self.max_true = max(len(h) for h in hist)
        self.q = self.prob = self.idx = None
        if alias:
            self.q = negative_q(n_items, R.counts_with_zeros(n_items))
            self.prob, self.idx = alias_table(self.q)
        self.d = dict(ptr=_dev(self.ptr), items=_dev(self.items), users=_dev(self.users), targets=_dev(self.targets),
                      prob=_dev(self.prob), idx=_dev(self.idx))

    def tables(self, K):
        """(item_log_q, user_log_keep) for K slots, host arrays"""
        import srfrd_amd
        keep = srfrd_amd.history_log_keep(R.interaction_data(self.hist, self.n_items), self.q)
        if self.q is None:
            return None, keep
        with np.errstate(divide="ignore"):
            return np.concatenate([[0.0], np.log(K * self.q)]).astype(np.float32), keep

    def launch(self, K, max_hist, index=0, state=None, exclude=1, want_log_q=True, keep=True, seed=SEED):
        from srfrd_amd import _lib
        from srfrd_amd._lib import check, ptr
        B, L = self.targets.shape
        ilq, ulk = self.tables(K)
        d = self.d
        d_ilq, d_ulk = _dev(ilq), (_dev(ulk) if keep else None)
        # sentinels: every element must be overwritten by the kernel itself
        ids = torch.full((B, L, K), -7, device="cuda", dtype=torch.int64)
        lq = torch.full((B, L, K), float("nan"), device="cuda", dtype=torch.float32) if want_log_q else None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(_lib.lib().srfrd_token_negatives(ptr(d["ptr"]), ptr(d["items"]), self.usernum, self.n_items, max_hist, ptr(d["users"]),
                                               ptr(d["targets"]), B, L, K, seed & 0xFFFFFFFF, index, ptr(state), ptr(d["prob"]),
                                               ptr(d["idx"]), ptr(d_ilq), ptr(d_ulk), exclude, ptr(ids), ptr(lq), st),
              "srfrd_token_negatives")
        torch.cuda.synchronize()
        return ids.cpu().numpy(), (None if lq is None else lq.cpu().numpy())

    def ref(self, K, max_hist, index=0, state2=None, exclude=1, keep=True, seed=SEED):
        ilq, ulk = self.tables(K)
        return R.token_negatives_ref(self.ptr, self.items, self.usernum, self.n_items, max_hist, self.users, self.targets, K, seed,
                                     index, state2=state2, alias_prob=self.prob, alias_idx=self.idx, item_log_q=ilq,
                                     user_log_keep=ulk if keep else None, exclude_history=bool(exclude))


def _same_bits(a, b):
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def _state(word):
    s = torch.zeros(32, dtype=torch.int32, device="cuda")
    s[2] = word - (1 << 32) if word >= (1 << 31) else word        # the uint32 word in the trainer's int32 tensor
    return s


@pytest.mark.parametrize("alias", [False, True], ids=["uniform", "alias"])
@pytest.mark.parametrize("long_hist", [False, True], ids=["hist33", "hist600"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_exact_against_the_restatement(shape, long_hist, alias):
    """max_hist: the true maximum, an exact power of two, and values below the true maximum (the kernel reads the first
    max_hist items of a history; the restatement clamps the same way).  With the short set, max_hist 32 puts the 32-item
    history at load 0.5 of a 64-slot set and 33 moves to 128 slots; 512 / 600 do the same at 1024 / 2048."""
    B, L, K = shape
    hist = R.users_long() if long_hist else R.users_short()
    users = (USERS_LONG if long_hist else USERS)[shape]
    case = Case(hist, 200, users, L, alias=alias, dead_row=1 if B >= 3 else None)
    assert case.max_true == (600 if long_hist else 33)
    word = 0xC0FFEE11
    for max_hist in ((600, 1024, 599, 512) if long_hist else (33, 64, 32)):
        for exclude in (1, 0):
            for st in (None, word):
                ids_r, lq_r, _ = case.ref(K, max_hist, index=3, state2=st, exclude=exclude)
                state = None if st is None else _state(st)
                ids, lq = case.launch(K, max_hist, index=3, state=state, exclude=exclude)
                assert (ids == ids_r).all(), (max_hist, exclude, st)
                assert _same_bits(lq, lq_r), (max_hist, exclude, st)
                ids2, none = case.launch(K, max_hist, index=3, state=state, exclude=exclude, want_log_q=False)
                assert none is None and (ids2 == ids_r).all()
    # without user_log_keep the correction is item_log_q (or the constant) alone
    ids_r, lq_r, _ = case.ref(K, case.max_true, keep=False)
    ids, lq = case.launch(K, case.max_true, keep=False)
    assert (ids == ids_r).all() and _same_bits(lq, lq_r)
    if not alias:
        assert (lq[ids != 0] == np.float32(math.log(K / 200))).all()


def test_large_sets_take_the_lds_opt_in():
    """max_hist 4096 is the last capacity (8192 slots, 32 KiB) inside the default dynamic-LDS limit; 4097 takes 16384 slots
    (64 KiB) and SRFRD_TNEG_MAX_HIST 32768 (128 KiB), both through the opt-in; the draws do not depend on the capacity"""
    from srfrd_amd import _lib
    case = Case(R.users_long(), 200, [8, 7, 6, 3, 0], 20, dead_row=3)
    ids_r, lq_r, _ = case.ref(16, 600, index=1)
    for max_hist in (4096, 4097, _lib.TNEG_MAX_HIST, 4097):
        ids, lq = case.launch(16, max_hist, index=1)
        assert (ids == ids_r).all() and _same_bits(lq, lq_r), max_hist


def test_tiny_catalog_edge_users():
    """8 items: a user holding 7 of them gets 8 or 0 in every live slot, a user holding all 8 gets 0 everywhere, a row
    without a target gets 0 everywhere; user ids 0 and above usernum are clamped"""
    hist = R.users_tiny()
    users = [1, 2, 3, 3, 0, 77, -5]                 # 77 -> user 3, -5 -> user 0 (an empty history)
    for alias in (False, True):
        case = Case(hist, 8, users, 6, alias=alias, dead_row=3)
        for K in (1, 9):
            ids, lq = case.launch(K, case.max_true)
            ids_r, lq_r, _ = case.ref(K, case.max_true)
            assert (ids == ids_r).all() and _same_bits(lq, lq_r)
            live = case.targets != 0
            assert set(np.unique(ids[0][live[0]]).tolist()) <= {0, 8}
            assert (ids[1] == 0).all() and (lq[1] == 0).all()
            assert (ids[3] == 0).all() and (lq[3] == 0).all()
            assert (ids[~live] == 0).all() and (lq[~live] == 0).all()
            assert not set(ids[2].ravel().tolist()) & {2, 6} and not set(ids[5].ravel().tolist()) & {2, 6}
            assert np.isfinite(lq).all() and ids.min() >= 0 and ids.max() <= 8
        if not alias:
            assert (case.launch(9, case.max_true)[0][0] == 8).any()


@pytest.mark.parametrize("alias", [False, True], ids=["uniform", "alias"])
def test_properties_without_the_restatement(alias):
    """the inputs of tests/test_token_neg_abi.py (200 items, histories of at most 30 % of them, seed 20240611)"""
    hist, ptr, items, usernum, users, targets = R.standard_case()
    case = Case(hist, 200, users, 20, alias=alias, dead_row=2)
    assert (case.targets == targets).all()
    for index in range(4):
        ids, lq = case.launch(16, 600, index=index)
        assert ((ids == 0) == np.repeat((targets == 0)[:, :, None], 16, axis=2)).all()
        assert ids.min() >= 0 and ids.max() <= 200 and np.isfinite(lq).all()
        for b, u in enumerate(users):
            assert not set(hist[min(int(u), usernum)]) & set(ids[b].ravel().tolist())
        if alias:
            assert not (case.q[ids[ids > 0] - 1] == 0).any()


def test_two_launches_give_equal_bits_and_arguments_matter():
    case = Case(R.users_long(), 200, [8, 7, 6, 5, 4], 50, alias=True)
    a = case.launch(16, 600, index=2, state=_state(5))
    b = case.launch(16, 600, index=2, state=_state(5))
    assert (a[0] == b[0]).all() and _same_bits(a[1], b[1])
    live = np.repeat((case.targets != 0)[:, :, None], 16, axis=2)
    for other in (case.launch(16, 600, index=3, state=_state(5)), case.launch(16, 600, index=2, state=_state(6)),
                  case.launch(16, 600, index=2, state=_state(5), seed=SEED + 1), case.launch(16, 600, index=2)):
        assert (a[0][live] != other[0][live]).mean() > 0.5
    zero = case.launch(16, 600, index=2, state=_state(0))
    none = case.launch(16, 600, index=2)
    assert (zero[0] == none[0]).all()


def test_graph_replay_draws_from_the_state_word():
    from srfrd_amd import _lib
    from srfrd_amd._lib import check, ptr
    case = Case(R.users_long(), 200, [8, 7, 6, 5], 20)
    B, L, K = 4, 20, 16
    _, ulk = case.tables(K)
    d, d_ulk = case.d, _dev(ulk)
    state = _state(101)
    ids = torch.zeros(B, L, K, device="cuda", dtype=torch.int64)
    lq = torch.zeros(B, L, K, device="cuda", dtype=torch.float32)

    def launch():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(_lib.lib().srfrd_token_negatives(ptr(d["ptr"]), ptr(d["items"]), case.usernum, 200, 600, ptr(d["users"]),
                                               ptr(d["targets"]), B, L, K, SEED, 9, ptr(state), None, None, None, ptr(d_ulk), 1,
                                               ptr(ids), ptr(lq), st), "srfrd_token_negatives")
    eager = {w: case.launch(K, 600, index=9, state=_state(w)) for w in (202, 303)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()                                   # warm-up on the side stream, as torch's capture recipe has it
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    got = {}
    for w in (202, 303):
        state[2] = w                               # changed on the device, between replays
        g.replay()
        torch.cuda.synchronize()
        got[w] = (ids.cpu().numpy().copy(), lq.cpu().numpy().copy())
    for w in (202, 303):
        assert (got[w][0] == eager[w][0]).all() and _same_bits(got[w][1], eager[w][1])
        assert (got[w][0] == case.ref(K, 600, index=9, state2=w)[0]).all()
    assert (got[202][0] != got[303][0]).any()


def _interactions(n_items=300, n_users=40, seed=4):
    import srfrd_amd
    rng = np.random.RandomState(seed)
    u, it = [], []
    for user in range(1, n_users + 1):
        n = int(rng.randint(3, 45))
        u += [user] * n
        it += list(rng.randint(1, n_items + 1, n))
    it[0] = n_items                                 # itemnum is the largest id seen
    return srfrd_amd.partition(np.array(u), np.array(it), rng.rand(len(u)) < 0.3)


def test_device_sampler_draws_with_every_batch():
    import srfrd_amd
    data = _interactions()
    s = srfrd_amd.DeviceSampler(data, 4, 20, seed=5, num_negatives=6)
    plain = srfrd_amd.DeviceSampler(data, 4, 20, seed=5)            # num_negatives = 0: today's sampler
    assert not hasattr(plain, "negatives")
    hist = [list(data.train_items[data.train_ptr[u]:data.train_ptr[u + 1]]) for u in range(data.usernum + 1)]
    keep = srfrd_amd.history_log_keep(data)
    for index in range(3):
        batch, ref_batch = s.next_batch(), plain.next_batch()
        assert len(batch) == 7 and all(torch.equal(a, b) for a, b in zip(batch, ref_batch))
        user, pos = batch[0], batch[3]
        neg, lq = s.negatives, s.log_q
        assert neg.shape == (4, 20, 6) and neg.dtype == torch.int64 and lq.shape == (4, 20, 6) and lq.dtype == torch.float32
        by_hand, lq_by_hand = s.token_negatives(user, pos, index=index)
        assert torch.equal(neg, by_hand) and torch.equal(lq, lq_by_hand) and by_hand.data_ptr() != neg.data_ptr()
        ids_r, lq_r, _ = R.token_negatives_ref(data.train_ptr, data.train_items, data.usernum, data.itemnum, s.max_hist,
                                               user.cpu().numpy(), pos.cpu().numpy(), 6, 5, index, user_log_keep=keep)
        assert (neg.cpu().numpy() == ids_r).all() and _same_bits(lq.cpu().numpy(), lq_r)
        for b in range(4):
            assert not set(hist[int(user[b])]) & set(neg[b].view(-1).tolist())
        assert bool(((neg == 0) == (pos == 0).unsqueeze(-1)).all())
    # the caller's tensors, and the state word
    mine, mine_lq = torch.zeros(4, 20, 6, dtype=torch.int64, device="cuda"), torch.zeros(4, 20, 6, device="cuda")
    batch = s.next_batch(neg_out=mine, log_q_out=mine_lq)
    assert s.negatives is mine and s.log_q is mine_lq and bool((mine != 0).any())
    state = _state(77)
    with_state, _ = s.token_negatives(batch[0], batch[3], index=3, state=state)
    ids_r, _, _ = R.token_negatives_ref(data.train_ptr, data.train_items, data.usernum, data.itemnum, s.max_hist,
                                        batch[0].cpu().numpy(), batch[3].cpu().numpy(), 6, 5, 3, state2=77, user_log_keep=keep)
    assert (with_state.cpu().numpy() == ids_r).all() and not torch.equal(with_state, mine)
    with pytest.raises(ValueError):
        s.next_batch(neg_out=torch.zeros(4, 20, 5, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        plain.next_batch(neg_out=mine)
    with pytest.raises(RuntimeError):
        plain.token_negatives(batch[0], batch[3], index=0)


def test_device_sampler_by_popularity_and_without_exclusion():
    import srfrd_amd
    from srfrd_amd.sampler import alias_table, negative_q
    data = _interactions()
    counts = np.bincount(data.train_items, minlength=data.itemnum + 1).astype(np.float64)
    q = negative_q(data.itemnum, counts, 0.75)
    prob, idx = alias_table(q)
    with np.errstate(divide="ignore"):
        ilq = np.concatenate([[0.0], np.log(6 * q)]).astype(np.float32)
    for exclude in (True, False):
        s = srfrd_amd.DeviceSampler(data, 4, 20, seed=5, num_negatives=6, neg_counts=counts, neg_alpha=0.75, exclude_history=exclude)
        batch = s.next_batch()
        keep = srfrd_amd.history_log_keep(data, q) if exclude else None
        ids_r, lq_r, _ = R.token_negatives_ref(data.train_ptr, data.train_items, data.usernum, data.itemnum, s.max_hist,
                                               batch[0].cpu().numpy(), batch[3].cpu().numpy(), 6, 5, 0, alias_prob=prob,
                                               alias_idx=idx, item_log_q=ilq, user_log_keep=keep, exclude_history=exclude)
        assert (s.negatives.cpu().numpy() == ids_r).all() and _same_bits(s.log_q.cpu().numpy(), lq_r)
        assert not (q[ids_r[ids_r > 0] - 1] == 0).any()


def test_losses_train_on_the_sampler_negatives():
    import srfrd_amd
    data = _interactions()
    torch.manual_seed(0)
    model = srfrd_amd.SASRec(300, 20, 50, 0.0, 2, 1, "cuda").to("cuda").train()
    s = srfrd_amd.DeviceSampler(data, 4, 20, seed=5, num_negatives=6, model=model)
    u, seq, rsq, pos, prs, neg, nrs = s.next_batch()
    for objective, kw in (("gbce", dict(beta=srfrd_amd.gbce_beta(300, 6, 0.75))), ("softmax", dict(log_q=s.log_q))):
        model.zero_grad()
        hidden = model(u, seq, rsq)[0]
        loss = model.token_negatives_loss(hidden, pos, s.negatives, objective=objective, **kw)
        loss.backward()
        assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        assert float(model.item_emb.weight.grad.abs().sum()) > 0
