"""-m gpu: ShardedRanker at k > 64 and within item filters: per-shard srfrd_logits_topk_wide /
srfrd_logits_topk_allow lists merged as sorted runs by srfrd_topk_merge_runs.

Every sharded list is held to two things: the fp64 reference of tests/rank_refs.py under the bar of the unsharded ranking,
unchanged (check_topk; tests/test_topk_merge_refs.py proves every case admissible on the reference alone), and the unsharded
call on the same operands, bit for bit in ids and values - a score does not depend on where its item range starts, and no case
here sends a user to a fallback.  2601 rows with a bit-identical pair across every shard cut, on the three table routes, at 1,
3 and 8 shards and k = 65, 100, 1024 (eight shards of 325 rows at k = 1024: every run has trailing empties, the lists come from
the no-threshold plans); with exclusion sets, filters (random, empty, a block over a shard cut), filter groups, SRFRN's side
term, the filtered k <= 64 route and the filtered target rank.  The data-parallel arm runs twice, each in a child process: the
forced exchange in a group of one rank on RCCL, and two gloo ranks on the one GPU."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import rank_refs as R
from tests import topk_allow_refs as A
from tests import topk_merge_refs as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (0, R.N_ITEMS + 1)


class Sharded:
    """a topk_allow_refs.Runner (the unsharded ops on a Case's own hidden state) and ShardedRankers over the same model, fed the
    same state: the model's ``_rank_inputs`` answers with the Case's last position and the exclusion sets of the call"""

    def __init__(self, case, route, monkeypatch):
        self.run = A.Runner(case, route)
        self.excl = (None, None, 0)
        monkeypatch.setattr(self.run.m, "_rank_inputs", lambda input_ids, fake_ids, exclude=None:
                            (self.run.hidden[:, -1:].contiguous(), self.run.ulab, self.excl))
        self.rankers = {}

    def ranker(self, n_shards):
        import srfrd_amd
        if n_shards not in self.rankers:
            self.rankers[n_shards] = srfrd_amd.ShardedRanker(self.run.m, n_shards=n_shards)
            assert len(self.rankers[n_shards].shards) == n_shards and not self.rankers[n_shards].dist_on
        return self.rankers[n_shards]

    def _args(self, excl_rows, filt, group):
        self.excl = (None, None, 0) if excl_rows is None else self.run._excl(excl_rows)
        kw = {} if excl_rows is None else dict(exclude="the rows above")
        if filt is not None:
            kw.update(allow=filt.f, allow_group=self.run.group_dev(group))
        return kw

    def topk(self, n_shards, k, excl_rows=None, filt=None, group=None):
        idx, val = self.ranker(n_shards).topk(None, None, None, k=k, **self._args(excl_rows, filt, group))
        return idx.cpu().numpy(), val.cpu().numpy()

    def rank(self, n_shards, targets, excl_rows=None, filt=None, group=None):
        t = torch.as_tensor(np.asarray(targets), dtype=torch.int64)
        return self.ranker(n_shards).target_rank(None, None, None, t, **self._args(excl_rows, filt, group)).cpu().numpy()

    def whole(self, k, excl_rows=None, filt=None, group=None):
        if filt is None:
            return self.run.wide(k, *FULL, True, excl_rows)
        return self.run.topk(filt, k, *FULL, True, excl_rows, group)


def _start(d, f, route, n_shards, monkeypatch, what):
    R.set_route(monkeypatch, route)
    sh = Sharded(M.sharded_case(d, n_shards, f), route, monkeypatch)
    return sh, sh.run.ref(), R.Tally(f"sharded {what} d_item {d} d_fake {f} {route} shards {n_shards}")


def _held(T, sh, ref, n_shards, k, excl_rows=None, filt=None, group=None, mask_rows=None, what=""):
    """one sharded list: the fp64 bar, then the unsharded call's bits"""
    got = sh.topk(n_shards, k, excl_rows, filt, group)
    T.add(*got, ref, k, *FULL, True, mask_rows if filt is not None else excl_rows, what=(what, k))
    assert A.same_bits(got, sh.whole(k, excl_rows, filt, group)), (T.tag, what, k, "differs from the unsharded call")
    return got


@pytest.mark.parametrize("n_shards", M.SHARD_COUNTS)
@pytest.mark.parametrize("d, route", M.SHARD_ROUTES)
def test_wide_lists_equal_the_unsharded_call_and_hold_the_fp64_bar(d, route, n_shards, monkeypatch):
    sh, ref, T = _start(d, 0, route, n_shards, monkeypatch, "wide")
    rows = R.exclusion_rows(ref, *FULL, R.N_ITEMS, 11)
    pairs = [i for cut in R.shard_cuts(n_shards) for i in (cut - 1, cut)]
    for k in M.SHARD_KS:
        idx, val = _held(T, sh, ref, n_shards, k, what="plain")
        assert idx[:, :len(pairs)].tolist() == [pairs] * idx.shape[0], (T.tag, k)          # the tied pairs lead, in id order
        _held(T, sh, ref, n_shards, k, excl_rows=rows, what="excl")
    T.close()


@pytest.mark.parametrize("n_shards", M.SHARD_COUNTS)
@pytest.mark.parametrize("d, route", M.SHARD_ROUTES)
def test_filtered_lists_at_k_100_and_on_the_narrow_k(d, route, n_shards, monkeypatch):
    sh, ref, T = _start(d, 0, route, n_shards, monkeypatch, "allow")
    B = sh.run.case.B
    for kind in M.SHARD_FILTERS:
        mask = M.shard_filter_mask(kind, n_shards)
        filt, off = A.Filter(mask, R.N_ITEMS), A.union_rows(mask, [0] * B)
        for k in (100, 10):
            idx, _ = _held(T, sh, ref, n_shards, k, filt=filt, mask_rows=off, what=kind)
            assert (idx < 0).all() if kind == "none" else mask[idx[idx >= 0]].all(), (T.tag, kind, k)
        if kind == "straddle" and n_shards > 1:
            cut = R.shard_cuts(n_shards)[0]
            assert (idx[:, :2] == np.array([cut - 1, cut])).all(), T.tag         # the tied pair the cut separates is allowed
    mask = M.shard_filter_mask("random_0.5", n_shards)
    x = R.exclusion_rows(ref, *FULL, R.N_ITEMS, 11)
    _held(T, sh, ref, n_shards, 100, excl_rows=x, filt=A.Filter(mask, R.N_ITEMS), mask_rows=A.union_rows(mask, [0] * B, x), what="allow + excl")
    masks, group = M.shard_group_masks(n_shards), M.shard_groups(B)
    idx, _ = _held(T, sh, ref, n_shards, 100, filt=A.Filter(masks, R.N_ITEMS), group=group, mask_rows=A.union_rows(masks, group), what="groups")
    for b in range(B):
        assert masks[group[b]][idx[b][idx[b] >= 0]].all(), (T.tag, b)
    T.close()


@pytest.mark.parametrize("n_shards", M.SHARD_COUNTS)
def test_the_side_term(n_shards, monkeypatch):
    sh, ref, T = _start(45, 5, "fp32", n_shards, monkeypatch, "side term")
    _held(T, sh, ref, n_shards, 100, what="plain")
    T.close()
    sh, ref, T = _start(45, 5, "bf16", n_shards, monkeypatch, "side term")
    mask = M.shard_filter_mask("random_0.5", n_shards)
    _held(T, sh, ref, n_shards, 100, filt=A.Filter(mask, R.N_ITEMS), mask_rows=A.union_rows(mask, [0] * sh.run.case.B), what="allow")
    T.close()


@pytest.mark.parametrize("n_shards", (3, 8))
@pytest.mark.parametrize("d, route", M.SHARD_ROUTES)
def test_filtered_target_rank_adds_up_over_the_shards(d, route, n_shards, monkeypatch):
    sh, ref, T = _start(d, 0, route, n_shards, monkeypatch, "rank")
    B = sh.run.case.B
    targets = R.rank_targets(ref, 5)
    masks, group = M.shard_group_masks(n_shards), M.shard_groups(B)
    x = R.exclusion_rows(ref, *FULL, R.N_ITEMS, 11)
    for filt, grp, m_rows in ((A.Filter(masks[0], R.N_ITEMS), None, masks[:1]), (A.Filter(masks, R.N_ITEMS), group, masks)):
        g = [0] * B if grp is None else grp
        for rows in (None, x):
            got = sh.rank(n_shards, targets, rows, filt, grp)
            assert got.dtype == np.int32 and got.shape == (B,)
            assert np.array_equal(got, sh.run.rank(filt, targets, *FULL, True, rows, grp)), (T.tag, "differs from the unsharded call")
            T.near += R.check_rank(got, ref, targets, *FULL, True, A.union_rows(m_rows, g, rows), tag=T.tag)
            T.targets += B
    assert np.array_equal(sh.rank(n_shards, targets), R.Runner.rank(sh.run, targets, *FULL))          # the unfiltered form, as before
    T.close()


def test_the_model_methods_agree_and_too_many_shards_are_refused_before_a_launch():
    import srfrd_amd
    torch.manual_seed(0)
    I, B, L = 3000, 9, 20
    m = srfrd_amd.SASRec(I, L, 50, 0.0, 2, 1, "cuda").to("cuda").eval()
    _, seq, rsq, *_ = srfrd_amd.synthetic_batch(I, L, B, seed=5, device="cuda")
    f = m.item_filter(torch.from_numpy(np.stack([A.filter_mask("random_0.5", I), A.filter_mask("random_0.1", I)])))
    grp = torch.arange(B, device="cuda") % 2
    tg = torch.arange(1, B + 1, device="cuda") * 7
    for n_shards in (3, 8):
        r = srfrd_amd.ShardedRanker(m, n_shards=n_shards)
        for kw in (dict(k=100, exclude="input"), dict(k=1024), dict(k=100, exclude="input", allow=f, allow_group=grp),
                   dict(k=10, allow=f, allow_group=grp)):
            a, b = r.topk(None, seq, rsq, **kw), m.topk(None, seq, rsq, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (n_shards, sorted(kw))
        assert torch.equal(r.target_rank(None, seq, rsq, tg, exclude="input", allow=f, allow_group=grp),
                           m.target_rank(None, seq, rsq, tg, exclude="input", allow=f, allow_group=grp))
    torch.cuda.synchronize()
    many = srfrd_amd.ShardedRanker(m, n_shards=17)
    with pytest.raises(ValueError, match="16384"):
        many.topk(None, seq, rsq, k=1024)
    with pytest.raises(ValueError, match="TOPK_WIDE_MAX"):
        many.topk(None, seq, rsq, k=1025)
    a, b = many.topk(None, seq, rsq, k=512), m.topk(None, seq, rsq, k=512)               # 32 x 512 slots: the cap exactly
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


# ---- the data-parallel arm ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _report(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, f"no report (rc {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    rep = json.loads(lines[-1])
    assert r.returncode == 0 and rep["ok"], rep
    return rep


def test_the_exchange_in_a_forced_group_of_one_rank_on_rccl():
    """SRFRD_FORCE_EXCHANGE=1, a 1-rank "nccl" group: the gathers of the filter groups, the filter check, all_to_all_single on
    RCCL and the merge from the received (world, B, k) buffer; filtered k = 100 and the filtered target rank"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0",
               SRFRD_FORCE_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sharded_rank_parity.py"), "--backend", "nccl", "--k", "100", "--allow"]
    rep = _report(subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600))
    assert rep["backend"] == "nccl" and rep["world"] == 1 and rep["k"] == 100 and rep["allow"] and rep["target_rank"]


def test_one_shard_per_rank_all_to_all_two_ranks():
    """two gloo ranks on the one GPU: each ranks both ranks' users against its half of the rows and receives its own users'
    lists only; filtered k = 100 with per-rank groups, and the filtered target rank (tools/sharded_rank_parity.py)"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "sharded_rank_parity.py"), "--backend", "gloo",
           "--k", "100", "--allow"]
    rep = _report(subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600))
    assert rep["world"] == 2 and rep["k"] == 100 and rep["allow"] and rep["target_rank"] and len(rep["shards"]) == 2
