"""What tests/test_gpu_skew_bits.py (-m gpu) and tests/test_skew_cover.py (CPU) share; no test functions.

``__graft_entry__.build()`` links four libraries with the same symbol names (``__graft_entry__.LIBRARIES``): the product and
three schedule-skew builds (srfrd_dev.h, -DSRFRD_SKEW=<wave mask>: every workgroup barrier followed by a ~2 us sleep of the
waves in the mask).  All Python in srfrd_amd/ reaches the library through ``_lib.lib()`` at call time, so ``use(name)`` swaps
another build in for the length of one call sequence, in this process, on the same device: "same input, same bits, whatever
the schedule" is then the detector of a missing barrier, for every output the project documents as bitwise reproducible.

    name      encoder units   every other unit
    product   0               0
    skew      0x0f0f          0x0f0f      waves 0-3 and 8-11: splits the 8- and 16-wave encoder workgroups; a 256-thread
                                          workgroup IS waves 0-3, all of them sleep alike, nothing runs ahead
    even      0x0f0f          0x5555      waves 0, 2, 4, ...: splits every workgroup of two or more waves
    odd       0x0f0f          0xaaaa      the complement

An EXERCISER is a function of a seed that builds its inputs on the device and returns ``({name: tensor}, {name: check})``:
everything its kernels wrote, on the CPU, and for the names listed in NOT_REPRODUCED / ATOMIC_SUMS the check that holds them
instead of the bits.  Two limits: the sleep FOLLOWS a barrier, so a race in a kernel's first barrier
interval is not widened by any mask; and a hand-off between waves that uses no workgroup barrier (the wave barriers of
srfrd_rank.hip, the row-owner forward) is not delayed at all.
"""
import contextlib
import ctypes as C
import fnmatch
import os
import re
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "srfrd_amd", "csrc")
SEED = 1


# ---------------------------------------------------------------------------------------------------------------------------
# the libraries
# ---------------------------------------------------------------------------------------------------------------------------
def libraries():
    """name -> (path, mask of the encoder units, mask of the others)"""
    import __graft_entry__ as g
    return dict(g.LIBRARIES)


ENCODER_LIBS = ("skew", "even", "odd")     # under even / odd the encoder kernels keep 0x0f0f; the kernels around them change
OTHER_LIBS = ("even", "odd")               # under 0x0f0f a 256-thread workgroup is not split: tests/test_skew_cover.py says so

_handles = {}


def load(name):
    """the ctypes handle of one library, every symbol of _lib.SIGNATURES bound; the product's is the process's own"""
    from srfrd_amd import _lib
    if name == "product":
        return _lib.lib()
    if name not in _handles:
        path = libraries()[name][0]
        assert os.path.exists(path), f"{path} is missing: __graft_entry__.build() links it"
        handle = C.CDLL(path)
        for sym, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(handle, sym)
            fn.restype, fn.argtypes = res, args
        _handles[name] = handle
    return _handles[name]


class Recorder:
    """a library handle that notes the entry points asked of it"""

    def __init__(self, handle):
        object.__setattr__(self, "_handle", handle)
        object.__setattr__(self, "called", set())

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._handle, name)


@contextlib.contextmanager
def use(name):
    """``srfrd_amd._lib.lib()`` answers with library `name` inside the block -> the Recorder around its handle.  Whatever
    captures a graph (a FusedTrainer's first step) belongs inside, so that the graph holds this library's kernels."""
    from srfrd_amd import _lib
    rec = Recorder(load(name))
    old = _lib._lib
    _lib._lib = rec
    try:
        yield rec
    finally:
        torch.cuda.synchronize()
        _lib._lib = old


def probe(name):
    """(host mask, device mask) srfrd_skew_mask reports through library `name`'s handle"""
    out = torch.full((1,), -1, device="cuda", dtype=torch.int32)
    with use(name) as lib:
        host = lib.srfrd_skew_mask(C.c_void_p(out.data_ptr()), _st())
    return host, int(out.item()) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------------------------------
# outputs the product itself does not reproduce, and what holds them instead of their bits
# ---------------------------------------------------------------------------------------------------------------------------
# Item-table gradients scattered by float atomics (the order of the additions is the hardware's): the module path's autograd
# backward.  (FusedTrainer(deterministic=False) scatters the same way; every fused step here runs deterministic=True.)  Held,
# under EVERY library, to the fp64 bar tests/grad_refs.py sets for them: row_errors <= bound(e32), zero rows exactly zero.
NOT_REPRODUCED = {
    "encoder-*": ["autograd.grad.item_emb.weight", "autograd.grad.embedding_layer.item_embed.weight"],
}
# Sums by double atomics (srfrd_eval_rank / srfrd_target_rank's metric_acc): [1] and [2] are counts, exact in any order; [0]
# is recomputed on the host from the ranks (which ARE compared by bits): n terms 1 / log2(rank + 2), each within 2^-51 of the
# host's (log2 within an ulp on either side, the division rounded once), summed in any order within (n - 1) 2^-52:
# |acc[0] - host| <= (n + 1) 2^-52 host.
ATOMIC_SUMS = {
    "ranking-*": ["*.metric_acc"],
}


def listed(exerciser, name):
    return any(fnmatch.fnmatch(exerciser, pat) and any(fnmatch.fnmatch(name, n) for n in names)
               for table in (NOT_REPRODUCED, ATOMIC_SUMS) for pat, names in table.items())


def metric_check(ranks, cut_k=10):
    """the check of one metric_acc (3 doubles) against the int32 ranks it was summed from"""
    r = ranks.double()
    hit = r < cut_k
    want0 = float(torch.where(hit, 1.0 / torch.log2(r + 2.0), torch.zeros_like(r)).sort().values.sum())
    want1, n = float(hit.sum()), r.numel()

    def check(acc):
        a = [float(x) for x in acc]
        assert a[1] == want1 and a[2] == float(n), (a, want1, n)
        assert abs(a[0] - want0) <= (n + 1) * 2.0 ** -52 * want0, (a[0], want0)
    return check


# ---------------------------------------------------------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def _L():
    from srfrd_amd import _lib
    return _lib.lib()


def _ok(rc, what):
    assert rc == 0, (what, rc)


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def _cpu(out):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@contextlib.contextmanager
def _env(name):
    """one of the kernel plan's switches (srfrd_amd._lib.SWITCHES) set for the block"""
    from srfrd_amd import _lib
    old = {k: os.environ.pop(k) for k in list(os.environ) if k in _lib.SWITCHES or k == "SRFRD_TOPK_FP32"}
    if name:
        os.environ[name] = "1"
    try:
        yield
    finally:
        if name:
            os.environ.pop(name, None)
        os.environ.update(old)


def bits(t):
    """a tensor as integers of its own width: NaN payloads and the sign of zero count"""
    if t.is_floating_point():
        return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def assert_bitwise(name, a, b, what):
    """as test_gpu_train_ranked._assert_bitwise: the count and the first indices on a mismatch"""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
    bad = (bits(a) != bits(b)).reshape(-1)
    if bool(bad.any()):
        first = [int(i) for i in bad.nonzero().flatten()[:8]]
        raise AssertionError(f"{what}: {name}: {int(bad.sum())} of {a.numel()} elements differ, first at flat indices {first} "
                             f"(product {a.reshape(-1)[first].tolist()}, here {b.reshape(-1)[first].tolist()})")


# ---------------------------------------------------------------------------------------------------------------------------
# exercisers
# ---------------------------------------------------------------------------------------------------------------------------
# run(seed) -> ({name: CPU tensor}, {name: check(tensor)}); libs: the skewed libraries it runs under; entries: the C entry points
# it asks of the library (the GPU test asserts each was called); sources: the non-encoder translation units whose kernels it
# launches; families: keys of ENCODER_WIDTHS
Exerciser = namedtuple("Exerciser", "name run libs entries sources families")
EXERCISERS = {}


def _register(name, run, libs, entries, sources=(), families=()):
    assert name not in EXERCISERS
    EXERCISERS[name] = Exerciser(name, run, tuple(libs), tuple(entries), tuple(sources), tuple(families))


# ---- every encoder family the plan can choose ---------------------------------------------------------------------------------
def _enc_forward(model, ids, p, seed, save):
    """modules._launch_fwd with ZEROED outputs: the ragged kernels write only the rows of a sequence's computed tiles, and what
    nobody wrote must not differ from run to run"""
    from srfrd_amd import _lib
    lay = model.layout
    B, L = ids[0].shape
    f32 = dict(device=ids[0].device, dtype=torch.float32)
    out = {"hidden": torch.zeros(B, L, lay.d_out, **f32), "pos_logits": torch.zeros(B, L, **f32), "neg_logits": torch.zeros(B, L, **f32),
           "save_x": torch.zeros(B, lay.n_blocks + 1, L, lay.D, **f32) if save else None,
           "save_h1": torch.zeros(B, lay.n_blocks, L, lay.D, **f32) if save else None,
           "save_aux": torch.zeros(_lib.query("srfrd_aux_floats", lay=lay, B=B, L=L), **f32) if save else None}
    model._launch_fwd(*ids, p, seed, save, out=out)
    return {k: v for k, v in out.items() if v is not None}


def _trainer_outputs(out, tag, losses, model, tr):
    out[f"{tag}.loss"] = torch.stack([x.reshape(()) for x in losses])
    out[f"{tag}.parameters"], out[f"{tag}.m"], out[f"{tag}.v"], out[f"{tag}.slabs"] = model._flat, tr.m, tr.v, tr.slabs


def _encoder_run(c):
    def run(seed):
        import srfrd_amd
        from oracle import srfrd_oracle as O
        from tests import grad_refs as G
        from tests import test_gpu_bf16_families as F
        from tests.gpu_util import build_model, cuda
        ref = G.reference(c.id, "autograd")                      # (weights, batch and the fp64 bar of the table gradient)
        G.assert_admissible(ref, f"case {c.id} autograd")
        torch.manual_seed(seed)
        out, checks = {}, {}
        with _env(c.switch):
            model = build_model(ref.cfg, {k: v.clone() for k, v in ref.sd.items()})
            assert not model.bf16_table
            batch = cuda(*ref.batch)
            model.eval()
            with torch.no_grad():
                ids = model._prep(*((batch[0], None, batch[2], None, batch[4], None) if ref.cfg.kind == "SASRec" else batch))
                F._assert_plan(c, model, "eval", (c.eval_fwd, None))
                for k, v in _enc_forward(model, ids, 0.0, 0, False).items():
                    out[f"eval.{k}"] = v
                F._assert_plan(c, model, "last", (c.last_fwd, None))
                out["last.hidden"] = model._launch_fwd_last(ids[0], ids[1])
                # the training forward with dropout 0.5: outputs and the three checkpoint planes
                for k, v in _enc_forward(model, ids, 0.5, 0x5EED0 + seed, True).items():
                    out[f"train.{k}"] = v
            # the module path under autograd (dropout 0): p.grad of every parameter
            model.train()
            F._assert_plan(c, model, "autograd", c.autograd)
            _, pl, nl = model(None, *batch)
            F._bce(pl, nl, batch[2]).backward()
            item = O.key_item(ref.cfg)
            for k, q in model.named_parameters():
                out[f"autograd.grad.{k}"] = q.grad
            assert listed("encoder-" + c.id, f"autograd.grad.{item}")

            def table_bar(g, name=item):
                fig = G.tensor_figures(name, g, ref.g64[name], ref.g32[name], ref.cfg.D, kbias=True, clamp=ref.clamp)
                assert not G.failures(fig), (c.id, name, G.failures(fig), fig)
            checks[f"autograd.grad.{item}"] = table_bar
            # one fused step, deterministic, eager and captured
            for graph in (False, True):
                m2 = build_model(G.cfg_of(c, "fused"), {k: v.clone() for k, v in ref.sd.items()}).train()
                tr = srfrd_amd.FusedTrainer(m2, batch_size=c.B, seq_len=c.L, seed=G.BASE, use_graph=graph, deterministic=True)
                F._assert_plan(c, m2, "fused", c.fused, scratch=tr.n_scratch)
                loss = tr.step(None, *batch).clone()
                _trainer_outputs(out, "fused." + ("graph" if graph else "eager"), [loss], m2, tr)
            return _cpu(out), checks
    return run


# workgroup widths of the encoder kernel families (threads; the template's wave count times 64): what 0x0f0f has to split.
# The two 256-thread kernels that live in encoder units have no workgroup barrier (tests/test_skew_cover.py reads that off
# their source): no mask changes them.
ENCODER_WIDTHS = {
    "encoder_fwd_kernel<NW=8>": 512, "encoder_fwd_kernel<NW=16>": 1024, "encoder_fwd_kernel<generic>": 512,
    "encoder_bwd_kernel<NW=8>": 512, "encoder_bwd_kernel<generic>": 512,
    "encoder_fwd_rows_kernel": ("kRowWaves", 64), "encoder_bwd_slots_kernel": ("kSlotWaves", 64),
    "encoder_bwd_chunks_kernel": ("kCkWaves", 64),
    "encoder_fwd_ragged_kernel": 512, "encoder_bwd_ragged_kernel": 512, "encoder_train_ragged_kernel": 512,
}
BARRIER_FREE = {"pack_weights_kernel": "srfrd_encoder_fwd.hip", "seq_order_kernel": "srfrd_encoder_fwd_ragged.hip"}
_ENC_ENTRIES = ("srfrd_pack_weights", "srfrd_encoder_fwd", "srfrd_encoder_fwd_last", "srfrd_encoder_bwd", "srfrd_reduce_dense",
                "srfrd_check_ids", "srfrd_step_begin", "srfrd_table_reduce", "srfrd_adam_pack_step")


def _register_encoders():
    from tests import grad_refs as G
    for c, cid in zip(G.ALL_CASES, G.case_ids()):
        # (under even / odd the encoder kernels are the 0x0f0f ones; the reductions and the optimizer behind them change)
        _register("encoder-" + cid, _encoder_run(c), ENCODER_LIBS, _ENC_ENTRIES, ("srfrd_optim.hip",), tuple(ENCODER_WIDTHS))


# ---- the one-launch train kernel at seq_len 50 ----------------------------------------------------------------------------------
TRAIN_I, TRAIN_L, TRAIN_STEPS = 400, 50, 2


def _launch_train_sched(tr):
    """the step's one launch through srfrd_seq_order + srfrd_encoder_train_sched (FusedTrainer itself takes
    srfrd_encoder_train_ranked, which ranks the batch inside the kernel)"""
    from srfrd_amd._lib import call

    def launch(slot):
        call("srfrd_seq_order", input_ids=tr.ids_ring[slot][0], B=tr.B, L=tr.L, pair_stride=tr.pair_stride, sched=tr.sched)
        call("srfrd_encoder_train_sched", **tr._enc_args(slot, True), loss_part=tr.loss_part, **tr._bwd_args(None, tr.contrib),
             **tr._sched_args())
    return launch


def _train_batches(seed):
    from tests import grad_refs as G
    from tests.test_gpu_train_ranked import _mixed
    big = 4 * torch.cuda.get_device_properties(0).multi_processor_count + 37
    return {"tile": [G.tile_batch(seed + s) for s in range(TRAIN_STEPS)], "dup": [G.dup_batch(seed + s) for s in range(TRAIN_STEPS)],
            "mixed51": [_mixed(51, s) for s in range(TRAIN_STEPS)], "mixed_big": [_mixed(big, s) for s in range(TRAIN_STEPS)]}


def _train_run(kind, entry):
    def run(seed):
        import srfrd_amd
        from srfrd_amd import _lib
        from tests.test_gpu_train_ranked import SEED as BASE, _model
        out = {}
        for tag, batches in _train_batches(seed).items():
            torch.manual_seed(seed)
            model = _model(kind)                                  # dropout 0.5, I = 400
            B = batches[0][0].shape[0]
            tr = srfrd_amd.FusedTrainer(model, B, TRAIN_L, seed=BASE, use_graph=False, deterministic=True)
            assert _lib.encoder_plan_train(tr.lay, B, TRAIN_L, tr._train_mode, _lib.env_switches())[0].startswith(
                "srfrd::encoder_train_ragged_kernel<"), "the plan offers no train kernel here"
            assert tr.train_launch and tr.sched_mode == 1
            if entry == "sched":
                tr._launch_train = _launch_train_sched(tr)
            losses = [tr.step(None, *[x.cuda() for x in b]).clone() for b in batches]
            _trainer_outputs(out, tag, losses, model, tr)
            out = {k: v.detach().cpu().clone() for k, v in out.items()}       # (the large batch's slabs leave the device here)
        return _cpu(out), {}
    return run


for _kind in ("SASRec", "SRFRN"):
    for _entry in ("sched", "ranked"):
        _register(f"train_kernel-{_kind}-{_entry}", _train_run(_kind, _entry), ENCODER_LIBS,
                  ("srfrd_encoder_train_" + _entry, "srfrd_table_reduce", "srfrd_reduce_dense", "srfrd_adam_pack_step")
                  + (("srfrd_seq_order",) if _entry == "sched" else ()), ("srfrd_optim.hip",), ("encoder_train_ragged_kernel",))


# ---- the three loss heads through the model methods ---------------------------------------------------------------------------------
HEAD_ITEMS, HEAD_B, HEAD_L, HEAD_K_SHARED = 301, 3, 50, 257


def _heads_run(d_item, d_fake):
    def run(seed):
        from tests import loss_refs as LR
        g = _gen(1000 * seed + 10 * d_item + d_fake)
        torch.manual_seed(seed)
        m = LR.head_model(d_item, d_fake, HEAD_ITEMS, HEAD_L, table=torch.randn(HEAD_ITEMS + 1, d_item, generator=g) * 0.5)
        h = _randn(g, HEAD_B, HEAD_L, d_item + d_fake, scale=0.5)
        out = {}

        def head(tag, call):
            for name, t in zip(("token_loss", "d_hidden", "d_table"), LR.run_head(m, call, h)):
                out[f"{tag}.{name}"] = t

        y, _ = LR.make_inputs(HEAD_B, HEAD_L, 1, HEAD_ITEMS, seed)
        yc = y.cuda()
        head("softmax", lambda hh: m.full_catalog_loss(hh, yc, "none"))
        neg = LR.shared_negatives(HEAD_K_SHARED, HEAD_ITEMS, y, seed + 1)
        assert bool((neg.view(-1, 1, 1) == y).any()), "no accidental hit among the shared negatives"
        lq = _randn(g, HEAD_K_SHARED, scale=2.0)
        negc = neg.cuda()
        head("sampled", lambda hh: m.sampled_softmax_loss(hh, yc, negc, lq, True, "none"))
        for K in (1, 6):
            yk, nk = LR.make_inputs(HEAD_B, HEAD_L, K, HEAD_ITEMS, seed + 10 + K)
            yk, nk, lqk = yk.cuda(), nk.cuda(), _randn(g, HEAD_B, HEAD_L, K, scale=2.0)
            head(f"token_softmax.K{K}", lambda hh: m.token_negatives_loss(hh, yk, nk, "softmax", lqk, 1.0, True, "none"))
            if not d_fake:                                        # (gBCE is refused for SRFRN)
                head(f"gbce.K{K}", lambda hh: m.token_negatives_loss(hh, yk, nk, "gbce", None, 0.6, True, "none"))
        return _cpu(out), {}
    return run


for _d, _f in ((50, 0), (50, 5), (64, 0)):
    _register(f"loss_heads-{_d}+{_f}", _heads_run(_d, _f), OTHER_LIBS,
              ("srfrd_xent_fwd", "srfrd_xent_bwd", "srfrd_sxent_fwd", "srfrd_sxent_bwd", "srfrd_tneg_fwd", "srfrd_tneg_bwd",
               "srfrd_table_reduce", "srfrd_table_reduce_rank1", "srfrd_check_ids"),
              ("srfrd_xent.hip", "srfrd_sxent.hip", "srfrd_tneg.hip", "srfrd_optim.hip"))


# ---- the first two fused steps of the four catalog losses ------------------------------------------------------------------------
STEP_I, STEP_B, STEP_L, STEP_K_TOKEN = 300, 6, 50, 6


def _loss_step_run(loss):
    def run(seed):
        import srfrd_amd
        from tests import grad_refs as G
        out = {}
        batches = [srfrd_amd.synthetic_batch(STEP_I, STEP_L, STEP_B, seed=50 + seed + s, device="cpu") for s in range(2)]
        kw = {}
        if loss == "sampled_softmax":
            kw = dict(num_negatives=HEAD_K_SHARED, neg_counts=torch.arange(STEP_I + 1.0) ** 0.5, neg_alpha=0.75)
        elif loss in G.TOKEN_LOSSES:
            kw = dict(num_negatives=STEP_K_TOKEN, gbce_beta=G.GBCE_BETA)
        for graph in (False, True):
            torch.manual_seed(seed)
            model = srfrd_amd.SASRec(STEP_I, STEP_L, 50, 0.5, 2, 1, "cuda")
            for _, q in model.named_parameters():
                if q.dim() >= 2:
                    torch.nn.init.xavier_normal_(q.data)
            model = model.cuda().train()
            tr = srfrd_amd.FusedTrainer(model, STEP_B, STEP_L, seed=G.BASE, use_graph=graph, deterministic=True, loss=loss, **kw)
            losses, tag = [], f"{loss}.{'graph' if graph else 'eager'}"
            for s, b in enumerate(batches):
                seq, rsq, pos, prs = (x.cuda() for x in b[1:5])
                if loss in G.TOKEN_LOSSES:
                    neg, lq = G.token_negatives(G.BY_ID["t0"], b[3], STEP_K_TOKEN, seed + s)
                    losses.append(tr.step(None, seq, rsq, pos, prs, neg.cuda(), None, lq.cuda()).clone())
                else:
                    losses.append(tr.step(None, seq, rsq, pos, prs, None, None).clone())
                if loss == "sampled_softmax":                    # what the step drew on the device
                    out[f"{tag}.negatives.{s}"], out[f"{tag}.log_q.{s}"] = tr.negatives, tr.log_q
            _trainer_outputs(out, tag, losses, model, tr)
        return _cpu(out), {}
    return run


_STEP_ENTRIES = {"softmax": ("srfrd_xent_fwd", "srfrd_xent_bwd", "srfrd_table_reduce"),
                 "sampled_softmax": ("srfrd_shared_negatives", "srfrd_sxent_fwd", "srfrd_sxent_bwd", "srfrd_table_reduce"),
                 "token_softmax": ("srfrd_tneg_fwd", "srfrd_tneg_bwd", "srfrd_table_reduce_mixed"),
                 "gbce": ("srfrd_tneg_fwd", "srfrd_tneg_bwd", "srfrd_table_reduce_mixed")}
_STEP_SOURCES = {"softmax": ("srfrd_xent.hip",), "sampled_softmax": ("srfrd_sxent.hip", "srfrd_negs.hip"),
                 "token_softmax": ("srfrd_tneg.hip",), "gbce": ("srfrd_tneg.hip",)}
for _loss in _STEP_ENTRIES:
    _register("loss_step-" + _loss, _loss_step_run(_loss), OTHER_LIBS,
              _STEP_ENTRIES[_loss] + ("srfrd_encoder_fwd_sched", "srfrd_encoder_bwd_sched", "srfrd_seq_order", "srfrd_reduce_dense",
                                      "srfrd_adam_pack_step", "srfrd_loss_finalize"),
              _STEP_SOURCES[_loss] + ("srfrd_optim.hip",))


# ---- the table reductions ---------------------------------------------------------------------------------------------------------
RED_N, RED_D, RED_D_OUT, RED_ITEMS, RED_RPT = 2000, 50, 55, 1400, 5
SENTINEL = -7.25


def _reduce_keys(g):
    """2000 keys: one key 600 times (more than two segments of SRFRD_TNEG_SPLIT_ROWS = 256: the merge kernel runs), 150 times
    key 0, 250 keys that occur once each, the rest drawn from 40 ids; shuffled"""
    from srfrd_amd import _lib
    assert 600 > 2 * _lib.TNEG_SPLIT_ROWS
    keys = torch.cat([torch.full((600,), 7), torch.zeros(150, dtype=torch.int64), torch.arange(1000, 1250),
                      torch.randint(100, 140, (RED_N - 1000,), generator=g)])
    return keys[torch.randperm(RED_N, generator=g)].contiguous()


def _table_reduce_run(seed):
    from srfrd_amd import loss_heads
    g = _gen(seed)
    keys = _reduce_keys(g).cuda()
    skeys, order = torch.sort(keys, stable=True)
    rows, coef = _randn(g, RED_N, RED_D), _randn(g, RED_N)
    hidden = _randn(g, RED_N // RED_RPT, RED_D_OUT)
    ws_n = loss_heads.mixed_workspace(RED_N, RED_D)
    assert ws_n > 0
    out = {}

    def table():
        return torch.full((RED_ITEMS + 1, RED_D), SENTINEL, device="cuda")
    G = out["table_reduce"] = table()
    _ok(_L().srfrd_table_reduce(_p(skeys), _p(order), _p(rows), RED_N, RED_D, _p(G), _st()), "srfrd_table_reduce")
    G, ws = out["rank1"], out["rank1.workspace"] = table(), torch.zeros(ws_n, device="cuda")
    _ok(_L().srfrd_table_reduce_rank1(_p(skeys), _p(order), _p(coef), _p(hidden), RED_D_OUT, RED_RPT, RED_N, RED_D, _p(G), _p(ws),
                                      ws_n, _st()), "srfrd_table_reduce_rank1")
    n_rows = 500                                                  # 500 full rows, then 1500 rank-1 rows over 300 hidden rows
    G, ws = out["mixed"], out["mixed.workspace"] = table(), torch.zeros(ws_n, device="cuda")
    _ok(_L().srfrd_table_reduce_mixed(_p(skeys), _p(order), RED_N, _p(rows), n_rows, _p(coef), _p(hidden), RED_D_OUT, RED_RPT, RED_D,
                                      _p(G), _p(ws), ws_n, _st()), "srfrd_table_reduce_mixed")
    return _cpu(out), {}


_register("table_reduce", _table_reduce_run, OTHER_LIBS,
          ("srfrd_table_reduce", "srfrd_table_reduce_rank1", "srfrd_table_reduce_mixed"), ("srfrd_optim.hip", "srfrd_tneg.hip"))


# ---- the optimizer and the gradient reductions --------------------------------------------------------------------------------------
OPT_N = 3 * 4096 + 1027            # not a multiple of 4, four shares of srfrd_grad_norm


def _optimizer_run(seed):
    from srfrd_amd import _lib
    assert OPT_N % 4 and OPT_N > _lib.GRAD_NORM_SHARE
    g = _gen(seed)
    out = {}
    f32 = dict(device="cuda", dtype=torch.float32)
    # srfrd_reduce_dense at 3 and 300 slabs, with the loss partials of B = 1 and 257; srfrd_loss_stats on the same partials
    for n_slabs, B in ((3, 1), (300, 257)):
        slabs = _randn(g, n_slabs, OPT_N)
        lp = torch.stack([torch.rand(B, generator=g) * 20, torch.rand(B, generator=g) * 20,
                          torch.randint(1, 50, (B,), generator=g).float()], 1).cuda().contiguous()
        grad, stats, loss = torch.zeros(OPT_N, **f32), torch.zeros(4, **f32), torch.zeros(1, **f32)
        _ok(_L().srfrd_reduce_dense(_p(slabs), n_slabs, OPT_N, _p(grad), _p(lp), B, _p(stats), _p(loss), _st()), "srfrd_reduce_dense")
        out[f"reduce_dense.{n_slabs}.grad"], out[f"reduce_dense.{n_slabs}.stats"], out[f"reduce_dense.{n_slabs}.loss"] = grad, stats, loss
        stats2, loss2 = torch.zeros(4, **f32), torch.zeros(1, **f32)
        _ok(_L().srfrd_loss_stats(_p(lp), B, _p(stats2), _p(loss2), _st()), "srfrd_loss_stats")
        out[f"loss_stats.{B}.stats"], out[f"loss_stats.{B}.loss"] = stats2, loss2
    stats = torch.tensor([2.0, 3.0, 41.0, 0.0]).cuda()
    # srfrd_grad_norm, clipping (the norm of ~115 standard normals over 41 is above 1) and not
    grad = _randn(g, OPT_N)
    for tag, max_norm in (("clip", 1.0), ("measure", float("inf"))):
        part, res = torch.zeros(_lib.GRAD_NORM_PARTIALS, device="cuda", dtype=torch.float64), torch.zeros(2, **f32)
        _ok(_L().srfrd_grad_norm(_p(grad), OPT_N, _p(stats), max_norm, _p(part), _p(res), _st()), "srfrd_grad_norm")
        out[f"grad_norm.{tag}"], out[f"grad_norm.{tag}.partials"] = res, part
        if tag == "clip":
            clip = res
    # srfrd_l2_norms / srfrd_l2_apply: the table and five dense tensors with alignment gaps
    n_tab = 5003
    ntp = (n_tab + 3) // 4 * 4
    segs, o = [(0, n_tab)], ntp
    for ln in (50, 2500, 1, 3000, 777):
        segs.append((o + 1, ln))
        o += 1 + ln
    assert o <= OPT_N
    param = _randn(g, OPT_N)
    so = torch.tensor([a for a, _ in segs]).cuda()
    sl = torch.tensor([b for _, b in segs]).cuda()
    part, l2buf, ds = torch.zeros(240 + len(segs), **f32), torch.zeros(2, **f32), torch.zeros(OPT_N - ntp, **f32)
    _ok(_L().srfrd_l2_norms(_p(param), _p(so), _p(sl), len(segs), ntp, 1e-3, _p(part), _p(l2buf), _p(ds), _st()), "srfrd_l2_norms")
    g2 = grad.clone()
    _ok(_L().srfrd_l2_apply(_p(g2), _p(param), 0, OPT_N, ntp, _p(l2buf), _p(ds), _p(stats), _st()), "srfrd_l2_apply")
    out["l2.partials"], out["l2.buf"], out["l2.dense_scale"], out["l2.grad"] = part, l2buf, ds, g2
    # srfrd_step_begin / _sched, then srfrd_adam_step and srfrd_adamw_step over the whole vector with a bf16 shadow
    opts = _lib.OptimOpts(2e-3, 0.9, 0.98, 0.01, 0.1, 3, 20, _lib.SCHEDULES["cosine"], 0)
    for tag, w in (("adam", False), ("adamw", True)):
        state = torch.zeros(32, device="cuda", dtype=torch.int32)
        state[0], state[1] = 4, 12345
        if w:
            _ok(_L().srfrd_step_begin_sched(_p(state), C.byref(opts), _st()), "srfrd_step_begin_sched")
        else:
            _ok(_L().srfrd_step_begin(_p(state), 2e-3, 0.9, 0.98, _st()), "srfrd_step_begin")
        P, Gr, M, V = param.clone(), grad.clone(), _randn(g, OPT_N, scale=0.1), _randn(g, OPT_N, scale=0.05).abs()
        H = torch.zeros(n_tab, device="cuda", dtype=torch.int16)
        if w:
            _ok(_L().srfrd_adamw_step(_p(P), _p(Gr), _p(M), _p(V), OPT_N, 0, OPT_N, ntp, 0.9, 0.98, 1e-8, _p(state), _p(stats), _p(clip),
                                      _p(H), n_tab, _st()), "srfrd_adamw_step")
        else:
            _ok(_L().srfrd_adam_step(_p(P), _p(Gr), _p(M), _p(V), OPT_N, 0, OPT_N, ntp, 0.9, 0.98, 1e-8, _p(state), _p(stats), _p(H), n_tab,
                                     _st()), "srfrd_adam_step")
        for k, t in (("param", P), ("grad", Gr), ("m", M), ("v", V), ("shadow", H), ("state", state)):
            out[f"{tag}_step.{k}"] = t
    # srfrd_adam_pack_step / srfrd_adamw_pack_step (512 threads): two launches each on a real layout - 24 workgroups, so all
    # sixteen shard counters state[8 + shard] and the root state[6] count and are put back
    lay = _lib.make_layout("SRFRN", 300, 20, 45, 5, 0, 2, 1)
    ntp = (lay.n_table + 3) // 4 * 4
    n = (ntp + lay.n_dense + 3) // 4 * 4
    assert min(((n >> 2) + 1 + 511) // 512, 768) >= 16
    n_packed = _L().srfrd_packed_floats(C.byref(lay))
    for tag, w in (("adam_pack", False), ("adamw_pack", True)):
        state = torch.zeros(32, device="cuda", dtype=torch.int32)
        state[1] = 777
        if w:
            _ok(_L().srfrd_step_begin_sched(_p(state), C.byref(opts), _st()), "srfrd_step_begin_sched")
        else:
            _ok(_L().srfrd_step_begin(_p(state), 2e-3, 0.9, 0.98, _st()), "srfrd_step_begin")
        P, M, V = _randn(g, n), _randn(g, n, scale=0.1), _randn(g, n, scale=0.05).abs()
        packed, H = torch.zeros(n_packed, **f32), torch.zeros(lay.n_table, device="cuda", dtype=torch.int16)
        _ok(_L().srfrd_pack_weights(C.byref(lay), _p(P, 4 * ntp), _p(packed), None, 0.0, 0.0, 0.0, _st()), "srfrd_pack_weights")
        for launch in range(2):
            Gr = _randn(g, n)
            if w:
                _ok(_L().srfrd_adamw_pack_step(C.byref(lay), _p(P), _p(Gr), _p(M), _p(V), n, ntp, ntp, C.byref(opts), 1e-8, _p(state),
                                               _p(stats), _p(clip), _p(packed), _p(H), _st()), "srfrd_adamw_pack_step")
            else:
                _ok(_L().srfrd_adam_pack_step(C.byref(lay), _p(P), _p(Gr), _p(M), _p(V), n, ntp, ntp, 2e-3, 0.9, 0.98, 1e-8, _p(state),
                                              _p(stats), _p(packed), _p(H), _st()), "srfrd_adam_pack_step")
            out[f"{tag}.{launch}.state"], out[f"{tag}.{launch}.grad"] = state.clone(), Gr
        for k, t in (("param", P), ("m", M), ("v", V), ("packed", packed), ("shadow", H)):
            out[f"{tag}.{k}"] = t
    # srfrd_table_to_bf16
    H = torch.zeros(OPT_N, device="cuda", dtype=torch.int16)
    _ok(_L().srfrd_table_to_bf16(_p(param), OPT_N, _p(H), _st()), "srfrd_table_to_bf16")
    out["table_to_bf16"] = H
    res = _cpu(out)
    for tag in ("adam_pack", "adamw_pack"):
        for launch in range(2):
            s = res[f"{tag}.{launch}.state"]
            assert int(s[6]) == 0 and not bool(s[8:24].any()) and int(s[0]) == launch + 2, (tag, launch, s)
    return res, {}


_register("optimizer", _optimizer_run, OTHER_LIBS,
          ("srfrd_reduce_dense", "srfrd_loss_stats", "srfrd_grad_norm", "srfrd_l2_norms", "srfrd_l2_apply", "srfrd_step_begin",
           "srfrd_step_begin_sched", "srfrd_adam_step", "srfrd_adamw_step", "srfrd_adam_pack_step", "srfrd_adamw_pack_step",
           "srfrd_table_to_bf16", "srfrd_pack_weights"), ("srfrd_optim.hip",))


# ---- ranking on the three table routes --------------------------------------------------------------------------------------------
RANK_ITEMS, RANK_L = 3000, 20
ROUTES = {"bf16": (50, True), "fp32_split": (50, False), "fp32_mfma": (64, False)}


def _ranking_run(route):
    d_item, bf16 = ROUTES[route]

    def run(seed):
        import srfrd_amd
        from srfrd_amd import _lib, ops
        from srfrd_amd._lib import check
        from srfrd_amd.ranker import ShardedRanker
        from tests import rank_refs as RR
        assert RR.is_stream16(d_item, "bf16" if bf16 else "fp32") == (route != "fp32_mfma")
        torch.manual_seed(seed)
        model = srfrd_amd.SASRec(RANK_ITEMS, RANK_L, d_item, 0.0, 2, 1, "cuda")
        for _, q in model.named_parameters():
            if q.dim() >= 2:
                torch.nn.init.xavier_normal_(q.data)
        model = model.cuda().eval()
        if bf16:
            model.use_bf16_table()
        g = _gen(seed + 7)
        out, checks = {}, {}
        with _env(None), torch.no_grad():
            for B in (1, 37):
                _, seq, rsq = srfrd_amd.synthetic_batch(RANK_ITEMS, RANK_L, B, seed=seed + B, device="cuda")[:3]
                # exclusion sets: row 0 at the cap (with duplicates), the last row empty, the others the user's own inputs
                rows = [torch.randint(1, RANK_ITEMS + 1, (_lib.EXCL_CAP,), generator=g)]
                rows += [seq[b][seq[b] != 0].cpu() for b in range(1, B)]
                rows[-1] = torch.zeros(0, dtype=torch.int64) if B > 1 else rows[-1]
                for k in (1, 10, 64):
                    out[f"B{B}.topk{k}.idx"], out[f"B{B}.topk{k}.val"] = model.topk(None, seq, rsq, k=k)
                    out[f"B{B}.topk{k}.excl.idx"], out[f"B{B}.topk{k}.excl.val"] = model.topk(None, seq, rsq, k=k, exclude=rows)
                targets = torch.randint(1, RANK_ITEMS + 1, (B,), generator=g).cuda()
                out[f"B{B}.target_rank"] = model.target_rank(None, seq, rsq, targets)
                out[f"B{B}.target_rank.excl"] = model.target_rank(None, seq, rsq, targets, exclude=rows)
                cand = torch.randint(1, RANK_ITEMS + 1, (B, 101), generator=g).cuda()
                logits = model.predict(None, seq, rsq, cand).reshape(B, 101)
                out[f"B{B}.predict"] = logits
                # srfrd_eval_rank and srfrd_target_rank with their metric sums
                rank, acc = torch.zeros(B, device="cuda", dtype=torch.int32), torch.zeros(3, device="cuda", dtype=torch.float64)
                check(_L().srfrd_eval_rank(_p(logits.contiguous()), B, 101, _p(rank), _p(acc), _st()), "srfrd_eval_rank")
                out[f"B{B}.eval_rank"], out[f"B{B}.eval_rank.metric_acc"] = rank, acc
                hidden = model._launch_fwd_last(*model._prep(seq, None, None, None, None, None)[:2])
                lay, tab = model._table_args()
                ws = torch.zeros(max(_L().srfrd_excl_workspace_bytes(B, 0, RANK_ITEMS + 1), 8), device="cuda", dtype=torch.uint8)
                rank2, acc2 = torch.zeros(B, device="cuda", dtype=torch.int32), torch.zeros(3, device="cuda", dtype=torch.float64)
                check(_L().srfrd_target_rank(C.byref(lay), tab, _p(model._flat, 4 * model.n_table_pad), _p(hidden), B, 1, 0,
                                             RANK_ITEMS + 1, 1, None, _p(targets), None, None, 0, 10, _p(rank2), _p(acc2), _p(ws), _st()),
                      "srfrd_target_rank")
                out[f"B{B}.target_metric.rank"], out[f"B{B}.target_metric.metric_acc"] = rank2, acc2
                # three row shards ranked one after the other and merged (srfrd_topk_merge)
                out[f"B{B}.sharded.idx"], out[f"B{B}.sharded.val"] = ShardedRanker(model, n_shards=3).topk(None, seq, rsq, k=10)
                for kind in ("SRFRN", "SRFU_B", "SRFU_F", "SRFU_R"):
                    out[f"B{B}.user_labels.{kind}"] = torch.ops.srfrd.user_labels(rsq.contiguous(), _lib.KINDS[kind])
        res = _cpu(out)
        for B in (1, 37):
            checks[f"B{B}.eval_rank.metric_acc"] = metric_check(res[f"B{B}.eval_rank"])
            checks[f"B{B}.target_metric.metric_acc"] = metric_check(res[f"B{B}.target_metric.rank"])
        return res, checks
    return run


for _route in ROUTES:
    _register("ranking-" + _route, _ranking_run(_route), OTHER_LIBS,
              ("srfrd_encoder_fwd_last", "srfrd_logits_topk", "srfrd_logits_topk_excl", "srfrd_target_rank", "srfrd_predict_logits",
               "srfrd_eval_rank", "srfrd_topk_merge", "srfrd_user_labels", "srfrd_check_ids")
              + (("srfrd_table_to_bf16",) if ROUTES[_route][1] else ()), ("srfrd_rank.hip", "srfrd_optim.hip"))


# ---- the samplers -----------------------------------------------------------------------------------------------------------------------
SAMPLE_ITEMS = 6000


def _sampler_histories():
    """users 0..4 in a 6000-item catalog: no history, 1 item, 40 distinct items, 5000 draws from 3000 items (the LDS set holds
    ~2400 distinct ids in 16384 slots, filled by atomicCAS in an arbitrary order), 12 items"""
    rng = np.random.RandomState(3)
    p = rng.permutation(SAMPLE_ITEMS) + 1
    return [[], [5], list(p[:40]), list(rng.choice(p[100:3100], 5000, replace=True)), list(p[4000:4012])]


def _samplers_run(seed):
    import srfrd_amd
    from srfrd_amd import _lib
    from srfrd_amd.sampler import alias_table, negative_q
    from tests import token_neg_refs as R
    from tests.test_gpu_token_neg import Case
    out = {}
    hist = _sampler_histories()
    # srfrd_sample_batch through DeviceSampler, two batches
    data = R.interaction_data(hist, SAMPLE_ITEMS)
    sampler = srfrd_amd.DeviceSampler(data, 37, 20, seed=seed, device="cuda")
    for i in range(2):
        user, packed = sampler.next_batch(packed=True)
        out[f"sample_batch.{i}.user"], out[f"sample_batch.{i}.ids"] = user, packed
    # srfrd_shared_negatives, uniform and alias
    K = HEAD_K_SHARED
    state = torch.zeros(32, device="cuda", dtype=torch.int32)
    state[2] = 0x0C0FFEE1
    q = negative_q(SAMPLE_ITEMS, R.counts_with_zeros(SAMPLE_ITEMS))
    prob, idx = alias_table(q)
    with np.errstate(divide="ignore"):
        ilq = torch.from_numpy(np.concatenate([[0.0], np.log(K * q)]).astype(np.float32)).cuda()
    prob, idx = torch.from_numpy(prob).cuda(), torch.from_numpy(idx).cuda()
    for tag, args in (("uniform", (None, None, None)), ("alias", (_p(prob), _p(idx), _p(ilq)))):
        ids, lq = torch.zeros(K, device="cuda", dtype=torch.int64), torch.zeros(K, device="cuda")
        _ok(_L().srfrd_shared_negatives(_p(state), SAMPLE_ITEMS, K, *args, _p(ids), _p(lq), _st()), "srfrd_shared_negatives")
        out[f"shared_negatives.{tag}.ids"], out[f"shared_negatives.{tag}.log_q"] = ids, lq
    # srfrd_token_negatives with exclusion: every history length, alias table and user_log_keep, 320 slots per row
    for alias in (False, True):
        case = Case(hist, SAMPLE_ITEMS, [3, 1, 2, 3, 0, 4, 99], 20, alias=alias, dead_row=4, seed=20240611 + seed)
        assert case.max_true == 5000 <= _lib.TNEG_MAX_HIST
        for exclude in (1, 0):
            ids, lq = case.launch(16, case.max_true, index=3, exclude=exclude, seed=20240611 + seed)
            tag = f"token_negatives.{'alias' if alias else 'uniform'}.{'excl' if exclude else 'all'}"
            out[f"{tag}.ids"], out[f"{tag}.log_q"] = torch.from_numpy(ids), torch.from_numpy(lq)
    return _cpu(out), {}


_register("samplers", _samplers_run, OTHER_LIBS, ("srfrd_sample_batch", "srfrd_shared_negatives", "srfrd_token_negatives"),
          ("srfrd_rank.hip", "srfrd_negs.hip", "srfrd_tneg_sample.hip"))

_register_encoders()

# ---------------------------------------------------------------------------------------------------------------------------
# what tests/test_skew_cover.py reads
# ---------------------------------------------------------------------------------------------------------------------------
# entry points that launch nothing: answers computed on the host (their declarations take no stream)
HOST_ONLY = ("srfrd_layout_init", "srfrd_lds_bytes", "srfrd_scratch_floats", "srfrd_bwd_grid", "srfrd_debug_shape",
             "srfrd_packed_floats", "srfrd_sched_ints", "srfrd_encoder_plan", "srfrd_encoder_plan_train", "srfrd_train_scratch_floats",
             "srfrd_aux_floats", "srfrd_topk_workspace_bytes", "srfrd_excl_workspace_bytes", "srfrd_rank_plan",
             "srfrd_xent_workspace_floats", "srfrd_sxent_workspace_floats", "srfrd_tneg_workspace_floats",
             "srfrd_table_reduce_mixed_workspace_floats")
# launching entry points no exerciser names, each with its reason
EXEMPT = {
    "srfrd_skew_mask": "the probe itself: one thread, no barrier; test_gpu_skew_bits.test_every_library_runs_its_own_code calls it "
                       "through every handle",
}


def non_encoder_sources():
    import __graft_entry__ as g
    return list(g.SPLIT_SOURCES)


def _includes(src):
    """a source file's text with the project headers it includes spliced in after it (srfrd_dev.h aside: it has no kernel)"""
    text = open(os.path.join(CSRC, src)).read()
    for inc in re.findall(r'#include "(srfrd_[a-z_]+\.h)"', text):
        if inc != "srfrd_dev.h":
            text += "\n" + _includes(inc)
    return text


def constants(text):
    """{name: value} of the integer constants a width is written with: ``constexpr int kName = <integer expression>;``"""
    out = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(k\w+)\s*=\s*([^;]+);", text):
        try:
            out[name] = int(eval(expr, {"__builtins__": {}}, dict(out)))        # (digits, names above, + * only)
        except Exception:                                                      # noqa: BLE001 - not an integer expression
            pass
    return out


def launch_widths(src):
    """the workgroup widths of the kernels of one non-encoder source, named constants resolved: every first argument of a
    __launch_bounds__ in the file and the headers it includes.  An expression that does not resolve raises."""
    text = _includes(src)
    names = constants(text)
    widths = set()
    for expr in re.findall(r"__launch_bounds__\(([^,)]+)", text):
        widths.add(int(eval(expr, {"__builtins__": {}}, dict(names))))
    return widths


def splits(mask, width):
    """mask delays some but not all of waves 0 .. width / 64 - 1"""
    waves = (width + 63) // 64
    group = (1 << waves) - 1
    return 0 < (mask & group) < group


def complementary(mask_a, mask_b, width):
    group = (1 << ((width + 63) // 64)) - 1
    return (mask_a & group) == (~mask_b & group)
