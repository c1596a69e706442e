"""-m gpu: every public path asks the library for the same C entry points, in the same order, as it always has.

An ordered recorder stands in ``_lib._lib`` (the seam tests/skew_cases.use swaps a library in by) and notes every name asked of
the handle, size and plan queries included, while a path runs once at the smallest shapes: SRFRN 45 + 5 over 300 items, B = 4,
L = 20 (its fake planes exercise pos_fake / neg_fake), and SASRec 50, B = 8, L = 50 (the one-launch train kernel exists only at
that length).  The expected lists below were recorded on the commit before the Python layer went over to calls by parameter
name (``_lib.call``); the test uses nothing but that seam, so it holds for both sides of that change and for every later one.
Four lists came later, with the trainer's one key sort: ``lazy_table`` and ``softmax`` with ``deterministic``, read off the
launches of the commit before it, and the step cut into three stages at an eager sort (``deterministic``,
``sampled_softmax``), which must ask for exactly what the one-stage step asks for."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"srfrn20": ("SRFRN", 300, 20, 4), "sasrec50": ("SASRec", 300, 50, 8)}     # kind, items, L, B


class Ordered:
    """a library handle that notes, in order, the entry points asked of it"""

    def __init__(self, handle):
        object.__setattr__(self, "_handle", handle)
        object.__setattr__(self, "names", [])

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._handle, name)


@contextlib.contextmanager
def recorded():
    from srfrd_amd import _lib
    rec = Ordered(_lib.lib())
    old = _lib._lib
    _lib._lib = rec
    try:
        yield rec
        torch.cuda.synchronize()
    finally:
        _lib._lib = old


def _model(shape):
    import srfrd_amd
    kind, items, L, B = SHAPES[shape]
    torch.manual_seed(0)
    m = srfrd_amd.SRFRN(items, L, 45, 5, 0.0, 2, 1, "cuda") if kind == "SRFRN" else srfrd_amd.SASRec(items, L, 50, 0.0, 2, 1, "cuda")
    for _, p in m.named_parameters():
        if p.dim() >= 2:
            torch.nn.init.xavier_normal_(p.data)
    batch = srfrd_amd.synthetic_batch(items, L, B, seed=3, device="cuda")[1:]      # seq, rsq, pos, prs, neg, nrs
    return m.to("cuda"), batch


def _autograd(library_ops):
    def run():
        m, batch = _model("srfrn20")
        m.train()
        m.library_ops = library_ops
        _, pl, nl = m(None, *batch)
        (pl.sum() - nl.sum()).backward()
    return run


def _step(shape, sort_limit=None, **options):
    """``sort_limit``: srfrd_amd.trainer.SORT_CAPTURE_LIMIT while the trainer is built (0: the program with the eager key sort)"""
    def run():
        import srfrd_amd
        from srfrd_amd import trainer
        m, batch = _model(shape)
        m.train()
        _, _, L, B = SHAPES[shape]
        with pytest.MonkeyPatch.context() as mp:
            if sort_limit is not None:
                mp.setattr(trainer, "SORT_CAPTURE_LIMIT", sort_limit)
            tr = srfrd_amd.FusedTrainer(m, B, L, use_graph=False, **options)
        assert len(tr._program) == (3 if sort_limit == 0 else 1)
        tr.step(None, *batch)
    return run


def _rank(what):
    def run():
        import srfrd_amd
        m, batch = _model("srfrn20")
        m.eval()
        seq, rsq, pos = batch[0], batch[1], batch[2]
        targets = pos[:, -1].contiguous()
        if what == "predict":
            m.predict(None, seq, rsq, torch.arange(1, 12, device="cuda"))
        elif what == "topk":
            m.topk(None, seq, rsq, k=5, exclude="input")
        elif what == "target_rank":
            m.target_rank(None, seq, rsq, targets)
        elif what == "sharded_topk":
            srfrd_amd.ShardedRanker(m, n_shards=2).topk(None, seq, rsq, k=5)
        else:
            srfrd_amd.ShardedRanker(m, n_shards=2).target_rank(None, seq, rsq, targets)
    return run


PATHS = {
    "autograd": _autograd(False),
    "autograd-library-ops": _autograd(True),
    "step-bce-20": _step("srfrn20"),
    "step-bce-50": _step("sasrec50"),
    "step-deterministic": _step("sasrec50", deterministic=True),
    "step-l2-emb": _step("srfrn20", l2_emb=1e-3),
    "step-sampled-softmax": _step("sasrec50", loss="sampled_softmax", num_negatives=16),
    "step-max-grad-norm": _step("srfrn20", max_grad_norm=1.0),
    "step-lazy-table": _step("sasrec50", lazy_table=True),
    "step-softmax-deterministic": _step("sasrec50", loss="softmax", deterministic=True),
    "step-deterministic-eager-sort": _step("sasrec50", sort_limit=0, deterministic=True),
    "step-sampled-softmax-eager-sort": _step("sasrec50", sort_limit=0, loss="sampled_softmax", num_negatives=16),
    "predict": _rank("predict"),
    "topk-exclude-input": _rank("topk"),
    "target-rank": _rank("target_rank"),
    "sharded-topk": _rank("sharded_topk"),
    "sharded-target-rank": _rank("sharded_target_rank"),
}


def record(path):
    with recorded() as rec:
        PATHS[path]()
    return list(rec.names)


# path -> the entry points it asks of the library, in order, each without its "srfrd_" prefix
EXPECTED = {
    "autograd": ("layout_init check_ids aux_floats packed_floats pack_weights scratch_floats encoder_fwd bwd_grid "
                 "scratch_floats encoder_bwd reduce_dense"),
    "autograd-library-ops": ("layout_init check_ids aux_floats packed_floats pack_weights scratch_floats encoder_fwd bwd_grid "
                             "scratch_floats encoder_bwd reduce_dense"),
    "step-bce-20": ("layout_init scratch_floats encoder_plan_train bwd_grid aux_floats encoder_plan bwd_grid packed_floats "
                    "pack_weights step_begin check_ids pack_weights encoder_plan_train encoder_fwd_sched encoder_bwd_sched "
                    "reduce_dense adam_pack_step"),
    "step-bce-50": ("layout_init scratch_floats encoder_plan_train train_scratch_floats bwd_grid aux_floats encoder_plan "
                    "sched_ints bwd_grid packed_floats pack_weights step_begin check_ids pack_weights encoder_plan_train "
                    "encoder_train_ranked reduce_dense adam_pack_step"),
    "step-deterministic": ("layout_init scratch_floats encoder_plan_train train_scratch_floats bwd_grid aux_floats encoder_plan "
                           "sched_ints bwd_grid packed_floats pack_weights step_begin check_ids pack_weights encoder_plan_train "
                           "encoder_train_ranked table_reduce reduce_dense adam_pack_step"),
    "step-l2-emb": ("layout_init scratch_floats encoder_plan_train bwd_grid aux_floats encoder_plan bwd_grid packed_floats "
                    "pack_weights step_begin check_ids pack_weights encoder_plan_train l2_norms encoder_fwd_sched "
                    "encoder_bwd_sched reduce_dense l2_apply adam_pack_step"),
    "step-sampled-softmax": ("layout_init scratch_floats encoder_plan_train train_scratch_floats bwd_grid aux_floats encoder_plan "
                             "sched_ints bwd_grid sxent_workspace_floats packed_floats pack_weights step_begin check_ids pack_weights "
                             "seq_order shared_negatives encoder_fwd_sched sxent_fwd sxent_bwd encoder_bwd_sched table_reduce reduce_dense "
                             "adam_pack_step loss_finalize"),
    "step-max-grad-norm": ("layout_init scratch_floats encoder_plan_train bwd_grid aux_floats encoder_plan bwd_grid packed_floats "
                           "pack_weights step_begin_sched check_ids pack_weights encoder_plan_train encoder_fwd_sched encoder_bwd_sched "
                           "reduce_dense grad_norm adamw_pack_step"),
    # (lazy Adam's row kernel sits behind the slab reduction, ahead of the dense update)
    "step-lazy-table": ("layout_init scratch_floats encoder_plan_train train_scratch_floats bwd_grid aux_floats encoder_plan "
                        "sched_ints bwd_grid packed_floats pack_weights step_begin check_ids pack_weights encoder_plan_train "
                        "encoder_train_ranked reduce_dense table_reduce_adam adam_pack_step"),
    "step-softmax-deterministic": ("layout_init scratch_floats encoder_plan_train train_scratch_floats bwd_grid aux_floats encoder_plan "
                                   "sched_ints bwd_grid xent_workspace_floats packed_floats pack_weights step_begin check_ids "
                                   "pack_weights seq_order encoder_fwd_sched xent_fwd xent_bwd encoder_bwd_sched table_reduce "
                                   "reduce_dense adam_pack_step loss_finalize"),
    "predict": ("layout_init check_ids packed_floats pack_weights scratch_floats encoder_fwd_last user_labels check_ids "
                "predict_logits"),
    "topk-exclude-input": ("layout_init check_ids packed_floats pack_weights scratch_floats encoder_fwd_last user_labels "
                           "topk_workspace_bytes excl_workspace_bytes logits_topk_excl"),
    "target-rank": ("layout_init check_ids packed_floats pack_weights scratch_floats encoder_fwd_last user_labels "
                    "excl_workspace_bytes target_rank"),
    "sharded-topk": ("layout_init check_ids packed_floats pack_weights scratch_floats encoder_fwd_last user_labels "
                     "topk_workspace_bytes logits_topk topk_workspace_bytes logits_topk topk_merge"),
    "sharded-target-rank": ("layout_init check_ids packed_floats pack_weights scratch_floats encoder_fwd_last user_labels "
                            "excl_workspace_bytes target_rank excl_workspace_bytes target_rank"),
}


# a step cut at its key sort into three stages asks for what the one-stage step asks for
EXPECTED["step-deterministic-eager-sort"] = EXPECTED["step-deterministic"]
EXPECTED["step-sampled-softmax-eager-sort"] = EXPECTED["step-sampled-softmax"]


def test_every_path_is_listed():
    assert set(EXPECTED) == set(PATHS)


@pytest.mark.parametrize("path", list(PATHS))
def test_entry_points_in_order(path):
    got = record(path)
    assert got == ["srfrd_" + n for n in EXPECTED[path].split()], (path, got)
