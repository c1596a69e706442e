"""srfrd_amd.trainer.step_program - the one place a train step's order is written - and FusedTrainer's walks over it (eager,
local, replay), on recording stubs: no device, no FusedTrainer instance.  The expected orders are the ladders the program
replaced, written out."""
import pytest

from srfrd_amd.trainer import ONE_GRAPH, FusedTrainer, step_program

G, E, X = "graph", "eager", "collective"
FORMS = {"single": ("single", False), "token": ("single", True), "allreduce": ("allreduce", False), "sharded": ("sharded", False)}

# (kind, per_slot) of every stage
SHAPES = {
    "single": [(G, True)],
    "token": [(G, True), (E, False), (G, False)],
    "allreduce": [(G, True), (X, False), (G, False)],
    "sharded": [(G, True), (X, False), (G, True), (X, False), (G, False), (X, False), (G, False)],
}

# what one eager step on slot 1 calls, in order; per stage
EAGER = {
    "single": [[("_enqueue_step_compute", 1), ("_enqueue_update",)]],
    "token": [[("_enqueue_ce_compute", 1)], [("_sort_keys",)],
              [("_enqueue_table_reduce",), ("_enqueue_ce_dense",), ("_enqueue_update",)]],
    "allreduce": [[("_enqueue_compute", 1)], [("ex.all_reduce", "grad")], [("_enqueue_update",)]],
    "sharded": [[("_enqueue_fwd", 1)], [("ex.all_reduce_stats", "stats")], [("_enqueue_bwd", 1)],
                [("ex.reduce_scatter", "grad", "recv"), ("handle.wait",)], [("_enqueue_shard_update",)],
                [("ex.all_gather", "flat_pad")], [("_enqueue_shard_finish",)]],
}


class _Handle:
    def __init__(self, log):
        self.log = log

    def wait(self):
        self.log.append(("handle.wait",))


class _Exchange:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*args):
            self.log.append(("ex." + name,) + args)
            return _Handle(self.log) if name == "all_reduce_stats" else None
        return call


class _Graph:
    def __init__(self, log, stage, slot):
        self.log, self.tag = log, ("replay", stage, slot)

    def replay(self):
        self.log.append(self.tag)


class _Trainer:
    """FusedTrainer's walks and eager stages over recorders in place of the enqueue methods and the exchange"""
    _walk, _enqueue_step, _replay = FusedTrainer._walk, FusedTrainer._enqueue_step, FusedTrainer._replay
    _all_reduce_grad, _start_stats_reduce = FusedTrainer._all_reduce_grad, FusedTrainer._start_stats_reduce
    _scatter_grad, _gather_params = FusedTrainer._scatter_grad, FusedTrainer._gather_params
    _enqueue_compute_update = FusedTrainer._enqueue_compute_update
    shadow_gather, slots = False, 2
    grad, stats, recv, flat_pad = "grad", "stats", "recv", "flat_pad"

    def __init__(self, form):
        self.log = []
        self.ex = _Exchange(self.log)
        self._stats_handle = None
        self._program = step_program(*FORMS[form])

    def __getattr__(self, name):
        if not (name.startswith("_enqueue_") or name == "_sort_keys"):
            raise AttributeError(name)
        return lambda *args: self.log.append((name,) + args)

    def captured_as(self, stages):
        self._graphs = (stages, [[_Graph(self.log, i, k) for k in range(self.slots if per_slot else 1)] if kind == G else None
                                 for i, (kind, per_slot, _) in enumerate(stages)])


def _flat(per_stage):
    return [c for stage in per_stage for c in stage]


@pytest.mark.parametrize("form", FORMS)
def test_stage_kinds_and_slot_flags(form):
    program = step_program(*FORMS[form])
    assert [(kind, per_slot) for kind, per_slot, _ in program] == SHAPES[form]
    for _, _, calls in program + ONE_GRAPH:
        assert calls and all(callable(getattr(FusedTrainer, name)) for name in calls), calls


def test_the_stages_depend_on_mode_and_token_alone():
    for mode in ("allreduce", "sharded"):              # (a cross-entropy loss trains on one rank: _loss_config refuses the rest)
        assert step_program(mode, True) == step_program(mode, False)
    assert ONE_GRAPH == [(G, True, ("_enqueue_step",))]


@pytest.mark.parametrize("form", FORMS)
def test_eager_walk_is_the_parent_order(form):
    tr = _Trainer(form)
    tr._enqueue_step(1)
    assert tr.log == _flat(EAGER[form])
    assert tr._stats_handle is None


@pytest.mark.parametrize("form", FORMS)
def test_local_walk_drops_the_collectives_and_keeps_the_sort(form):
    tr = _Trainer(form)
    tr._enqueue_step(1, local=True)
    want = _flat(calls for calls, (kind, _) in zip(EAGER[form], SHAPES[form]) if kind != X)
    assert tr.log == want
    assert not any(c[0].startswith(("ex.", "handle.")) for c in tr.log)
    assert (("_sort_keys",) in tr.log) == (form == "token")


@pytest.mark.parametrize("form", FORMS)
def test_replay_walk_calls_the_eager_stages_between_graph_replays(form):
    tr = _Trainer(form)
    tr.captured_as(tr._program)
    tr._replay(1)
    want = _flat([("replay", i, 1 if per_slot else 0)] if kind == G else calls
                 for i, (calls, (kind, per_slot)) in enumerate(zip(EAGER[form], SHAPES[form])))
    assert tr.log == want
    # spin_up's walk: the same graphs, the sort, no collective
    del tr.log[:]
    tr._replay(0, local=True)
    assert tr.log == _flat([("replay", i, 0)] if kind == G else calls
                           for i, (calls, (kind, _)) in enumerate(zip(EAGER[form], SHAPES[form])) if kind != X)


@pytest.mark.parametrize("form", ["allreduce", "sharded"])
def test_one_graph_form_is_the_eager_walk_per_slot(form):
    tr = _Trainer(form)
    tr._walk(ONE_GRAPH, [None], 1)                     # what the capture of slot 1's graph enqueues
    assert tr.log == _flat(EAGER[form])
    del tr.log[:]
    tr.captured_as(ONE_GRAPH)
    tr._replay(1)
    tr._replay(0, local=True)                          # (the collectives are inside the graph: spin_up replays it whole)
    assert tr.log == [("replay", 0, 1), ("replay", 0, 0)]
