"""Where a train step's key sort runs (srfrd_amd.trainer: sort_key_count, SORT_CAPTURE_LIMIT, sort_plan, step_program's
``eager_sort`` form, FusedTrainer._sort_keys) - host logic and walks on recording stubs: no device, no FusedTrainer instance."""
import itertools

import pytest
import torch

from srfrd_amd import trainer
from srfrd_amd.trainer import SORT_CAPTURE_LIMIT, FusedTrainer, sort_key_count, sort_plan, step_program

G, E, X = "graph", "eager", "collective"
B, L, K = 7, 50, 16
T = B * L


# ---- the key count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,det,lazy,want", [
    ("bce", False, False, 0), ("bce", True, False, 3 * T), ("bce", False, True, 3 * T), ("bce", True, True, 3 * T),
    ("softmax", False, False, 0), ("softmax", True, False, T),
    ("sampled_softmax", False, False, 2 * T + K), ("sampled_softmax", True, False, 2 * T + K),
    ("token_softmax", False, False, T * (2 + K)), ("token_softmax", True, False, T * (2 + K)),
    ("gbce", False, False, T * (2 + K)), ("gbce", True, False, T * (2 + K)),
])
def test_key_count(loss, det, lazy, want):
    assert sort_key_count(loss, det, lazy, B, L, K) == want


def test_key_count_of_the_issue_shapes():
    assert sort_key_count("bce", True, False, 7000, 50) == 1_050_000
    assert sort_key_count("bce", False, True, 7000, 50) == 1_050_000
    assert sort_key_count("sampled_softmax", False, False, 10_500, 50, 64) == 1_050_064
    assert sort_key_count("bce", True, False, 1748, 200) > SORT_CAPTURE_LIMIT >= sort_key_count("bce", True, False, 1747, 200)
    assert sort_key_count("bce", True, False, 4, 20) == 240 and sort_key_count("bce", False, False, 7000, 50) == 0


# ---- the decision ------------------------------------------------------------------------------------------------------------------
def test_the_limit_is_rocprims_merge_sort_limit():
    assert SORT_CAPTURE_LIMIT == 1024 * 1024


@pytest.mark.parametrize("use_graph", [True, False])
def test_single_rank_boundary(use_graph):
    """2^20 keys take rocprim's merge sort (size <= merge_sort_limit) and are captured; one more is sorted eagerly"""
    for n in (0, 1, 240, SORT_CAPTURE_LIMIT):
        assert sort_plan("single", n, use_graph) == (False, use_graph, None)
    for n in (SORT_CAPTURE_LIMIT + 1, 1_050_000, 1_689_600):
        assert sort_plan("single", n, use_graph) == (True, use_graph, None)


@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_data_parallel_over_the_limit_steps_without_graphs_and_says_why(mode):
    assert sort_plan(mode, SORT_CAPTURE_LIMIT, True) == (False, True, None)
    assert sort_plan(mode, 0, True) == (False, True, None)
    eager_sort, use_graph, reason = sort_plan(mode, SORT_CAPTURE_LIMIT + 1, True)
    assert (eager_sort, use_graph) == (False, False)          # no split exchange program, no graph - so never ONE_GRAPH
    assert str(SORT_CAPTURE_LIMIT + 1) in reason and mode in reason and "without graphs" in reason
    assert sort_plan(mode, SORT_CAPTURE_LIMIT + 1, False) == (False, False, None)      # (nobody asked for graphs: nothing to explain)


def test_the_decision_reads_the_limit_when_asked(monkeypatch):
    monkeypatch.setattr(trainer, "SORT_CAPTURE_LIMIT", 0)
    assert sort_plan("single", 240) == (True, True, None)
    assert sort_plan("single", 0) == (False, True, None)           # an unsorted trainer stays one graph
    assert sort_plan("sharded", 240)[:2] == (False, False)


# ---- step_program ------------------------------------------------------------------------------------------------------------------
# what step_program answered before it took ``eager_sort``, for every (mode, token, lazy) it accepts
PARENT = {
    ("single", False, False): [(G, True, ("_enqueue_compute_update",))],
    ("single", True, False): [(G, True, ("_enqueue_ce_compute",)), (E, False, ("_sort_keys",)),
                              (G, False, ("_enqueue_table_reduce", "_enqueue_ce_dense", "_enqueue_update"))],
    ("single", False, True): [(G, True, ("_enqueue_lazy_step",))],
    ("allreduce", False, False): [(G, True, ("_enqueue_compute",)), (X, False, ("_all_reduce_grad",)), (G, False, ("_enqueue_update",))],
    ("sharded", False, False): [(G, True, ("_enqueue_fwd",)), (X, False, ("_start_stats_reduce",)), (G, True, ("_enqueue_bwd",)),
                                (X, False, ("_scatter_grad",)), (G, False, ("_enqueue_shard_update",)),
                                (X, False, ("_gather_params",)), (G, False, ("_enqueue_shard_finish",))],
}
PARENT["allreduce", True, False] = PARENT["allreduce", False, False]
PARENT["sharded", True, False] = PARENT["sharded", False, False]


@pytest.mark.parametrize("mode,token,lazy", list(itertools.product(("single", "allreduce", "sharded"), (False, True), (False, True))))
def test_defaults_are_the_parents_lists(mode, token, lazy):
    if (mode, token, lazy) not in PARENT:
        with pytest.raises(ValueError, match="lazy_table"):
            step_program(mode, token, lazy)
        with pytest.raises(ValueError, match="lazy_table"):
            step_program(mode, token, lazy, eager_sort=True)
        return
    assert step_program(mode, token, lazy) == step_program(mode, token, lazy, False) == PARENT[mode, token, lazy]
    assert step_program(mode, token, lazy, eager_sort=False) == PARENT[mode, token, lazy]


@pytest.mark.parametrize("lazy", [False, True])
def test_eager_sort_form_has_the_token_programs_shape(lazy):
    program = step_program("single", lazy=lazy, eager_sort=True)
    assert [(kind, per_slot) for kind, per_slot, _ in program] == [(G, True), (E, False), (G, False)]
    assert [(kind, per_slot) for kind, per_slot, _ in program] == [(k, p) for k, p, _ in step_program("single", True)]
    assert program[1][2] == ("_sort_keys",)
    assert program[2][2][-1] == ("_enqueue_lazy_update" if lazy else "_enqueue_update")
    for _, _, calls in program:
        assert calls and all(callable(getattr(FusedTrainer, name)) for name in calls), calls


def test_eager_sort_leaves_the_token_program_and_refuses_the_exchange_modes():
    assert step_program("single", True, eager_sort=True) == PARENT["single", True, False]      # (eager at every size already)
    for mode in ("allreduce", "sharded"):
        with pytest.raises(ValueError, match="eager sort"):
            step_program(mode, eager_sort=True)


# ---- the walks, on recording stubs -------------------------------------------------------------------------------------------------
class _Graph:
    def __init__(self, log, stage, slot):
        self.log, self.tag = log, ("replay", stage, slot)

    def replay(self):
        self.log.append(self.tag)


class _Trainer:
    """FusedTrainer's walks and the methods that put a step's three pieces together, over recorders in place of the pieces"""
    _walk, _enqueue_step, _replay = FusedTrainer._walk, FusedTrainer._enqueue_step, FusedTrainer._replay
    _enqueue_compute_update, _enqueue_lazy_step = FusedTrainer._enqueue_compute_update, FusedTrainer._enqueue_lazy_step
    _enqueue_step_compute = FusedTrainer._enqueue_step_compute
    slots, keys = 2, "keys"                        # (a sorted trainer: `keys` is not None)
    PIECES = ("_enqueue_to_keys", "_sort_keys", "_enqueue_reduce", "_enqueue_update", "_enqueue_lazy_update")

    def __init__(self, lazy, eager_sort):
        self.log = []
        self._program = step_program("single", lazy=lazy, eager_sort=eager_sort)

    def __getattr__(self, name):
        if name not in self.PIECES:
            raise AttributeError(name)
        return lambda *args: self.log.append((name,) + args)

    def captured_as(self, stages):
        self._graphs = (stages, [[_Graph(self.log, i, k) for k in range(self.slots if per_slot else 1)] if kind == G else None
                                 for i, (kind, per_slot, _) in enumerate(stages)])


def _pieces(lazy):
    return [("_enqueue_to_keys", 1), ("_sort_keys",), ("_enqueue_reduce",), ("_enqueue_lazy_update" if lazy else "_enqueue_update",)]


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_eager_and_local_walks_call_what_the_one_stage_form_calls(lazy, local):
    one, split = _Trainer(lazy, False), _Trainer(lazy, True)
    one._enqueue_step(1, local=local)
    split._enqueue_step(1, local=local)
    assert split.log == one.log == _pieces(lazy)              # (the local walk keeps the sort: it is no collective)


@pytest.mark.parametrize("lazy", [False, True])
def test_an_unsorted_step_calls_no_sort(lazy):
    tr = _Trainer(lazy, False)
    tr.keys = None
    tr._enqueue_step(1)
    assert tr.log == [c for c in _pieces(lazy) if c != ("_sort_keys",)]


@pytest.mark.parametrize("lazy", [False, True])
def test_replay_walk_sorts_between_the_two_graphs(lazy):
    tr = _Trainer(lazy, True)
    tr.captured_as(tr._program)
    tr._replay(1)
    assert tr.log == [("replay", 0, 1), ("_sort_keys",), ("replay", 2, 0)]
    del tr.log[:]
    tr._replay(0, local=True)                                  # spin_up's walk: the same graphs, and the sort
    assert tr.log == [("replay", 0, 0), ("_sort_keys",), ("replay", 2, 0)]
    # what the capture of each stage enqueues: the one-stage form's calls, cut at the sort
    del tr.log[:]
    for stage in tr._program:
        tr._walk([stage], [None], 1)
    assert tr.log == _pieces(lazy)


def test_the_gradient_tail_is_the_three_pieces_back_to_back():
    """`_enqueue_bwd`'s tail (the data-parallel programs, the two-launch step): key list, sort, what follows"""
    class T:
        _enqueue_grad_tail = FusedTrainer._enqueue_grad_tail
        keys = "keys"

        def __init__(self):
            self.log = []

        def __getattr__(self, name):
            if name not in ("_write_keys", "_sort_keys", "_enqueue_reduce"):
                raise AttributeError(name)
            return lambda *a: self.log.append((name,) + a)

    t = T()
    t._enqueue_grad_tail(1)
    assert t.log == [("_write_keys", 1), ("_sort_keys",), ("_enqueue_reduce",)]
    t.keys, t.log = None, []
    t._enqueue_grad_tail(1)
    assert t.log == [("_write_keys", 1), ("_enqueue_reduce",)]


# ---- _sort_keys --------------------------------------------------------------------------------------------------------------------
class _Sorter:
    _sort_keys = FusedTrainer._sort_keys

    def __init__(self, keys):
        self.keys = torch.tensor(keys, dtype=torch.int64)
        self.skeys, self.order = torch.full_like(self.keys, -1), torch.full_like(self.keys, -1)


def test_sort_keys_is_a_stable_sort_into_the_persistent_buffers(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)       # under the limit nobody asks
    s = _Sorter([3, 1, 3, 0, 1, 3])
    skeys, order = s.skeys, s.order
    s._sort_keys()
    assert s.skeys is skeys and s.order is order
    assert skeys.tolist() == [0, 1, 1, 3, 3, 3] and order.tolist() == [3, 1, 4, 0, 2, 5]


def test_sort_keys_refuses_a_long_list_under_capture_and_sorts_nothing(monkeypatch):
    monkeypatch.setattr(trainer, "SORT_CAPTURE_LIMIT", 4)
    asked = []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: asked.append(1) or True)
    s = _Sorter([3, 1, 3, 0, 1])                     # 5 keys: over the limit
    with pytest.raises(RuntimeError, match="5 keys.*must not be captured"):
        s._sort_keys()
    assert asked and s.skeys.tolist() == [-1] * 5 and s.order.tolist() == [-1] * 5
    # exactly the limit: captured (no question asked); over it outside a capture: sorted
    del asked[:]
    s4 = _Sorter([2, 0, 2, 1])
    s4._sort_keys()
    assert not asked and s4.skeys.tolist() == [0, 1, 2, 2] and s4.order.tolist() == [1, 3, 0, 2]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    s._sort_keys()
    assert s.skeys.tolist() == [0, 1, 1, 3, 3] and s.order.tolist() == [3, 1, 4, 0, 2]


def test_trainer_py_holds_one_sort():
    import inspect
    src = inspect.getsource(trainer)
    assert src.count("torch.sort(") == 1 and ".sort(" not in src.replace("torch.sort(", "")
    assert "torch.sort(self.keys, stable=True, out=(self.skeys, self.order))" in inspect.getsource(FusedTrainer._sort_keys)
