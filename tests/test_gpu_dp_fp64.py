"""-m gpu: the data-parallel train step's gradient against the fp64 oracle of the WHOLE batch, relative to each row's own size.

Two and three ranks (fresh child processes started by torch.distributed.run, gloo, sharing the one GPU, as tests/test_gpu_dp.py
starts them) each make ONE FusedTrainer step on their B / N sequences of a case's batch; the optimizer state then holds
exp_avg = (1 - beta1) g and exp_avg_sq = (1 - beta2) g^2 of the exchanged gradient.  tests/dp_refs.py: the jobs, the skewed
batches, and why ``grad_refs.fp64_grads`` of the whole batch with ``b0 = 0`` is the reference (tests/test_dp_refs.py shows it, and
shows the wrong exchanges - a mean of local means, rank 0's masks on every rank, the statistics summed twice, a rank dropped,
a shard's first element lost - at least ten times over the bound; tools/dp_parity.py's stepped-weight tolerance, the older check
of this path, accepts a gradient of the wrong scale).  tests/dp_fp64_worker.py is the rank program: one launch per world size
runs all of that world's jobs in order and is shared by all of that world's tests; the oracle runs here, in the parent.

Per job: the inputs admissible (grad_refs.assert_admissible), every tensor's row_errors <= grad_refs.bound(e32) on this run's own
e32 (no new tolerance), rows whose fp64 gradient is exactly zero exactly zero, the K slice of in_proj_bias under its own rule,
exp_avg_sq / (1 - beta2) against g64^2 under twice the bound, the step's loss against the fp64 loss of the whole batch
(fwd_refs.assert_loss_holds: it pins the GLOBAL count), every replica's stepped parameters the same bits, the planned kernel
names the case's.  The deterministic sharded job of the skewed batch runs twice: equal bits.

A launch is started once per session and its outcome cached, failure included: after a crash or a timeout no further test
starts it again.  Measured on the MI355X machine: run on its own (three sessions) the 2-rank launch (43 steps) took 5.5, 5.8
and 6.3 s of wall time and the 3-rank launch 6.2, 7.3 and 8.7 s - about 5 s of it start-up (interpreters, rendezvous), 1.1 ..
3.9 s the jobs; inside the whole -m gpu suite the 3-rank launch took 11.4 s.  LAUNCH_SECONDS holds the largest; the timeout is
four times that (25 s and 46 s), and never more than the 600 s tests/test_gpu_dp.py allows a launch.  The whole module runs
in 15 s.
profiles/dp_fp64_errors.json holds the measured figures (SRFRD_DP_FP64_REPORT=<path> makes this module write them): the worst
tensor of the 84 jobs is at 0.13 of its bound (v1, three ranks), the worst second moment at 0.035 of twice the bound, the loss
within 5.6e-8, no leak into a zero row.
"""
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

import pytest
import torch

from tests import dp_refs as D
from tests import fwd_refs as R
from tests import grad_refs as G
from tests.test_gpu_dp import ROOT, _free_port

pytestmark = pytest.mark.gpu

LAUNCH_SECONDS = {2: 6.3, 3: 11.4}             # wall time of one launch, measured on the MI355X machine (the largest seen)
TIMEOUT = {w: min(4.0 * s, 600.0) for w, s in LAUNCH_SECONDS.items()}
_LAUNCHES = {}                                  # world -> {"results": ..., "status": ..., "seconds": ...} | {"error": text}
_FIGURES = {}                                   # job id -> what profiles/dp_fp64_errors.json records


def _launch(world):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, f"dp_fp64_w{world}.pt")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dp_fp64_worker.py"), out]
        t0 = time.time()
        p = subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             start_new_session=True)
        try:
            stdout, stderr = p.communicate(timeout=TIMEOUT[world])
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)            # the launcher and every rank: nothing stays on the GPU
            stdout, stderr = p.communicate()
            return {"error": f"{world}-rank launch killed after {TIMEOUT[world]:.0f} s:\n{stdout[-2000:]}\n{stderr[-4000:]}"}
        seconds = time.time() - t0
        lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines or not json.loads(lines[-1])["ok"] or not os.path.exists(out):
            return {"error": f"{world}-rank launch failed (rc {p.returncode}):\n{stdout[-2000:]}\n{stderr[-6000:]}"}
        print(f"{world}-rank launch: {seconds:.1f} s ({lines[-1]})")
        return {"results": torch.load(out, weights_only=False), "status": json.loads(lines[-1]), "seconds": seconds}


def _run(world):
    """the outcome of the one launch of this world size, started at the first call of the session"""
    if world not in _LAUNCHES:
        _LAUNCHES[world] = {"error": f"the {world}-rank launch did not return"}      # (whatever interrupts it: never again)
        _LAUNCHES[world] = _launch(world)
    got = _LAUNCHES[world]
    assert "error" not in got, got["error"]
    return got


def _worst(figs):
    k = max(figs, key=lambda k: figs[k]["err"] / figs[k]["bound"])
    return k, figs[k]["err"] / figs[k]["bound"]


@pytest.mark.parametrize("job", D.JOBS, ids=[D.job_id(j) for j in D.JOBS])
def test_data_parallel_step_gradients_meet_the_fp64_oracle(job):
    cid, world, exchange, det, graph, l2 = job
    what = f"job {D.job_id(job)}"
    ref = D.reference(cid, l2)
    G.assert_admissible(ref, what)                              # (e32 is this machine's: the bounds below come from it)
    assert ref.clamp == D.over_cap(cid)
    got = _run(world)["results"][D.job_id(job)]
    figs, figs2 = G.compare(got["g"], ref), G.compare(got["g2"], ref, squares=True)
    _FIGURES[D.job_id(job)] = {"worst": _worst(figs), "second_moment_worst": _worst(figs2),
                               "old": max(f["old"] for f in figs.values()),
                               "zero_leaks": sum(f["zero_leaks"] for f in figs.values()), "e32": max(ref.e32.values())}
    G.assert_holds(figs, what)
    G.assert_holds(figs2, what + " second moment")
    err = R.assert_loss_holds(torch.tensor(got["loss"]), D.step_reference(cid), what, l2)
    _FIGURES[D.job_id(job)]["loss_error"] = err
    assert got["replicas_equal"], what
    assert tuple(got["names"]) == D.local_names(cid, world), (what, got["names"])


@pytest.mark.parametrize("world", D.WORLDS, ids=[f"w{w}" for w in D.WORLDS])
def test_deterministic_exchange_repeats_its_bits(world):
    rep = _run(world)["results"]["repeat"]
    assert rep["job"] == D.job_id((D.REPEATED[0], world) + D.REPEATED[1:]) and rep["equal_bits"], rep


def test_two_launches_and_their_figures():
    """after the tests above: one launch per world size ran, inside its time; the figures go where the report is asked for"""
    for world in D.WORLDS:
        got = _run(world)
        assert got["status"]["world"] == world and got["status"]["jobs"] == len(D.jobs_of(world)) + 1
        assert got["seconds"] <= TIMEOUT[world]
    assert sorted(_LAUNCHES) == list(D.WORLDS)
    path = os.environ.get("SRFRD_DP_FP64_REPORT")
    if path and len(_FIGURES) == len(D.JOBS):
        num = lambda x: float(f"{x:.2g}")
        jobs = {}
        for jid, f in _FIGURES.items():
            jobs[jid] = {"e32_worst": num(f["e32"]), "worst": [f["worst"][0], num(f["worst"][1])],
                         "second_moment_worst": [f["second_moment_worst"][0], num(f["second_moment_worst"][1])],
                         "old": num(f["old"]), "zero_leaks": f["zero_leaks"], "loss_error": num(f["loss_error"])}
        report = {"metric": "tests/grad_refs.py: row_errors against the fp64 gradient of the WHOLE batch, bound(e32) = max(64 e32, "
                            "2e-5), clamped at 1e-4 for the OVER_CAP jobs; per job of tests/dp_refs.py (case-world-exchange-scatter"
                            "[-graph][-l2]): worst = [tensor, row error / bound], second_moment_worst the same for g^2 under twice "
                            "the bound, old = max|g - g_oracle32|, loss_error = |loss - loss64| / loss64, e32_worst the fp32 "
                            "oracle's worst row error on the machine that ran the tests",
                  "launch_seconds": {str(w): round(_LAUNCHES[w]["seconds"], 1) for w in D.WORLDS}, "jobs": jobs}
        with open(path, "w") as f:
            f.write("{\n \"metric\": " + json.dumps(report["metric"]) + ",\n \"launch_seconds\": "
                    + json.dumps(report["launch_seconds"]) + ",\n \"jobs\": {\n"
                    + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in jobs.items()) + "\n }\n}\n")
