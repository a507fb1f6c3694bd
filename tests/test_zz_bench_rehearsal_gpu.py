"""(Named to run last in the GPU suite: the longest and most box-sensitive tests.)

Rehearsal of the driver's multi-GPU bench (SCALE: N = 2, 4, 8 back to back) on one MI355X:
``bench.py --gpus N --full`` under ``torch.distributed.run`` with N ranks sharing the GPU (gloo
bootstrap; RCCL refuses two ranks on one device), the ``auto`` TP transport decision enabled on
gloo (``DPFS_TP_COMM_AUTO_ANY_BACKEND=1``: xGMI kernels -- two-shot and one-shot -- and, at
TP 2 with other pairs, the relayed exchange are built, validated and timed per size class), and
a reduced model (1 layer, seq 128) so it fits the test time limit.

It runs the same code as the driver's runs, per N:
  N = 2: the headline ``tp2`` (= pure TP);
  N = 4: ``tp2dp2`` (relay candidate), then the extra pure ``tp4`` layout;
  N = 8: ``tp2dp4`` (relay candidate), then the extra pure ``tp8`` layout (12 heads over 8
  ranks: 2 / 1 per rank);
each reported in ONE JSON line with its transport decisions, inside a wall-clock budget that
leaves the driver's 600 s lease room for the full-size model.
"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The driver's lease for a bench run is 600 s, most of it for the full-size model's warmup and
# timed steps; the reduced-model rehearsal of the protocol (bootstrap, transport decisions, both
# layouts, teardown) must take well under half of it.
# (N ranks time-share the one GPU here: the N = 4 rehearsal has taken 100-224 s from box to box)
BUDGET_S = 280


@pytest.mark.timeout(320)
@pytest.mark.parametrize("n,layouts", [(2, ["tp2"]), (4, ["tp2dp2", "tp4"]), (8, ["tp2dp4", "tp8"])])
def test_bench_n_ranks_on_one_gpu(n, layouts):
    from dist_helpers import _free_port
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", DPFS_BACKEND="gloo", DPFS_TP_COMM="auto",
               DPFS_TP_COMM_AUTO_ANY_BACKEND="1", DPFS_GEMM_BACKEND="ours", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py",
           "--gpus", str(n), "--layers", "1", "--seq-len", "128", "--batch-per-gpu", "2", "--steps", "2",
           "--warmup", "2", "--full", "--pure-tp-budget-s", "120"]
    # the ranks' output goes to a log file as it comes (gpurun_out/ on the GPU box: a run that
    # prints nothing for minutes is taken to be hung), read back afterwards
    logdir = os.path.join(ROOT, "gpurun_out") if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else None
    log = os.path.join(logdir or "/tmp", f"rehearsal_n{n}.log")
    t0 = time.time()
    with open(log, "w") as f:
        rc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=f, stderr=subprocess.STDOUT, text=True,
                            timeout=300).returncode
    wall = time.time() - t0
    out = open(log).read()
    assert rc == 0, out[-6000:]
    lines = [json.loads(l) for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-3000:]
    d = lines[0]
    if os.environ.get("DPFS_REHEARSAL_OUT"):     # keep the lines (profiles/ record of the rehearsal)
        with open(os.environ["DPFS_REHEARSAL_OUT"], "a") as f:
            f.write(json.dumps(dict(d, rehearsal_wall_s=round(wall, 1))) + "\n")
    assert wall < BUDGET_S, f"rehearsal took {wall:.0f} s (budget {BUDGET_S} s)"
    assert d["n_gpus"] == n and d["value"] > 0
    assert d["config"]["parallelism"].split("+")[0] == layouts[0]
    got = [L["parallelism"].split("+")[0] for L in d["layouts"]]
    if len(layouts) > 1 and (d["tp_pure"] or {}).get("error", "").startswith("timeout"):
        # The extra pure-TP layout ran past its wall-clock budget: with N ranks time-sharing one
        # GPU its step time varies by an order of magnitude from box to box.  That budget is the
        # bench's own guard for the driver's lease, and this is its designed outcome: the
        # headline line still printed, every rank exited 0, the extra layout reported as an error.
        assert got == layouts[:1], d["layouts"]
        print(f"[rehearsal] N={n}: extra layout {layouts[1]} timed out ({d['tp_pure']['error']}); headline kept")
    else:
        assert got == layouts, d["layouts"]
        assert "error" not in d["tp_pure"], d["tp_pure"]
        assert d["tp_pure"]["value"] > 0 and d["tp_pure"]["parallelism"].split("+")[0] == f"tp{n}"
    # every layout made (and reports) a transport decision per op and size class
    for L in d["layouts"]:
        tc = L["tp_comm"]
        assert tc is not None and "transport" in tc, L
        assert all(f"{op}:s=" in tc["transport"] for op in ("all_reduce", "reduce_scatter", "all_gather")), tc
        for c in ("s", "m", "l"):
            assert "xgmi_ms" in tc["all_reduce"][c], tc                   # the xGMI kernels were timed
        assert "xgmi1_ms" in tc["all_reduce"]["s"], tc                    # and the one-shot form
    if n >= 4:                                   # TP 2 with other pairs: the relay was a candidate
        assert "relay_ms" in d["layouts"][0]["tp_comm"]["all_reduce"]["s"]
