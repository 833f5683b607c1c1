"""The multi-process GPU jobs of `pytest -m gpu`, run one after the other by ONE child of the test session (started by
tests/conftest.py before the test process touches the GPU; this wrapper itself never does):
  0. tools/ae_dp_check.py     - data-parallel Stage-1 training (synchronised BatchNorm in the HIP path, GradSync): 2 gloo ranks on the
                                card against the reference's whole-batch steps, then 1 rank on real RCCL against the plain step.  The
                                shortest jobs, so they run first; each under its own 300 s limit
  1. tools/dp_check.py        - 2 ranks on one card (gloo on device tensors): the real data-parallel step == one process
  2. bench.py --gpus 2        - the N > 1 branch of the benchmark itself (rank-strided model build, GradSync, SyncBatchNorm,
                                MAX-over-ranks timing, the JSON line) on the BASELINE multi-GPU shard workload (c4: 8 clips)
  3. bench.py --gpus 1 on RCCL - one rank, backend nccl, NPVP_DP_FORCE=1: the data-parallel path on real RCCL (see below)
  4. the same with NPVP_DP_COMM=c - the gradient buckets through the library's own npvp_dp_* exchange
  5. tools/dp_check.py with 4 ranks on the card
  7. tools/graph_alloc_hazard.py - replayed steps with a caller allocating / copying batches between the replays, in both replay modes
                                of the runtime
  6. tools/dp_segments_check.py - the data-parallel step replayed as HIP-graph segments with the collectives issued eagerly between
                                them (trainer.StepTape) against the eager data-parallel step, bit for bit: on one RCCL rank and on two
                                gloo ranks sharing the card
Each job's output goes to <log>.<name>; the wrapper's exit code is the first failure's.  A job that ends by abort, segmentation
fault or time limit (rc 134, 139, 124, 137 or negative - its own, or a rank's as torch.distributed.run reports it - or a GPU memory
fault in its log) ends the chain: nothing further is started on that card and the wrapper exits with that code."""
import os, re, signal, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
log = sys.argv[1]
env = dict(os.environ, NPVP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
run = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1"]
run1 = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1"]
# 0. data-parallel Stage-1 training: 2 ranks over gloo on device tensors, then ONE rank with backend nccl and NPVP_DP_FORCE=1 (the
#    [sum x, sum x^2, n] / [sum g', sum g' xhat] all-reduces of doubles on real RCCL)
jobs = [("ae_dp2", run + ["--master-port", "29539", os.path.join(ROOT, "tools", "ae_dp_check.py")]),
        ("ae_dp1", run1 + ["--master-port", "29540", os.path.join(ROOT, "tools", "ae_dp_check.py")]),
        ("dp_check", run + ["--master-port", "29531", os.path.join(ROOT, "tools", "dp_check.py")]),
        ("bench2", run + ["--master-port", "29532", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--workload", "c4", "--steps", "3",
                          "--warmup", "1", "--dp-fused-trial", "always", "--dp-graph", "always", "--trial-steps", "2", "--no-cpu-baseline", "--full"])]
# 3. RCCL itself, as far as one GPU allows: ONE rank, backend nccl, NPVP_DP_FORCE=1 = the whole data-parallel code path on a group
#    of one (ProcessGroupNCCL init, model broadcast, SyncBatchNorm2d's all-reduces on their own communicator, GradSync's bucket
#    all_reduce(async_op=True) on the side stream + work.wait() + finish()) inside the benchmark's own step
jobs.append(("rccl1", run1 + ["--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c4", "--steps", "3",
                              "--warmup", "2", "--no-secondary", "--no-cpu-baseline", "--dp-graph", "always", "--trial-steps", "3", "--full"]))
# 4. the same one-rank RCCL step with the gradient buckets on the LIBRARY's exchange (NPVP_DP_COMM=c: npvp_dp_unique_id / npvp_dp_init /
#    npvp_dp_allreduce_async / npvp_dp_wait of include/npvp_hip.h) instead of ProcessGroupNCCL's all_reduce
#    (and with the mode trial's second leg forced - one launch per layer backward beside the gradient stream: GradSync must see the
#    same per-parameter contribution counts in both legs)
jobs.append(("rccl1c", run1 + ["--master-port", "29534", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c4", "--steps", "3",
                               "--warmup", "2", "--no-secondary", "--no-cpu-baseline", "--dp-fused-trial", "always", "--dp-graph", "never",
                               "--trial-steps", "3", "--full"]))
# 5. tools/dp_check.py once more with FOUR ranks on the card (gloo on device tensors; 8-sample global batch, 2 per rank)
run4 = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1"]
jobs.append(("dp_check4", run4 + ["--master-port", "29535", os.path.join(ROOT, "tools", "dp_check.py")]))
# 6. the segmented replay of the data-parallel step == the eager data-parallel step, bit for bit (parameters, Adam state, gradients, loss)
jobs.append(("seg1", run1 + ["--master-port", "29536", os.path.join(ROOT, "tools", "dp_segments_check.py")]))
jobs.append(("seg2", run + ["--master-port", "29537", os.path.join(ROOT, "tools", "dp_segments_check.py")]))
#    ... and once more on the RCCL rank with the runtime's prepared-packet replay switched on: the segments carry no memset node
#    (SyncBatchNorm's statistics are the library's column sums), so that mode is exact too and the host pays less per replay
jobs.append(("seg1f", run1 + ["--master-port", "29538", os.path.join(ROOT, "tools", "dp_segments_check.py")]))
# 7. replayed steps and what a caller does between replays (tools/graph_alloc_hazard.py): in the package's default runtime mode
#    (hazard0-2) and with the runtime's prepared-packet replay switched on (fast0-2: the step has no memset node, which that mode
#    does not execute reliably on ROCm 7.2 - npvp_amd/__init__.py) losses and parameters must stay on the eager trajectory, bit for bit
for i in range(3):
    jobs.append((f"hazard{i}", [sys.executable, os.path.join(ROOT, "tools", "graph_alloc_hazard.py")]))
for i in range(3):
    jobs.append((f"fast{i}", [sys.executable, os.path.join(ROOT, "tools", "graph_alloc_hazard.py")]))
fast = {k: v for k, v in env.items() if k != "DEBUG_CLR_GRAPH_PACKET_CAPTURE"}         # (inherited from a parent that imported npvp_amd)
envs = {"hazard0": dict(env, BETWEEN="tiny"), "hazard1": dict(env, BETWEEN="fill:0.001"), "hazard2": dict(env, BETWEEN="clone"),
        "fast0": dict(fast, NPVP_GRAPH_PACKET_CAPTURE="1", BETWEEN="inputs"), "fast1": dict(fast, NPVP_GRAPH_PACKET_CAPTURE="1", BETWEEN="tiny"),
        "fast2": dict(fast, NPVP_GRAPH_PACKET_CAPTURE="1", BETWEEN="inputs", STOCHASTIC="1"),     # (NPVP-S: one memcpy node, same noise in both runs)
        "seg1": dict(env, NPVP_DIST_BACKEND="nccl", NPVP_DP_FORCE="1"),
        "seg1f": dict(fast, NPVP_DIST_BACKEND="nccl", NPVP_DP_FORCE="1", NPVP_GRAPH_PACKET_CAPTURE="1"),
        "seg2": dict(env, SEG_CHECK_STEPS="4", SEG_CHECK_LAYERS="4"),
        "dp_check4": dict(env, DP_CHECK_SEED="12"),      # (clip seed 11 puts ONE unit of the 8-clip batch on a ReLU kink, counted: profiles/r06_dp_check_relu_kink.txt)
        "ae_dp1": dict(env, NPVP_DIST_BACKEND="nccl", NPVP_DP_FORCE="1"),
        "rccl1": dict(env, NPVP_DIST_BACKEND="nccl", NPVP_DP_FORCE="1"),
        "rccl1c": dict(env, NPVP_DIST_BACKEND="nccl", NPVP_DP_FORCE="1", NPVP_DP_COMM="c")}
limits = {"ae_dp2": 300, "ae_dp1": 300}          # seconds; a job over its limit is ended (its whole process group) with rc 124
FATAL = (134, 139, 124, 137)


def run_job(name, cmd, out):
    limit = limits.get(name)
    p = subprocess.Popen(cmd, stdout=out, stderr=subprocess.STDOUT, env=envs.get(name, env), cwd=ROOT, start_new_session=limit is not None)
    try:
        return p.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGTERM)              # (the launcher and its ranks: the session this job was started in)
        try:
            p.wait(timeout=10)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
        return 124


def fatal_code(rc, text):
    """the code to stop the chain with, or None: the job's own exit status, or what the launcher's failure report says of a rank"""
    codes = [rc] + [int(c) for c in re.findall(r"exitcode\s*:\s*(-?\d+)", text)]
    for c in codes:
        if c < 0 or c in FATAL:
            return c if c > 0 else 128 - c
    if rc != 0 and "illegal memory access" in text:
        return rc
    return None


import time
rc = 0
with open(f"{log}.times", "w") as tf:
    for name, cmd in jobs:
        t0 = time.time()
        with open(f"{log}.{name}", "w") as f:
            r = run_job(name, cmd, f)
        tf.write(f"{name} {time.time() - t0:.1f} s rc={r}\n"); tf.flush()
        if r != 0 and rc == 0:
            rc = r
        stop = fatal_code(r, open(f"{log}.{name}", errors="replace").read()) if r != 0 else None
        if stop is not None:
            tf.write(f"stopped after {name}: nothing further is started on a card whose last job ended with {stop}\n"); tf.flush()
            sys.exit(stop)
sys.exit(rc)
