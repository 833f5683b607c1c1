"""The share of (MlpDWBN layer, sample) pairs that the layers' DropPath drops in the steps of a bench workload - what
ops.DROP_PATH_SKIP leaves out - counted from the very masks the kernels draw (ops.DropRecorder.mask replays a site's mask on the
GPU from the step's device seed):
    python tools/droppath_fraction.py <workload> [steps] [warmup]
Runs the workload eagerly like tools/ab_bench.py does (`warmup` untimed steps, then `steps` and one more); prints the fraction per step and over
the timed steps."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
import bench          # noqa: E402
from npvp_amd import ops, sched          # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "c2"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)

node_sites, per_step = [], []
real_node, real_begin = ops.mlpdwbn, sched.RngState.begin_step


def node(*a):
    n = len(ops.DropRecorder.sites)
    out = real_node(*a)
    node_sites.extend(s for s in ops.DropRecorder.sites[n:] if s[1] == "group")
    return out


def begin_step(self, d):
    # the masks of the step that just ended, while its seed is still the device seed
    if node_sites:
        dropped = sum(int((ops.DropRecorder.mask(s, d) == 0).sum()) for s in node_sites)
        per_step.append((dropped, sum(s[2] for s in node_sites)))
        node_sites.clear()
    ops.DropRecorder.sites = []
    real_begin(self, d)


ops.mlpdwbn = node
sched.RngState.begin_step = begin_step
ops.DropRecorder.sites = []
args = argparse.Namespace(flavour="predictor", graph=False, probe_all=False, graph_streams=1, dp_fused_trial="auto", trial_steps=10,
                          dp_graph="never", graph_packets="safe")
bench.run_workload(wl, steps + 1, warmup, args, 0, 1, dev, probe=False)      # (a step's masks are read when the next one begins)
timed = per_step[warmup:warmup + steps]
assert len(timed) == steps, (len(per_step), warmup, steps)
print(f"{wl}: (dropped, layer x sample pairs) per timed step: {timed}")
d, n = sum(t[0] for t in timed), sum(t[1] for t in timed)
print(f"{wl}: dropped fraction of the {steps} timed steps: {d}/{n} = {d / n:.4f}")
