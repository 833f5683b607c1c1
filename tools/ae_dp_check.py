"""GPU rehearsal of data-parallel Stage-1 training (what ref/train_AutoEncoder_lightning.py:40-42 gets from devices=world_size, the
DDP strategy and sync_batchnorm=True): ae_data_parallel + ae_train_step(grad_sync=...) with synchronised BatchNorm in the HIP path.

Two or more ranks (gloo on device tensors, the ranks share the card):
    NPVP_DIST_BACKEND=gloo python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 tools/ae_dp_check.py
  - two data-parallel steps of the "64" case of tests/ae_train_cases.py (KTH pair, 2 clips x 4 frames of 64x64, one clip per rank)
    against the reference LitAE's own two WHOLE-BATCH steps (tests/golden/ae_train_64.npz) - whole-batch BatchNorm is what SyncBN over
    the shards must reproduce: rank-mean loss, per-parameter gradient norms and gradient heads of step 1, running statistics after
    step 1, parameter heads after both steps, at the bounds of tests/test_hip_ae_train.py::test_ae_train_step_vs_reference_fixture;
  - after the steps the flat parameters, both Adam moments and every running statistic are torch.equal on all ranks;
  - GradSync's overlapped path ran, and a step issues one statistics all-reduce per training-mode BatchNorm layer and direction;
  - uneven shards through autograd: rank r holds 2 + r frames of a seeded (5, 64, 6, 6) tensor, ops.bn_act_train(..., group)
    forward and backward in both layouts against float64.
One rank (NPVP_DIST_BACKEND=nccl NPVP_DP_FORCE=1: the double all-reduces on real RCCL):
  - ops.bn_act_train with the group == without it, bit for bit, forward and backward;
  - three steps of a converted pair with GradSync against three plain steps from the same state.  The yardstick is the plain
    path itself: it is run twice; if those runs are bit-equal the data-parallel run must be bit-equal to them too, otherwise (MIOpen
    convolutions that do not repeat) both distances are printed and the data-parallel one may be at most twice the plain one.
Rank 0 ends with "[ae_dp_check] OK"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import torch.distributed as dist
import torch.nn.functional as F
import npvp_amd
from npvp_amd import dp, ops
from oracle import ops as O
import ae_train_cases as AC
import golden_cases as GC

# the bounds of tests/test_hip_ae_train.py (KERNEL_TOL :13, the step bounds and the zero-gradient parameters :199-204)
KERNEL_TOL = 1e-5
GRAD_TOL, LOSS_TOL, NORM_TOL = 5e-3, 1e-4, 0.15
ZERO_GRAD = ("spatial_conv.0.bias", "attn2d.Wk.bias", "attn2d.Wv.bias", "attn2d.out_proj.bias")
TAG = "64"

rank, world, local = dp.init_distributed()
assert dp.active(), "ae_dp_check: start it under torch.distributed.run (one rank: NPVP_DP_FORCE=1)"
dev = torch.device("cuda", local % torch.cuda.device_count())
torch.cuda.set_device(dev)
say = lambda *a: print("[ae_dp_check]", *a, flush=True) if rank == 0 else None
say(f"world={world} backend={dist.get_backend()}")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def all_ranks(ok, what):
    """every rank's verdict, so that rank 0 cannot print OK beside a rank that failed"""
    t = torch.tensor([1.0 if ok else 0.0], device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    assert float(t) == 1.0, f"{what}: failed on at least one rank (this rank: {'ok' if ok else 'FAILED'})"


def build_pair():
    ci, AE = AC.CASES[TAG][:2]
    torch.manual_seed(0)
    enc, dec = npvp_amd.build_autoencoder(AE, ci)
    AC.fill(npvp_amd.AEPair(enc, dec))
    enc, dec = enc.to(dev).to(memory_format=torch.channels_last), dec.to(dev)
    npvp_amd.prepare_trainable_autoencoder(enc, dec)
    return enc, dec, npvp_amd.ae_optimizer(enc, dec, lr=AC.LR)


def running_stats(pair):
    sd = pair.state_dict()
    return [sd[k] for k in sd if k.endswith(("running_mean", "running_var"))]


COLLECTIVES = [0]
_collective0 = dp._collective


def _counted(fn):
    COLLECTIVES[0] += 1
    _collective0(fn)


dp._collective = _counted


# ------------------------------------------------------------------------------------------------------------ several ranks
def fixture_steps():
    gold = GC.load(f"ae_train_{TAG}")
    B = AC.CASES[TAG][2]
    assert B % world == 0, f"the fixture's batch of {B} clips does not split over {world} ranks"
    enc, dec, opt = build_pair()
    gs = npvp_amd.ae_data_parallel(enc, dec, opt, bucket_bytes=8 << 20)
    pair = opt.ae_pair
    assert list(AC.param_names(pair)) == list(gold["param_names"]) and list(AC.state_keys(pair)) == list(gold["state_keys"])
    n_bn = sum(isinstance(m, dp.SyncBatchNorm2d) and m.training for m in pair.modules())
    assert n_bn > 0 and not any(type(m) is torch.nn.BatchNorm2d for m in pair.modules())
    per_step = []

    def step(past, fut):
        c0 = COLLECTIVES[0]
        loss = npvp_amd.ae_train_step(enc, dec, opt, dp.shard_batch(past, rank, world), dp.shard_batch(fut, rank, world), grad_sync=gs)
        per_step.append(COLLECTIVES[0] - c0)
        loss = loss.clone()
        dist.all_reduce(loss)
        return loss / world                      # the rank-mean loss: equal shards, so the whole batch's

    res = AC.record(pair, step, TAG, dev)
    torch.cuda.synchronize()
    say(f"buckets={len(gs.buckets)} launched={gs.launched}; BatchNorm layers in training mode {n_bn}, statistics all-reduces per step "
        f"{per_step} (forward + backward)")
    assert per_step == [2 * n_bn] * 2, (per_step, n_bn)
    assert gs.launched > len(gs.buckets), "the overlapped path (buckets reduced during backward) never ran"
    for k in ("loss_0", "loss_1"):
        say(f"{k}: data parallel {float(res[k]):.8f}  reference {float(gold[k]):.8f}")
        assert abs(float(res[k]) - float(gold[k])) <= LOSS_TOL * abs(float(gold[k])), (k, float(res[k]), float(gold[k]))
    keep = [i for i, n in enumerate(gold["param_names"]) if not str(n).endswith(ZERO_GRAD)]
    worst = 0.0
    for i, n in enumerate(gold["param_names"]):
        nh, ng = float(res["grad_norm"][i]), float(gold["grad_norm"][i])
        if i in keep:
            worst = max(worst, abs(nh - ng) / ng)
            assert abs(nh - ng) <= NORM_TOL * ng, (str(n), nh, ng)
        else:
            assert nh < 1e-6 and ng < 1e-6, (str(n), nh, ng)
    e_g = rel(res["grad_head"][keep], gold["grad_head"][keep])
    e_r = rel(res["running"], gold["running"])
    e_p = [max(rel(res[k][i], gold[k][i]) for i in keep) for k in ("param_head_0", "param_head_1")]
    say(f"vs the reference fixture: gradient norms worst {worst:.3e} (bound {NORM_TOL}), gradient heads rel-L2 {e_g:.3e} (bound {GRAD_TOL}), "
        f"running statistics {e_r:.3e} (bound 1e-3), parameter heads worst {e_p[0]:.3e} / {e_p[1]:.3e} (bound {GRAD_TOL})")
    assert e_g < GRAD_TOL and e_r < 1e-3 and max(e_p) < GRAD_TOL
    # every rank holds the same model and optimiser state
    same = True
    for t in [opt.flat_p, opt.m, opt.v] + running_stats(pair):
        r0 = t.detach().clone()
        dist.broadcast(r0, 0)
        same = same and torch.equal(r0, t)
    all_ranks(same, "parameters / Adam moments / running statistics equal on all ranks")
    say("parameters, Adam moments and running statistics are torch.equal on all ranks")
    gs.remove()


def uneven_shards():
    N, C, H, W = 5, 64, 6, 6
    assert world == 2, "the uneven-shard case is written for 2 ranks (2 + 3 frames)"
    lo, hi = (0, 2) if rank == 0 else (2, 5)
    x = O.seeded_randn((N, C, H, W), 1) * 1.7 + 0.6
    w, b = 1 + 0.1 * O.seeded_randn((C,), 2), 0.1 * O.seeded_randn((C,), 3)
    res, g = O.seeded_randn((N, C, H, W), 4), O.seeded_randn((N, C, H, W), 5)
    rm, rv = 0.1 * O.seeded_randn((C,), 6), 0.5 + O.seeded_randn((C,), 7).abs()
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    rmd, rvd = rm.double(), rv.double()
    yd = torch.relu(F.batch_norm(xd, rmd, rvd, wd, bd, True, 0.1, 1e-5)) + res.double()
    yd.backward(g.double())
    for mf, name in ((torch.channels_last, "channels_last"), (torch.contiguous_format, "NCHW")):
        xg = x[lo:hi].to(dev).contiguous(memory_format=mf).requires_grad_()
        wg, bg = w.to(dev).requires_grad_(), b.to(dev).requires_grad_()
        rmg, rvg = rm.to(dev), rv.to(dev)
        yg = ops.bn_act_train(xg, wg, bg, rmg, rvg, 0.1, 1e-5, 1, True, res[lo:hi].to(dev).contiguous(memory_format=mf),
                              group=dp.syncbn_group())
        yg.backward(g[lo:hi].to(dev).contiguous(memory_format=mf))
        full = lambda t: torch.zeros(N, C, H, W, device=dev).index_copy_(0, torch.arange(lo, hi, device=dev), t.detach().contiguous())
        y_all, dx_all = full(yg), full(xg.grad)
        dw_all, db_all = wg.grad.clone(), bg.grad.clone()
        for t in (y_all, dx_all, dw_all, db_all):          # (each rank fills its own frames of a zero tensor: the sum is the gather)
            dist.all_reduce(t)
        errs = {"y": rel(y_all, yd), "dx": rel(dx_all, xd.grad), "dw": rel(dw_all, wd.grad), "db": rel(db_all, bd.grad),
                "running_mean": rel(rmg, rmd), "running_var": rel(rvg, rvd)}
        say(f"uneven shards (2 + 3 frames of (5, 64, 6, 6)), {name}, vs float64: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
        all_ranks(all(e < KERNEL_TOL for e in errs.values()), f"uneven shards {name}")


# ------------------------------------------------------------------------------------------------- one rank on its own group
def op_equals_plain():
    for mf, name in ((torch.channels_last, "channels_last"), (torch.contiguous_format, "NCHW")):
        shape = (3, 64, 6, 6)
        x = (O.seeded_randn(shape, 1) * 1.7 + 0.6).to(dev).contiguous(memory_format=mf)
        res, g = (O.seeded_randn(shape, s).to(dev).contiguous(memory_format=mf) for s in (4, 5))
        outs = []
        for group in (None, dp.syncbn_group()):
            xg = x.clone(memory_format=torch.preserve_format).requires_grad_()
            wg, bg = (1 + 0.1 * O.seeded_randn((64,), 2)).to(dev).requires_grad_(), (0.1 * O.seeded_randn((64,), 3)).to(dev).requires_grad_()
            rm, rv = (0.1 * O.seeded_randn((64,), 6)).to(dev), (0.5 + O.seeded_randn((64,), 7).abs()).to(dev)
            y = ops.bn_act_train(xg, wg, bg, rm, rv, 0.1, 1e-5, 1, True, res, group=group)
            y.backward(g)
            outs.append((y.detach(), xg.grad, wg.grad, bg.grad, rm, rv))
        eq = [torch.equal(a, b) for a, b in zip(*outs)]
        say(f"ops.bn_act_train with the group == without, {name}: y, dx, dw, db, running_mean, running_var bit-equal {eq}")
        assert all(eq)


def three_steps(parallel):
    enc, dec, opt = build_pair()
    gs = npvp_amd.ae_data_parallel(enc, dec, opt, bucket_bytes=8 << 20) if parallel else None
    losses = []
    for step in range(3):
        past, fut = (t.to(dev) for t in AC.frames(TAG, step))
        losses.append(npvp_amd.ae_train_step(enc, dec, opt, dp.shard_batch(past, rank, world), dp.shard_batch(fut, rank, world),
                                             grad_sync=gs))
    torch.cuda.synchronize()
    if gs is not None:
        assert gs.launched > len(gs.buckets), "the overlapped path never ran"
        assert any(isinstance(m, dp.SyncBatchNorm2d) for m in opt.ae_pair.modules())
        gs.remove()
    return {"loss": torch.stack(losses).clone(), "params": opt.flat_p.clone(), "adam_m": opt.m.clone(), "adam_v": opt.v.clone(),
            "running": torch.cat([t.reshape(-1).float() for t in running_stats(opt.ae_pair)])}


def step_equals_plain():
    plain, again = three_steps(False), three_steps(False)
    c0 = COLLECTIVES[0]
    par = three_steps(True)
    say(f"statistics all-reduces of the three data-parallel steps: {COLLECTIVES[0] - c0}")
    assert COLLECTIVES[0] > c0
    eq_pp = {k: torch.equal(plain[k], again[k]) for k in plain}
    eq_dp = {k: torch.equal(plain[k], par[k]) for k in plain}
    k_pp = {k: rel(again[k], plain[k]) for k in plain}
    k_dp = {k: rel(par[k], plain[k]) for k in plain}
    d_pp, d_dp = max(k_pp.values()), max(k_dp.values())
    fmt = lambda d: ", ".join(f"{k} {e:.3e}" for k, e in d.items())
    say(f"three steps, plain vs plain': bit-equal {eq_pp}; rel-L2 {fmt(k_pp)} (distance = the largest: {d_pp:.3e})")
    say(f"three steps, data parallel vs plain: bit-equal {eq_dp}; rel-L2 {fmt(k_dp)} (distance = the largest: {d_dp:.3e})")
    say(f"per step losses: plain {plain['loss'].tolist()}  plain' {again['loss'].tolist()}  data parallel {par['loss'].tolist()}")
    if all(eq_pp.values()):
        assert all(eq_dp.values()), "the plain step repeats bit for bit, the data-parallel step on a group of one differs from it"
    else:
        assert d_dp <= 2 * d_pp, f"data parallel vs plain {d_dp:.3e} exceeds twice plain vs plain' {d_pp:.3e}"


if world > 1:
    fixture_steps()
    uneven_shards()
else:
    op_equals_plain()
    step_equals_plain()
dist.barrier()
say("OK")
dist.destroy_process_group()
