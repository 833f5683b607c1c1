"""GPU: synchronised BatchNorm of the data-parallel Stage-1 path through the C ABI (npvp_bn_act_apply_sync, npvp_bn_bwd_sums,
npvp_bn_act_bwd_apply of csrc/ae_train.hip), in one process: a batch split along N into two UNEVEN shards.
  1. per shard, alone: the split calls fed the shard's own sums and count give the bits of npvp_bn_act_apply / npvp_bn_act_bwd;
  2. the two shards' buffers added on the device (what the all-reduce does), each shard applied with the sums: the concatenation is
     the whole batch's BatchNorm (float64 on the CPU), forward, backward and running statistics;
  3. the collectors of the two rehearsal jobs tools/dp_jobs.py starts first (tools/ae_dp_check.py on 2 gloo ranks and on 1 RCCL rank).
"""
import functools
import os
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL_TOL = 1e-5        # the bound tests/test_hip_ae_train.py:13 holds these kernels to: hand-written kernels vs float64, no MIOpen
EPS, MOM = 1e-5, 0.1

# (layout, C, H, W, frames of shard a, frames of shard b)
SHAPES = [
    (0, 4, 2, 2, 1, 2),          # smallest C
    (0, 64, 3, 3, 2, 3),         # 18 and 27 rows: odd, one part
    (0, 32, 12, 12, 2, 3),       # 288 and 432 rows: more than one part
    (0, 512, 8, 8, 1, 2),        # the BAIR / KTH bottleneck, 8 channel blocks
    (1, 64, 3, 4, 2, 3),
    (1, 512, 8, 8, 1, 2),
]
IDS = [f"l{s[0]}-c{s[1]}-{s[2]}x{s[3]}-{s[4]}+{s[5]}" for s in SHAPES]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    import npvp_amd  # noqa: F401
    from npvp_amd._lib import lib
    return lib()


@functools.lru_cache(maxsize=None)
def _inputs(shape, with_res):
    """seeded CPU tensors in NCHW: x, w, b, residual, upstream gradient, initial running statistics (never modified)"""
    layout, C, H, W, na, nb = shape
    full = (na + nb, C, H, W)
    x = O.seeded_randn(full, 1) * 1.7 + 0.6
    w, b = 1 + 0.1 * O.seeded_randn((C,), 2), 0.1 * O.seeded_randn((C,), 3)
    res = O.seeded_randn(full, 4) if with_res else None
    g = O.seeded_randn(full, 5)
    rm, rv = 0.1 * O.seeded_randn((C,), 6), 0.5 + O.seeded_randn((C,), 7).abs()
    return x, w, b, res, g, rm, rv


@functools.lru_cache(maxsize=None)
def _reference(shape, act, with_res):
    """whole-batch F.batch_norm(training=True) (+ ReLU) (+ residual) in float64 on the CPU: y, dx, dw, db, running statistics"""
    x, w, b, res, g, rm, rv = _inputs(shape, with_res)
    xd, wd, bd = (t.double().requires_grad_() for t in (x, w, b))
    rmd, rvd = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(xd, rmd, rvd, wd, bd, True, MOM, EPS)
    if act:
        y = torch.relu(y)
    if with_res:
        y = y + res.double()
    y.backward(g.double())
    return y.detach(), xd.grad, wd.grad, bd.grad, rmd, rvd


def _mem(t, layout):
    """NCHW tensor -> the device memory the kernels read: rows [N*H*W][C] (layout 0) or planes [N*C][H*W] (layout 1)"""
    t = t.to(DEV)
    return t.permute(0, 2, 3, 1).contiguous() if layout == 0 else t.contiguous()


def _nchw(t, layout):
    return t.permute(0, 3, 1, 2) if layout == 0 else t


class _Shard:
    """one rank's slice of the batch on the device and the C calls on it"""

    def __init__(self, L, shape, frames, with_res):
        self.L = L
        self.layout, self.C, H, W = shape[:4]
        x, w, b, res, g, rm, rv = _inputs(shape, with_res)
        self.x, self.g = _mem(x[frames], self.layout), _mem(g[frames], self.layout)
        self.res = _mem(res[frames], self.layout) if with_res else None
        self.w, self.b = w.to(DEV), b.to(DEV)
        self.rm0, self.rv0 = rm.to(DEV), rv.to(DEV)
        n = self.x.shape[0]
        self.outer, self.inner = (n * H * W, self.C) if self.layout == 0 else (n * self.C, H * W)
        self.count = n * H * W
        self.wsn = L.npvp_bn_workspace_bytes(self.C)
        self.ws = torch.empty(self.wsn // 4, dtype=torch.float32, device=DEV)

    def stat(self):
        """[sum x, sum x^2, n] of this shard (2C+1 doubles)"""
        st = torch.empty(2 * self.C + 1, dtype=torch.float64, device=DEV)
        assert self.L.npvp_bn_stats(self.x.data_ptr(), self.outer, self.inner, self.C, self.layout, st.data_ptr(), self.ws.data_ptr(),
                                    self.wsn, None) == 0, self.L.npvp_last_error()
        st[2 * self.C:].fill_(float(self.count))
        return st

    def _out(self):
        f = lambda: torch.empty(self.C, dtype=torch.float32, device=DEV)
        return torch.empty_like(self.x), f(), f(), self.rm0.clone(), self.rv0.clone()

    def apply_fused(self, act):
        st = self.stat()
        y, mean, rstd, rm, rv = self._out()
        p = lambda t: None if t is None else t.data_ptr()
        assert self.L.npvp_bn_act_apply(p(self.x), p(self.w), p(self.b), p(self.res), p(st), self.count, EPS, MOM, p(rm), p(rv), self.outer,
                                        self.inner, self.C, self.layout, act, p(y), p(mean), p(rstd), None) == 0, self.L.npvp_last_error()
        return y, mean, rstd, rm, rv

    def apply_sync(self, act, st):
        y, mean, rstd, rm, rv = self._out()
        p = lambda t: None if t is None else t.data_ptr()
        assert self.L.npvp_bn_act_apply_sync(p(self.x), p(self.w), p(self.b), p(self.res), p(st), EPS, MOM, p(rm), p(rv), self.outer,
                                             self.inner, self.C, self.layout, act, p(y), p(mean), p(rstd), None) == 0, self.L.npvp_last_error()
        return y, mean, rstd, rm, rv

    def bwd_fused(self, act, mean, rstd, ws=None):
        """ws: a workspace of the caller's (a byte tensor) instead of the shard's own"""
        dx, dw, db = torch.empty_like(self.x), torch.empty_like(mean), torch.empty_like(mean)
        ws, wsn = (self.ws, self.wsn) if ws is None else (ws, ws.numel())
        assert self.L.npvp_bn_act_bwd(self.g.data_ptr(), self.x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), self.w.data_ptr(),
                                      self.b.data_ptr(), self.outer, self.inner, self.C, self.layout, act, 1, dx.data_ptr(), dw.data_ptr(),
                                      db.data_ptr(), ws.data_ptr(), wsn, None) == 0, self.L.npvp_last_error()
        return dx, dw, db

    def bwd_sums(self, act, mean, rstd):
        sums = torch.empty(2 * self.C, dtype=torch.float64, device=DEV)
        dw, db = torch.empty_like(mean), torch.empty_like(mean)
        assert self.L.npvp_bn_bwd_sums(self.g.data_ptr(), self.x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), self.w.data_ptr(),
                                       self.b.data_ptr(), self.outer, self.inner, self.C, self.layout, act, sums.data_ptr(), dw.data_ptr(),
                                       db.data_ptr(), self.ws.data_ptr(), self.wsn, None) == 0, self.L.npvp_last_error()
        return sums, dw, db

    def bwd_apply(self, act, mean, rstd, sums, st):
        dx = torch.empty_like(self.x)
        assert self.L.npvp_bn_act_bwd_apply(self.g.data_ptr(), self.x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), self.w.data_ptr(),
                                            self.b.data_ptr(), sums.data_ptr(), st.data_ptr() + 2 * self.C * 8, self.outer, self.inner,
                                            self.C, self.layout, act, dx.data_ptr(), None) == 0, self.L.npvp_last_error()
        return dx


def _shards(L, shape, with_res):
    na, nb = shape[4:]
    return _Shard(L, shape, slice(0, na), with_res), _Shard(L, shape, slice(na, na + nb), with_res)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
def test_split_calls_equal_fused_bit_for_bit(L, shape, act, with_res):
    """each shard alone, with its own sums and count: stats + apply_sync == bn_act_apply, bwd_sums + bwd_apply == bn_act_bwd.
    At (0, 32, 12, 12, 2, 3) - 288 and 432 rows: two parts per shard - the fused backward is also run in a fresh workspace of exactly
    npvp_bn_workspace_bytes(C) bytes, every double in it a NaN: its sums and its partials share that buffer and must not overlap."""
    for sh in _shards(L, shape, with_res):
        fused = sh.apply_fused(act)
        st = sh.stat()
        split = sh.apply_sync(act, st)
        for name, a, b in zip(("y", "mean", "rstd", "running_mean", "running_var"), split, fused):
            assert torch.equal(a, b), name
        mean, rstd = fused[1], fused[2]
        dx, dw, db = sh.bwd_fused(act, mean, rstd)
        sums, dw2, db2 = sh.bwd_sums(act, mean, rstd)
        dx2 = sh.bwd_apply(act, mean, rstd, sums, st)
        assert torch.equal(dx2, dx), "dx"
        assert torch.equal(dw2, dw) and torch.equal(db2, db), "dw / db"
        if shape == (0, 32, 12, 12, 2, 3):
            tight = torch.full((L.npvp_bn_workspace_bytes(sh.C),), 0xFF, dtype=torch.uint8, device=DEV)
            for name, a, b in zip(("dx", "dw", "db"), sh.bwd_fused(act, mean, rstd, tight), (dx2, dw2, db2)):
                assert torch.equal(a, b), f"{name}, workspace of exactly npvp_bn_workspace_bytes(C)"
        assert not torch.equal(split[3], sh.rm0)                      # (the running statistics were updated, not left alone)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("with_res", [False, True])
def test_two_uneven_shards_equal_whole_batch_float64(L, shape, act, with_res):
    """stat and sums of the two shards added on the device, each shard applied with the totals == whole-batch BatchNorm in float64"""
    layout = shape[0]
    a, b = _shards(L, shape, with_res)
    st = a.stat() + b.stat()
    assert float(st[-1]) == a.count + b.count
    fa, fb = a.apply_sync(act, st), b.apply_sync(act, st)
    for k in range(1, 5):                                             # mean, rstd, both running statistics: the same on both shards
        assert torch.equal(fa[k], fb[k])
    (sa, dwa, dba), (sb, dwb, dbb) = a.bwd_sums(act, fa[1], fa[2]), b.bwd_sums(act, fb[1], fb[2])
    sums = sa + sb
    dxa, dxb = a.bwd_apply(act, fa[1], fa[2], sums, st), b.bwd_apply(act, fb[1], fb[2], sums, st)
    y = _nchw(torch.cat([fa[0], fb[0]]), layout)
    dx = _nchw(torch.cat([dxa, dxb]), layout)
    yd, dxd, dwd, dbd, rmd, rvd = _reference(shape, act, with_res)
    errs = {"y": rel(y, yd), "dx": rel(dx, dxd), "dw": rel(dwa + dwb, dwd), "db": rel(dba + dbb, dbd),
            "running_mean": rel(fa[3], rmd), "running_var": rel(fa[4], rvd)}
    print(errs)
    for k, e in errs.items():
        assert e < KERNEL_TOL, (k, e)


# ------------------------------------------------------------------------------------------------- the two rehearsal jobs
def _job_log(request, name, deadline_s=660.0):
    """the log of job `name` of tools/dp_jobs.py once its line stands in <log>.times.  The two jobs run first, each under its own
    300 s limit, so the deadline covers both; nothing is waited for beyond that line and nothing is killed."""
    job = getattr(request.config, "_npvp_dp_job", None)
    if job is None:
        pytest.skip("the rehearsal jobs are only started for `-m gpu` sessions on a box with a GPU")
    proc, log_path = job
    read = lambda suffix: open(f"{log_path}.{suffix}").read() if os.path.exists(f"{log_path}.{suffix}") else ""
    done = lambda: [l for l in read("times").splitlines() if l.split(" ")[0] == name]
    end = time.monotonic() + deadline_s
    line = done()
    while not line and proc.poll() is None and time.monotonic() < end:
        time.sleep(0.5)
        line = done()
    line = line or done()
    assert line, f"job {name} has not finished (wrapper rc={proc.poll()}): {read('times')!r}\n{read(name)[-3000:]}"
    print(f"\n[dp jobs] {line[0]}")
    return line[0], read(name)


def test_ae_two_ranks_equal_whole_batch(request):
    """tools/ae_dp_check.py, 2 gloo ranks on the card: two data-parallel Stage-1 steps == the reference LitAE's whole-batch steps
    (tests/golden/ae_train_64.npz), cross-rank identity, the collective count, uneven shards through autograd"""
    line, log = _job_log(request, "ae_dp2")
    assert "[ae_dp_check] OK" in log, f"tools/ae_dp_check.py on 2 ranks failed ({line}):\n{log[-3000:]}"
    assert "world=2" in log and "backend=gloo" in log, log[-2000:]


def test_ae_one_rccl_rank_equals_plain_step(request):
    """tools/ae_dp_check.py on one forced RCCL rank: the double all-reduces on real RCCL; op and step equal the plain path"""
    line, log = _job_log(request, "ae_dp1")
    assert "[ae_dp_check] OK" in log, f"tools/ae_dp_check.py on 1 RCCL rank failed ({line}):\n{log[-3000:]}"
    assert "world=1" in log and "backend=nccl" in log, log[-2000:]
