"""CPU: the host side of the any-grid non-local attention (npvp_nonlocal_attn_grid_fwd / _bwd): declared, bound, fast-wrapped,
argument checks before any launch - the guard that the existing pair still ends at the configs' grids - the predicate that states
the old rule, and which op the trainable autoencoder's attention picks."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["npvp_nonlocal_attn_grid_fwd", "npvp_nonlocal_attn_grid_bwd"]
CONFIG = {(8, 64, 64), (16, 32, 32), (32, 16, 16), (64, 8, 8)}        # (A, H, W) of the five AE configs; V = 4 A


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_declared_in_the_header_bound_and_fast_wrapped(L):
    from npvp_amd import _npvp_fast as FW
    from npvp_amd._lib import SIGNATURES
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npvp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(npvp_[a-z0-9_]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/npvp_hip.h"
        assert n in SIGNATURES, f"{n} has no signature in npvp_amd/_lib.py"
        assert hasattr(L._cdll, n) and getattr(L, n) is getattr(FW, n), n
    # the argument lists of the existing pair
    assert SIGNATURES["npvp_nonlocal_attn_grid_fwd"] == SIGNATURES["npvp_nonlocal_attn_fwd"]
    assert SIGNATURES["npvp_nonlocal_attn_grid_bwd"] == SIGNATURES["npvp_nonlocal_attn_bwd"]


def fwd_args(A=8, V=32, H=6, W=6, F_=2, ld=64, ldo=None, null=None):
    a = [16, ld, 16, ld, 16, ld, 16, V if ldo is None else ldo, 16, F_, H, W, A, V, None]
    if null is not None:
        a[null] = None
    return a


def bwd_args(A=8, V=32, H=6, W=6, F_=2, ld=64, null=None, **lds):
    # q ldq k ldk v ldv go ldgo lse D dq lddq dk lddk dv lddv F H W A V stream
    a = [16, ld, 16, ld, 16, ld, 16, V, 16, 16, 16, ld, 16, ld, 16, ld, F_, H, W, A, V, None]
    for k, v in lds.items():
        a[dict(ldq=1, ldk=3, ldv=5, ldgo=7, lddq=11, lddk=13, lddv=15)[k]] = v
    if null is not None:
        a[null] = None
    return a


def test_argument_errors_do_not_need_a_gpu(L):
    """(every call here fails its host-side check: nothing is launched)"""
    f, b, err = L.npvp_nonlocal_attn_grid_fwd, L.npvp_nonlocal_attn_grid_bwd, L.npvp_last_error
    for i in (0, 2, 4, 6, 8):
        assert f(*fwd_args(null=i)) == -1 and b"nonlocal_attn_grid_fwd: null buffer" in err(), i
    for i in (0, 2, 4, 6, 8, 9, 10, 12, 14):
        assert b(*bwd_args(null=i)) == -1 and b"nonlocal_attn_grid_bwd: null buffer" in err(), i
    for H, W in ((1, 6), (6, 1), (0, 0), (1, 1), (-2, 4)):
        assert f(*fwd_args(H=H, W=W)) == -1 and b"H >= 2, W >= 2" in err(), (H, W)
        assert b(*bwd_args(H=H, W=W)) == -1 and b"H >= 2, W >= 2" in err(), (H, W)
    assert f(*fwd_args(F_=0)) == -1 and b"F >= 1" in err()
    for A, V in ((12, 48), (8, 64), (16, 32), (4, 16), (128, 512)):
        assert f(*fwd_args(A=A, V=V, ld=1024)) == -1 and b"attn dim" in err(), (A, V)
        assert b(*bwd_args(A=A, V=V, ld=1024)) == -1 and b"attn dim" in err(), (A, V)
    assert f(*fwd_args(ld=7)) == -1 and b"leading dimensions" in err()
    assert f(*fwd_args(ld=31)) == -1 and b"leading dimensions" in err()              # ldv < V
    assert f(*fwd_args(ldo=31)) == -1 and b"leading dimensions" in err()
    for k, v in (("ldq", 7), ("ldk", 7), ("ldv", 31), ("ldgo", 31), ("lddq", 7), ("lddk", 7), ("lddv", 31)):
        assert b(*bwd_args(**{k: v})) == -1 and b"leading dimensions" in err(), k
    # F*H*W >= 2^31 (the largest below passes this check and fails the next one, so still nothing is launched)
    assert f(*fwd_args(F_=1 << 15, H=256, W=256)) == -1 and b"2^31" in err()
    assert b(*bwd_args(F_=1 << 15, H=256, W=256)) == -1 and b"2^31" in err()
    assert f(*fwd_args(F_=(1 << 15) - 1, H=256, W=256, ld=7)) == -1 and b"leading dimensions" in err()
    # a config shape is checked by this entry point before it is handed on
    assert f(*fwd_args(A=64, V=256, H=8, W=8, ld=63)) == -1 and b"nonlocal_attn_grid_fwd: leading dimensions" in err()


def test_the_existing_entry_points_still_end_at_the_config_grids(L):
    old = lambda A, V, H, W: (16, 64, 16, 64, 16, 64, 16, 64, 16, 2, H, W, A, V, None)
    assert L.npvp_nonlocal_attn_fwd(*old(8, 32, 6, 6)) == -1 and b"nonlocal_attn:" in L.npvp_last_error()
    assert L.npvp_nonlocal_attn_fwd(*old(8, 32, 32, 32)) == -1 and b"grid not supported" in L.npvp_last_error()
    a = bwd_args(A=8, V=32, H=6, W=6)
    assert L.npvp_nonlocal_attn_bwd(*a) == -1 and b"nonlocal_attn:" in L.npvp_last_error()
    from npvp_amd import ops
    with pytest.raises(RuntimeError, match="grid"):
        ops.nonlocal_attn_packed(torch.zeros(36, 48), 1, 6, 6, 8, 32)
    assert ops._NL_GRID == {8: 64, 16: 32, 32: 16, 64: 8}


def test_config_shape_predicate_states_the_old_rule():
    """true for exactly the four (C, grid) pairs of the configs over square grids; over every grid, true exactly where
    nonlocal_attn_packed gets past its own shape check (H even, W a power of two, the config's cell count: a 16x64 grid at C=128
    has always been accepted) - a CPU tensor is then refused one step later, without a launch"""
    from npvp_amd import ops
    sides = (2, 3, 4, 6, 8, 12, 16, 24, 32, 40, 64, 96, 128, 256)
    hit = set()
    for A in (4, 8, 12, 16, 32, 64, 128):
        for H in sides:
            for W in sides:
                got = ops.nonlocal_attn_config_shape(A, 4 * A, H, W)
                assert not ops.nonlocal_attn_config_shape(A, 4 * A + 4, H, W)
                if got and H == W:
                    hit.add((A, H, W))
                try:
                    ops.nonlocal_attn_packed(torch.empty(H * W, 6 * A), 1, H, W, A, 4 * A)
                    old = None
                except RuntimeError as e:
                    old = "MI355X" in str(e)
                assert old is not None and got == old, (A, H, W, got, old)
    assert hit == CONFIG


def test_op_argument_checks():
    from npvp_amd import ops
    with pytest.raises(RuntimeError, match="attn dim"):
        ops.nonlocal_attn_grid_packed(torch.zeros(36, 72), 1, 6, 6, 12, 48)
    with pytest.raises(RuntimeError, match="attn dim"):
        ops.nonlocal_attn_grid_packed(torch.zeros(36, 72), 1, 6, 6, 8, 48)
    with pytest.raises(RuntimeError, match="2x2 window"):
        ops.nonlocal_attn_grid_packed(torch.zeros(6, 48), 1, 1, 6, 8, 32)
    with pytest.raises(RuntimeError, match="qkv must be"):
        ops.nonlocal_attn_grid_packed(torch.zeros(36, 47), 1, 6, 6, 8, 32)
    with pytest.raises(RuntimeError, match="qkv must be"):
        ops.nonlocal_attn_grid_packed(torch.zeros(35, 48), 1, 6, 6, 8, 32)
    with pytest.raises(RuntimeError, match=r"q / k \(F, H\*W, a\)"):
        ops.nonlocal_attn_grid(torch.zeros(1, 36, 8), torch.zeros(1, 36, 8), torch.zeros(1, 36, 32), 6, 5)
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor never reaches a kernel
        ops.nonlocal_attn_grid_packed(torch.zeros(36, 48), 1, 6, 6, 8, 32)


@pytest.mark.parametrize("C,H,W,want", [(64, 64, 64, "config"), (512, 8, 8, "config"), (64, 24, 40, "grid"), (512, 3, 5, "grid"),
                                        (128, 16, 64, "config"), (128, 64, 16, "config"), (128, 30, 32, "grid")])
def test_attn_picks_its_op_by_the_grid(monkeypatch, C, H, W, want):
    """models/ae_train._attn: the configs' (C, grid) pairs call ops.nonlocal_attn_packed (what they launch today), any other grid
    ops.nonlocal_attn_grid_packed - both replaced by recorders here"""
    from npvp_amd import ops
    from npvp_amd.models import ae_train as M
    from npvp_amd.models.ResNetAutoEncoder import NonLocalAttenion2D
    import torch.nn as nn
    calls = []
    rec = lambda tag: lambda qkv, N, H, W, A, V: (calls.append((tag, N, H, W, A, V, tuple(qkv.shape))), qkv[:, 2 * A:2 * A + V])[1]
    monkeypatch.setattr(ops, "nonlocal_attn_packed", rec("config"))
    monkeypatch.setattr(ops, "nonlocal_attn_grid_packed", rec("grid"))
    monkeypatch.setattr(ops, "linear", lambda x, w, b=None: F.linear(x, w, b))
    monkeypatch.setattr(ops, "bn_act_train", lambda x, *a, **k: x)
    attn = [m for m in M.build_autoencoder(dict(ngf=C // 2, n_downsampling=1, num_res_blocks=1, out_layer='Tanh', learn_3d=False), 1)[0]
            .modules() if isinstance(m, NonLocalAttenion2D)][0]
    assert (attn.attn_dim, attn.value_dim) == (C // 8, C // 2) and isinstance(attn.norm_func, nn.BatchNorm2d)
    with torch.no_grad():
        y = M._attn(attn, torch.zeros(2, C, H, W))
    assert y.shape == (2, C, H, W)
    assert calls == [(want, 2, H, W, C // 8, C // 2, (2 * H * W, -(-(C // 4 + C // 2) // 32) * 32))]


@pytest.mark.parametrize("N,H,W", [(4, 3, 5), (4, 6, 10), (1, 3, 5), (4, 12, 20)])
def test_attn_hands_the_gemms_whole_row_blocks(monkeypatch, N, H, W):
    """The weight-gradient GEMM sums over the token rows and takes only row counts % 32 == 0: _attn appends zero rows to the two
    projections' inputs and cuts them from the outputs.  Here the projections are F.linear with a recorder: their row counts, that
    the attention op still sees F*H*W rows, and that the output and every gradient equal those of the same block without
    padding (zero rows add exact zeros, so the bound is float32 rounding of the differently blocked F.linear sums)."""
    from npvp_amd import ops
    from npvp_amd.models import ae_train as M
    from npvp_amd.models.ResNetAutoEncoder import NonLocalAttenion2D
    C, rows = 64, []

    def linear(x, w, b=None):
        rows.append(x.shape[0])
        return F.linear(x, w, b)

    def attn_op(qkv, N_, H_, W_, A, V):
        assert qkv.shape[0] == N_ * H_ * W_
        return qkv[:, 2 * A:2 * A + V] * qkv[:, :1]
    monkeypatch.setattr(ops, "nonlocal_attn_grid_packed", attn_op)
    monkeypatch.setattr(ops, "linear", linear)
    monkeypatch.setattr(ops, "bn_act_train", lambda x, *a, **k: x)
    torch.manual_seed(7)
    attn = [m for m in M.build_autoencoder(dict(ngf=C // 2, n_downsampling=1, num_res_blocks=1, out_layer='Tanh', learn_3d=False), 1)[0]
            .modules() if isinstance(m, NonLocalAttenion2D)][0].double()
    with torch.no_grad():
        attn.gamma.fill_(0.5)
    x = torch.randn(N, C, H, W, dtype=torch.float64, requires_grad=True)
    g = torch.randn(N, C, H, W, dtype=torch.float64)
    params = [x] + list(attn.parameters())
    got = torch.autograd.grad(M._attn(attn, x), params, g, allow_unused=True)
    y = M._attn(attn, x)
    assert rows[:2] == [-(-N * H * W // 32) * 32] * 2 and y.shape == x.shape
    # the same block, no padding: the projections written out
    A, V = attn.attn_dim, attn.value_dim
    tok = x.permute(0, 2, 3, 1).reshape(N * H * W, C)
    q, v = attn.Wq(tok), attn.Wv(tok)
    o = F.linear(v * q[:, :1], attn.out_proj.weight, attn.out_proj.bias).view(N, H, W, C).permute(0, 3, 1, 2)
    want_y = x + attn.gamma * o                 # (the stubbed bn_act_train carries the ReLU too)
    want = torch.autograd.grad(want_y, params, g, allow_unused=True)
    assert torch.allclose(y, want_y, rtol=0, atol=1e-12)
    for p, a, b in zip(params, got, want):
        b = torch.zeros_like(p) if b is None else b           # (Wk: unused by the stand-in attention)
        if a is not None or bool(b.any()):
            assert torch.allclose(a, b, rtol=0, atol=1e-12 * max(1.0, float(b.abs().max()))), tuple(p.shape)
