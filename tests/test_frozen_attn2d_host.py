"""CPU: the host side of the frozen encoder's opt-in NonLocalAttenion2D route - the attn2d switch of to_device_layout /
fuse_frozen_autoencoder, the C ABI of npvp_bias_act_scaled and its refusals, the case tables of tests/frozen_attn2d_cases.py, and that
float64 restatement against the module's own forward and against seven wrong restatements at the bar the GPU tests use."""
import copy

import pytest
import torch
import torch.nn as nn

import frozen_attn2d_cases as FC
from oracle import ops as O

NAME = "npvp_bias_act_scaled"
AE_SMALL = dict(ngf=32, n_downsampling=2, num_res_blocks=1, learn_3d=True, out_layer='Tanh')        # attn2d at C = 64 and C = 128


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def _pair():
    import npvp_amd
    enc, dec = npvp_amd.build_frozen_autoencoder(AE_SMALL, 1)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), 711)
    return enc, dec


def _attn2ds(enc):
    from npvp_amd.models import Factorized3DConvAttn
    return [(n, m.attn2d) for n, m in enc.named_children() if isinstance(m, Factorized3DConvAttn)]


# ------------------------------------------------------------------------------------------------------------------ the switch
def test_the_switch_refuses_unknown_values_by_name():
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    enc, dec = _pair()
    before = [n for n, _ in enc.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="attn2d=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, attn2d=bad)
        with pytest.raises(ValueError, match="attn2d="):
            npvp_amd.to_device_layout(enc, dec, "cpu", attn2d=bad)
    assert [n for n, _ in enc.named_modules()] == before and isinstance(enc.block0[2], nn.BatchNorm2d), "a refused call changed the pair"


def test_stock_is_the_default_and_touches_no_attn2d():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, NonLocalAttenion2D
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, attn2d="stock")
    assert [n for n, _ in e0.named_modules()] == [n for n, _ in e1.named_modules()]
    for e in (e0, e1):
        found = _attn2ds(e)
        assert len(found) == 2
        for n, a in found:
            assert not [b for b, _ in a.named_buffers() if b.startswith("_npvp_")], n
            assert "forward" not in a.__dict__ and type(a) is NonLocalAttenion2D and type(a).forward is NonLocalAttenion2D.forward, n
            assert isinstance(a.norm_func, nn.Identity)
    for (k0, v0), (k1, v1) in zip(e0.state_dict().items(), e1.state_dict().items()):
        assert k0 == k1 and torch.equal(v0, v1), k0


def test_hip_registers_the_buffers_and_folds_the_batchnorm_as_before():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, _fused_attn2d
    (e0, d0), (e1, d1) = _pair(), _pair()
    raw = dict(_attn2ds(copy.deepcopy(e0)))
    fuse_frozen_autoencoder(e0, d0, attn2d="stock")
    fuse_frozen_autoencoder(e1, d1, attn2d="hip")
    assert [n for n, _ in e0.named_modules()] == [n for n, _ in e1.named_modules()], "the module tree depends on the switch"
    assert list(e0.state_dict()) == list(e1.state_dict()), "the buffers must be non-persistent"
    for (n, s), (_, h) in zip(_attn2ds(e0), _attn2ds(e1)):
        A, V, C = h.attn_dim, h.value_dim, h.in_channels
        assert h.forward.__func__ is _fused_attn2d and h.forward.__self__ is h, n
        assert torch.equal(h._npvp_wqkv, torch.cat([h.Wq.weight, h.Wk.weight, h.Wv.weight], 0)) and h._npvp_wqkv.shape == (2 * A + V, C)
        assert torch.equal(h._npvp_bqkv, torch.cat([h.Wq.bias, h.Wk.bias, h.Wv.bias], 0))
        assert not h._npvp_wqkv.requires_grad and not h.gamma.requires_grad
        # the fold is the stock switch's, and it is BatchNorm2d(eval) behind out_proj
        assert isinstance(h.norm_func, nn.Identity)
        assert torch.equal(h.out_proj.weight, s.out_proj.weight) and torch.equal(h.out_proj.bias, s.out_proj.bias)
        bn, lin = raw[n].norm_func, raw[n].out_proj
        y = O.seeded_randn((5, V), 3)
        want = bn(lin(y).view(5, C, 1, 1)).view(5, C)
        assert FC.rel(h.out_proj(y), want) < 1e-6
        # attn1d is the same under either switch
        assert torch.equal(getattr(e0, n).attn1d._npvp_wqkv, getattr(e1, n).attn1d._npvp_wqkv)
    # a copy of a routed module routes to itself
    c = copy.deepcopy(e1)
    for (_, a) in _attn2ds(c):
        assert a.forward.__self__ is a


def test_hip_leaves_an_attention_without_kernels_on_its_own_forward():
    """ngf 8: (attn_dim, value_dim) = (2, 8) and (4, 16) have no non-local kernels"""
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    enc, dec = npvp_amd.build_frozen_autoencoder(dict(AE_SMALL, ngf=8, learn_3d=False), 1)
    ref = copy.deepcopy(enc)
    fuse_frozen_autoencoder(enc, dec, attn2d="hip")
    for n, a in _attn2ds(enc):
        assert not npvp_amd.ops.nonlocal_attn_dims(a.attn_dim, a.value_dim)
        assert "forward" not in a.__dict__ and not hasattr(a, "_npvp_wqkv"), n
    with torch.no_grad():
        for (n, a), (_, r) in zip(_attn2ds(enc), _attn2ds(ref)):
            x = O.seeded_randn((2, a.in_channels, 4, 6), 5).contiguous(memory_format=torch.channels_last)
            assert FC.rel(a(x), r(x)) < 1e-5, n


def test_routed_forward_keeps_stock_for_other_inputs_and_refuses_grad(monkeypatch):
    """on CPU tensors: NCHW memory and a grid without a 2x2 window run NonLocalAttenion2D.forward itself (the same bits, no op of the HIP
    route called); a channels-last input that requires grad is refused and the message names the switch"""
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, NonLocalAttenion2D
    called = []
    for op in ("nonlocal_attn_packed", "nonlocal_attn_grid_packed"):
        monkeypatch.setattr(ops, op, lambda qkv, Fr, H, W, A, V, _op=op: (called.append(_op), qkv[:, 2 * A:2 * A + V])[1])
    monkeypatch.setattr(ops, "bias_act_scaled", lambda y, *a, **k: (called.append("bias_act_scaled"), y)[1])
    blk = FC.make_block(64)
    fuse_frozen_autoencoder(FC.Holder(blk), FC.Holder(), attn2d="hip")
    a = blk.attn2d
    assert "forward" in a.__dict__
    with torch.no_grad():
        x = O.seeded_randn((2, 64, 4, 6), 1)
        assert torch.equal(a(x), NonLocalAttenion2D.forward(a, x))
        for shape in ((2, 64, 1, 6), (2, 64, 6, 1)):          # the stock forward's own refusal (MaxPool2d), not one of the route's
            with pytest.raises(RuntimeError, match="Output size is too small"):
                a(O.seeded_randn(shape, 2).contiguous(memory_format=torch.channels_last))
    assert not called
    x = O.seeded_randn((1, 64, 4, 6), 4).contiguous(memory_format=torch.channels_last).requires_grad_()
    with pytest.raises(NotImplementedError, match='attn2d="hip"'):
        a(x)
    assert not called
    with torch.no_grad():           # no graph: the route is taken (here: the recorders)
        a(x)
    assert called == ["nonlocal_attn_grid_packed", "bias_act_scaled"]


def test_route_picks_the_config_kernels_at_config_shapes(monkeypatch):
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    taken = []

    def rec(name):
        def op(qkv, Fr, H, W, A, V):
            taken.append((name, tuple(qkv.shape), Fr, H, W, A, V))
            return qkv[:, 2 * A:2 * A + V]
        return op
    monkeypatch.setattr(ops, "nonlocal_attn_packed", rec("config"))
    monkeypatch.setattr(ops, "nonlocal_attn_grid_packed", rec("grid"))
    monkeypatch.setattr(ops, "bias_act_scaled", lambda y, b, s, act=0, residual=None: (taken.append(("tail", s is a.gamma, act)), y)[1])
    blk = FC.make_block(512)
    fuse_frozen_autoencoder(FC.Holder(blk), FC.Holder(), attn2d="hip")
    a = blk.attn2d
    with torch.no_grad():
        for (H, W) in ((8, 8), (4, 16), (16, 4), (3, 5)):
            a(O.seeded_randn((2, 512, H, W), 9).contiguous(memory_format=torch.channels_last))
    cores = [t[0] for t in taken if t[0] != "tail"]
    assert cores == ["config", "config", "config", "grid"], cores
    assert taken[0] == ("config", (2 * 64, 2 * 64 + 256), 2, 8, 8, 64, 256)
    assert all(t == ("tail", True, 1) for t in taken if t[0] == "tail")


# ----------------------------------------------------------------------------------------------------------------------- C ABI
def _args(x=4096, bias=8192, scale=None, res=None, out=12288, outer=4, inner=8, C=8, layout=0, act=1):
    return (x, bias, scale, res, out, outer, inner, C, layout, act, None)


REFUSALS = ((dict(x=None), b"empty problem"), (dict(bias=None), b"empty problem"), (dict(out=None), b"empty problem"),
            (dict(layout=2), b"layout 0 (channel = column) or 1 (channel = plane)"), (dict(inner=8, C=4), b"layout 0 needs inner == C"),
            (dict(act=4), b"act in 0..3"), (dict(act=-1), b"act in 0..3"), (dict(outer=0), b"empty problem"))


def test_export_and_argument_errors_do_not_need_a_gpu(L):
    """declared in the header the binding parses, defined in the library, reachable through the generated wrappers; every refusal is
    made on the host before anything is launched"""
    from npvp_amd import _lib, _npvp_fast as Fast
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    assert NAME in protos and len(protos[NAME][1]) == len(protos["npvp_bias_act"][1]) + 1
    assert protos[NAME][1][:4] == ["const float*"] * 4 and protos[NAME][1][-1] == "npvp_stream_t"
    assert hasattr(L._cdll, NAME) and getattr(L, NAME) is getattr(Fast, NAME)
    n0 = L.npvp_launch_count()
    for kw, what in REFUSALS:
        assert getattr(L, NAME)(*_args(**kw)) == -1, kw
        err = L.npvp_last_error()
        assert b"bias_act_scaled: " in err and what in err, (kw, err)
    assert L.npvp_launch_count() == n0


def test_op_is_forward_only_and_checks_its_arguments():
    from npvp_amd import ops
    x, b = torch.zeros(1, 4, 2, 2), torch.zeros(4)
    with pytest.raises(NotImplementedError, match="bias_act_scaled: forward only"):
        ops.bias_act_scaled(x.clone().requires_grad_(), b, None)
    with pytest.raises(NotImplementedError, match="bias_act_scaled: forward only"):
        ops.bias_act_scaled(x, b, torch.tensor(1.0, requires_grad=True), residual=x)
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor never reaches a kernel
        ops.bias_act_scaled(x, b, None)


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_kernel_case_table_covers_the_paths():
    names = [c[0] for c in FC.KERNEL_CASES]
    assert len(set(names)) == len(names)
    vec = {c[0]: FC.kernel_is_vector(c) for c in FC.KERNEL_CASES}
    assert vec == {"rows_c64_vector": True, "rows_c6_scalar_by_shape": False, "rows_c64_scalar_by_alignment": False,
                   "planes_c3_inner15": False, "rows_c64_vector_two_strides": True, "rows_c6_scalar_two_strides": False}
    for c in FC.KERNEL_CASES:
        _, layout, outer, inner, C, off = c
        assert (inner == C) if layout == 0 else (outer % C == 0)
        assert (FC.kernel_work(c) > FC.GRID_CAP) == (c in FC.LOOP_KERNEL_CASES), c
    assert any(c[2] * c[3] > 16384 * 256 * 4 for c in FC.KERNEL_CASES)
    ch = FC.kernel_channel(FC.SMALL_KERNEL_CASES[3])
    assert ch.shape == (6, 15) and ch[:, 0].tolist() == [0, 1, 2, 0, 1, 2]
    ref, pre = FC.kernel_ref64(FC.SMALL_KERNEL_CASES[1], 1, FC.SCALE, True)
    i = FC.kernel_inputs(FC.SMALL_KERNEL_CASES[1])
    e = (4, 5)
    assert float(ref[e]) == FC.SCALE * max(float(i["x"][e]) + float(i["bias"][5]), 0.0) + float(i["res"][e])


def test_module_shapes_are_the_routes_they_claim():
    from npvp_amd import ops
    for (C, H, W, Fr) in FC.MODULE_SHAPES:
        assert ops.nonlocal_attn_dims(C // 8, C // 2) and H >= 2 and W >= 2
        assert ops.nonlocal_attn_config_shape(C // 8, C // 2, H, W) == ((C, H, W, Fr) in FC.CONFIG_SHAPES)
    assert any(H % 2 and W % 2 for (_, H, W, _) in FC.GRID_SHAPES)


# --------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("shape", FC.MODULE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_float64_restatement_is_the_forward_and_rejects_wrong_ones(shape):
    """the restatement equals NonLocalAttenion2D.forward of the float64 module (1e-12), its inputs are what the docstring of the case
    file says, and every wrong restatement misses the attention branch out - x by more than the 1e-4 bar of the GPU tests"""
    C, H, W, Fr = shape
    a = FC.make_block(C).attn2d
    x = FC.module_input(shape)
    p = FC.params64(a)
    assert float(p["gamma"]) == FC.GAMMA and all(float(p[b].abs().min()) > 0 for b in ("bq", "bk", "bv", "bo", "bn_b"))
    with torch.no_grad():
        want = copy.deepcopy(a).double()(x.double())
        ref = FC.attn2d_ref64(p, x)
        tok = x.double().flatten(2).transpose(1, 2)
        scores = (tok @ p["Wq"].T + p["bq"]) @ (tok @ p["Wk"].T + p["bk"]).transpose(1, 2)
        assert FC.rel(ref, want) < 1e-12
        assert 0.3 < float(scores.std()) < 3.0, float(scores.std())
        branch = ref - x.double()
        assert float(branch.norm()) > 0.05 * float(x.norm()), "the branch is too small to be seen"
        for mutant in FC.MUTANTS:
            e = FC.rel(FC.attn2d_ref64(p, x, mutant) - x.double(), branch)
            print(f"{shape} {mutant}: {e:.2e}")
            assert e > 10 * FC.BAR, (mutant, e)
