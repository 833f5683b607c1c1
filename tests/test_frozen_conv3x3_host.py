"""CPU: the host side of the frozen encoder's opt-in 3 x 3 convolution route - the conv3x3 switch of to_device_layout /
fuse_frozen_autoencoder and which convolutions it marks, the index function and the planner the kernel calls (exported unchanged by the
C ABI), the refusals of the entry points, and the float64 reference of tests/frozen_conv3x3_cases.py against seven wrong restatements."""
import copy
import ctypes
import os

import pytest
import torch
import torch.nn as nn

import frozen_conv3x3_cases as CC
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE_SMALL = dict(ngf=32, n_downsampling=2, num_res_blocks=1, learn_3d=True, out_layer='Tanh')


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def _ints(n):
    buf = (ctypes.c_int * n)()
    return buf, ctypes.addressof(buf)


# ------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.fixture(scope="module")
def refs():
    return {c: (CC.inputs(c), CC.ref64(c)) for c in CC.KERNEL_CASES}


def test_reference_is_the_padded_convolution_of_the_modules(refs):
    """the reference equals what the module stack computes in float64: ReflectionPad2d / zero padding -> Conv2d -> activation, + skip"""
    for case in (CC.KERNEL_CASES[0], CC.KERNEL_CASES[2], CC.KERNEL_CASES[5]):
        Ci, Co, H, W, Fr, pad, act, res = case
        i, ref = refs[case]
        conv = nn.Conv2d(Ci, Co, 3, padding=1 if pad == "zero" else 0).double()
        with torch.no_grad():
            conv.weight.copy_(i["w"]); conv.bias.copy_(i["bias"])
            x = i["x"].double()
            y = CC.act64(conv(nn.ReflectionPad2d(1)(x) if pad == "reflect" else x), act)
            if res:
                y = y + i["res"].double()
        assert CC.rel(y, ref) < 1e-12, case
    i, _ = refs[CC.SCALED_CASE]
    assert 1000 < float(i["x"].abs().max()) and float(i["w"].abs().max()) < 1e-3, "the scaled case is not scaled"


def test_every_mutant_misses_the_bar_by_two_orders(refs):
    worst = {m: 0.0 for m in CC.MUTANTS}
    for case in CC.KERNEL_CASES:
        ins, ref = refs[case]
        for m in CC.MUTANTS:
            e = CC.rel(CC.ref64(case, m, ins), ref)
            worst[m] = max(worst[m], e)
            if m in CC.PADDING_MUTANTS and case[5] == "reflect":
                assert e > 100 * CC.F16X3_TOL, (m, CC.case_id(case), e)
    print(worst)
    for m, e in worst.items():
        assert e > 100 * CC.F16X3_TOL, (m, e)


def test_case_table_reaches_what_it_claims(L):
    ids = [CC.case_id(c) for c in CC.KERNEL_CASES]
    assert len(set(ids)) == len(ids)
    assert CC.rows(CC.KERNEL_CASES[0]) == 192 and CC.rows(CC.KERNEL_CASES[0]) % 128
    assert {c[5] for c in CC.KERNEL_CASES} == {"zero", "reflect"} and {c[6] for c in CC.KERNEL_CASES} >= {"none", "relu", "tanh"}
    assert any(c[2] == 2 and c[5] == "reflect" for c in CC.KERNEL_CASES) and any(c[2] == 1 for c in CC.KERNEL_CASES)
    assert any(c[0] != c[1] for c in CC.KERNEL_CASES) and any(not c[7] for c in CC.KERNEL_CASES)
    variants = set()
    for c in CC.KERNEL_CASES:
        out, p = _ints(6)
        assert L.npvp_conv3x3_route(c[4], c[2], c[3], c[0], c[1], p) == 0
        variants.add(out[0])
    assert variants == {1, 2}, "both tile variants are in the table"
    # a tile that holds pixels of two frames
    c = CC.KERNEL_CASES[5]
    assert c[4] > 1 and c[2] * c[3] < 128


# ------------------------------------------------------------------------------------------------- index function and planner
@pytest.mark.parametrize("pad_mode", [0, 1])
def test_src_is_the_index_map_of_functional_pad(L, pad_mode):
    """exhaustive: every extent 1..9 (2..9 for reflection), every coordinate, every tap"""
    n = 0
    for extent in range(1 + pad_mode, 10):
        want = CC.expected_src(extent, pad_mode)
        for c in range(extent):
            for tap in range(3):
                assert L.npvp_conv3x3_src(c, tap, extent, pad_mode) == want[c][tap], (extent, c, tap, pad_mode)
                n += 1
    assert n == 3 * sum(range(1 + pad_mode, 10))
    if pad_mode == 1:
        assert [L.npvp_conv3x3_src(c, t, 2, 1) for c in range(2) for t in range(3)] == [1, 0, 1, 0, 1, 0]
    else:
        assert [L.npvp_conv3x3_src(0, t, 1, 0) for t in range(3)] == [-1, 0, -1]


def test_src_refuses_what_is_outside_its_domain(L):
    for args in ((0, 3, 4, 0), (0, -1, 4, 0), (4, 0, 4, 0), (-1, 0, 4, 0), (0, 0, 1, 1), (0, 0, 0, 0), (0, 0, 4, 2)):
        assert L.npvp_conv3x3_src(*args) == -2, args


@pytest.mark.parametrize("case", CC.KERNEL_CASES, ids=CC.case_id)
def test_the_planners_tiles_are_a_partition(L, case):
    """every (row, column) of the [F H W][C_out] output belongs to exactly one workgroup of the plan"""
    Ci, Co, H, W, Fr = case[:5]
    out, p = _ints(6)
    assert L.npvp_conv3x3_route(Fr, H, W, Ci, Co, p) == 0
    variant, bm, bn, tm, tn, grid = list(out)
    M = Fr * H * W
    assert (variant, bn) == ((1, 128) if Co % 128 == 0 else (2, 64)) and bm == 128
    assert tm == -(-M // bm) and tn == Co // bn and grid == tm * tn
    count = torch.zeros(M, Co, dtype=torch.int32)
    t4, p4 = _ints(4)
    for b in range(grid):
        assert L.npvp_conv3x3_tile(Fr, H, W, Ci, Co, b, p4) == 0
        m0, m1, n0, n1 = list(t4)
        assert 0 <= m0 < m1 <= M and m1 - m0 <= bm and 0 <= n0 < n1 <= Co and n1 - n0 == bn
        count[m0:m1, n0:n1] += 1
    assert int(count.min()) == 1 and int(count.max()) == 1
    for bad in (-1, grid):
        assert L.npvp_conv3x3_tile(Fr, H, W, Ci, Co, bad, p4) == -1


def test_entry_points_are_declared_and_refuse_on_the_host(L):
    from npvp_amd import _lib
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    for name in ("npvp_conv3x3_planes_bytes", "npvp_conv3x3_planes", "npvp_conv3x3_f16", "npvp_conv3x3_route", "npvp_conv3x3_tile",
                 "npvp_conv3x3_src"):
        assert name in protos and hasattr(L._cdll, name), name
    assert protos["npvp_conv3x3_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_conv3x3_f16"][1]) == 18
    assert L.npvp_conv3x3_planes_bytes(128, 256) == 2 * 2 * 9 * 128 * 256 and L.npvp_conv3x3_planes_bytes(96, 128) == -1
    out, p = _ints(6)
    for shape in ((1, 8, 8, 96, 128), (1, 8, 8, 128, 32), (0, 8, 8, 64, 64), (1 << 20, 64, 64, 64, 64)):
        assert L.npvp_conv3x3_route(*shape, p) == -1, shape

    def args(**kw):
        a = dict(x=4096, planes=8192, bias=12288, res=None, y=16384, F=1, H=4, W=4, Ci=64, Co=64, pad=0, act=1, xa=20480, wa=24576,
                 ya=None, ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)
    n0 = L.npvp_launch_count()
    for kw, what in ((dict(x=None), b"non-null"), (dict(xa=None), b"non-null"), (dict(Ci=96), b"multiples of 64"),
                     (dict(pad=2), b"pad_mode 0 (zero) or 1 (reflect)"), (dict(pad=1, H=1), b"reflection padding needs H, W >= 2"),
                     (dict(act=4), b"act in 0..3"), (dict(y=16388), b"16-byte aligned")):
        assert L.npvp_conv3x3_f16(*args(**kw)) == -1, kw
        assert what in L.npvp_last_error(), (kw, L.npvp_last_error())
    assert L.npvp_conv3x3_planes(None, 64, 64, 8192, 4096, None) == -1 and L.npvp_conv3x3_planes(4096, 64, 96, 8192, 4096, None) == -1
    assert L.npvp_launch_count() == n0, "a refused call launched something"


# ------------------------------------------------------------------------------------------------------------------ the switch
def _pair(AE=AE_SMALL, ci=1, padding_type=None):
    import npvp_amd
    enc, dec = npvp_amd.build_frozen_autoencoder(AE, ci)
    if padding_type is not None:
        from npvp_amd.models import ResnetBlock
        for n, m in list(enc.named_children()):
            if isinstance(m, ResnetBlock):
                setattr(enc, n, ResnetBlock(m.conv_block[1].in_channels, padding_type, nn.BatchNorm2d, False, False).eval())
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), 811)
    return enc, dec


def _folded(m):
    from npvp_amd.models.ResNetAutoEncoder import FoldedConvAct
    return [(n, c) for n, c in m.named_modules() if isinstance(c, FoldedConvAct)]


def test_the_switch_refuses_unknown_values_by_name():
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, CONV3X3_ROUTES
    assert CONV3X3_ROUTES == ("stock", "hip")
    enc, dec = _pair()
    before = [n for n, _ in enc.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="conv3x3=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, conv3x3=bad)
        with pytest.raises(ValueError, match="conv3x3="):
            npvp_amd.to_device_layout(enc, dec, "cpu", conv3x3=bad)
    assert [n for n, _ in enc.named_modules()] == before and isinstance(enc.block0[2], nn.BatchNorm2d), "a refused call changed the pair"


def test_stock_is_the_default_and_routes_nothing():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedConvAct
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, conv3x3="stock")
    for a, b in ((e0, e1), (d0, d1)):
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        for (k0, v0), (k1, v1) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k0 == k1 and torch.equal(v0, v1), k0
        for n, c in _folded(a) + _folded(b):
            assert c.conv3x3_pad is None and not [k for k, _ in c.named_buffers() if k.startswith("_npvp_")], n
            assert set(dict(c.named_buffers())) == {"weight", "bias"} and type(c).forward is FoldedConvAct.forward and "forward" not in c.__dict__


@pytest.mark.parametrize("name", CC.AE_CONFIGS)
def test_hip_marks_exactly_the_eligible_convolutions_of_the_configs(name):
    """the five configs' AE sections: every spatial_conv with 64-multiple channels and every ResnetBlock convolution, nothing else - not the
    7 x 7, not the stride-2 convolutions, nothing in the decoder; the state dict does not change"""
    from npvp_amd import trainer
    from npvp_amd.models import Factorized3DConvAttn, ResnetBlock
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    cfg = trainer.load_config(os.path.join(ROOT, "configs", f"config_{name}.yaml"))
    (e0, d0), (e1, d1) = _pair(cfg["AE"], cfg["Dataset"]["img_channels"]), _pair(cfg["AE"], cfg["Dataset"]["img_channels"])
    fuse_frozen_autoencoder(e0, d0, conv3x3="stock")
    fuse_frozen_autoencoder(e1, d1, conv3x3="hip")
    assert list(e0.state_dict()) == list(e1.state_dict()) and list(d0.state_dict()) == list(d1.state_dict())
    want = {}
    for n, m in e1.named_children():
        if isinstance(m, Factorized3DConvAttn) and m.in_channels % 64 == 0:
            want[f"{n}.spatial_conv"] = "zero"
        if isinstance(m, ResnetBlock):
            want[f"{n}.conv_block.0"] = want[f"{n}.conv_block.1"] = "reflect"
    got = {n: c.conv3x3_pad for n, c in _folded(e1) if c.conv3x3_pad is not None}
    assert got == want and len(want) >= 2 * cfg["AE"]["num_res_blocks"] + 1, (got, want)
    for n, c in _folded(e1):
        if n in want:
            assert tuple(c.weight.shape[2:]) == (3, 3) and tuple(c.stride) == (1, 1) and c.weight.shape[0] % 64 == 0 and c.weight.shape[1] % 64 == 0
            assert "_npvp_planes" in dict(c.named_buffers(recurse=False)) or hasattr(c, "_npvp_planes")
        else:
            assert tuple(c.weight.shape[2:]) == (7, 7) or tuple(c.stride) == (2, 2) or c.weight.shape[0] % 64 or c.weight.shape[1] % 64, n
    assert all(c.conv3x3_pad is None for _, c in _folded(d1)) and len(_folded(d1)) == cfg["AE"]["n_downsampling"] + 1
    for (k0, v0), (k1, v1) in zip(e0.state_dict().items(), e1.state_dict().items()):
        assert torch.equal(v0, v1), k0


def test_hip_leaves_replication_padding_and_small_channel_counts_on_stock():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    enc, dec = _pair(dict(AE_SMALL, ngf=64, learn_3d=False), padding_type="replicate")
    fuse_frozen_autoencoder(enc, dec, conv3x3="hip")
    marks = {n: c.conv3x3_pad for n, c in _folded(enc)}
    assert marks["res_conv_0.conv_block.0"] is None and marks["res_conv_0.conv_block.1"] is None
    assert isinstance(enc.res_conv_0.conv_block[0].pad, nn.ReplicationPad2d)
    assert marks["block2_3dConvAttn.spatial_conv"] == "zero" and marks["res_3dConvAttn_0.spatial_conv"] == "zero"
    enc, dec = _pair(dict(AE_SMALL, ngf=64, learn_3d=False), padding_type="zero")
    fuse_frozen_autoencoder(enc, dec, conv3x3="hip")
    assert {n: c.conv3x3_pad for n, c in _folded(enc)}["res_conv_0.conv_block.1"] == "zero"
    enc, dec = _pair(dict(AE_SMALL, ngf=16, learn_3d=False))         # channels 32 and 64
    fuse_frozen_autoencoder(enc, dec, conv3x3="hip")
    marks = {n: c.conv3x3_pad for n, c in _folded(enc)}
    assert marks["block2_3dConvAttn.spatial_conv"] is None and marks["res_3dConvAttn_0.spatial_conv"] == "zero"


def test_routed_forward_keeps_stock_for_other_inputs_and_refuses_grad(monkeypatch):
    """on CPU tensors: NCHW memory runs the stock forward itself (the same bits, no op of the HIP route called); a channels-last input
    that requires grad is refused and the message names the switch; without a graph the route is taken"""
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    called = []
    monkeypatch.setattr(ops, "bias_act", lambda y, b, act=0, residual=None: (called.append("bias_act"), y)[1])
    monkeypatch.setattr(ops, "conv3x3_planes", lambda w: (called.append("planes"), (torch.zeros(1), torch.zeros(1)))[1])
    monkeypatch.setattr(ops, "conv3x3_packed", lambda x, p, wa, b, pad, act, res: (called.append(("conv3x3", pad, act, res is not None)), x)[1])
    (e0, d0), (e1, d1) = _pair(dict(AE_SMALL, ngf=64, learn_3d=False)), _pair(dict(AE_SMALL, ngf=64, learn_3d=False))
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, conv3x3="hip")
    assert not called, "CPU weights: the planes wait for the first routed forward"
    s, h = e0.res_conv_0, e1.res_conv_0
    x = O.seeded_randn((2, 256, 4, 6), 1)
    with torch.no_grad():
        assert torch.equal(h(x), s(x))
    assert called == ["bias_act"] * 4
    del called[:]
    xcl = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    with pytest.raises(NotImplementedError, match='conv3x3="hip"'):
        h(xcl)
    assert not called
    with torch.no_grad():
        h(xcl)
    assert called == ["planes", ("conv3x3", "reflect", 1, False), "planes", ("conv3x3", "reflect", 0, True)]
