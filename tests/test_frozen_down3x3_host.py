"""CPU: the host side of the frozen encoder's opt-in stride-2 3 x 3 convolution route - the down3x3 switch of to_device_layout /
fuse_frozen_autoencoder and which convolutions it marks, the index function and the planner the kernel calls (exported unchanged by the
C ABI), the refusals of the entry points, and the float64 reference of tests/frozen_down3x3_cases.py against seven wrong restatements."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frozen_down3x3_cases as DC
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
    return {c: (DC.inputs(c), DC.ref64(c)) for c in DC.KERNEL_CASES}


def test_reference_is_the_strided_convolution_of_the_modules(refs):
    """the reference equals what the module stack computes in float64: Conv2d(stride 2, padding 1) -> activation (+ residual)"""
    for case in (DC.KERNEL_CASES[2], DC.KERNEL_CASES[3], DC.KERNEL_CASES[6]):
        Ci, Co, H, W, Fr, act, res = case
        i, ref = refs[case]
        conv = nn.Conv2d(Ci, Co, 3, stride=2, padding=1).double()
        with torch.no_grad():
            conv.weight.copy_(i["w"]); conv.bias.copy_(i["bias"])
            y = conv(i["x"].double())
            y = nn.ReLU()(y) if act == "relu" else y
            if res:
                y = y + i["res"].double()
        assert y.shape == ref.shape == (Fr, Co, DC.out_extent(H), DC.out_extent(W))
        assert DC.rel(y, ref) < 1e-12, case
    i, _ = refs[DC.SCALED_CASE]
    assert 1000 < float(i["x"].abs().max()) and float(i["w"].abs().max()) < 1e-3, "the scaled case is not scaled"


def test_every_mutant_misses_the_bar_by_two_orders(refs):
    worst = {m: 0.0 for m in DC.MUTANTS}
    for case in DC.KERNEL_CASES:
        ins, ref = refs[case]
        for m in DC.MUTANTS:
            mut = DC.ref64(case, m, ins)
            assert mut.shape == ref.shape, (m, DC.case_id(case))
            worst[m] = max(worst[m], DC.rel(mut, ref))
    print(worst)
    for m, e in worst.items():
        assert e > 100 * DC.F16X3_TOL, (m, e)


def test_case_table_reaches_what_it_claims(L):
    ids = [DC.case_id(c) for c in DC.KERNEL_CASES]
    assert len(set(ids)) == len(ids) and len(DC.KERNEL_CASES) == 8
    assert [c[:5] for c in DC.KERNEL_CASES] == [(256, 512, 8, 8, 5), (64, 128, 16, 16, 3), (32, 64, 12, 10, 2), (64, 64, 7, 9, 3),
                                                (128, 256, 1, 1, 3), (64, 128, 2, 3, 70), (256, 512, 30, 40, 1), (128, 256, 32, 32, 1)]
    plans = {}
    for c in DC.KERNEL_CASES:
        out, p = _ints(8)
        assert L.npvp_conv3x3s2_route(c[4], c[2], c[3], c[0], c[1], p) == 0
        plans[c] = list(out)
        assert out[6] * out[7] * c[4] == DC.rows(c)
    assert {p[0] for p in plans.values()} == {1, 2}, "both tile variants are in the table"
    c0, c1, c2, c3, c4, c5, c6, c7 = DC.KERNEL_CASES
    assert DC.rows(c0) == 80 and plans[c0][3] == 1 and c0[4] == 5, "one ragged tile holding five frames"
    assert DC.rows(c1) == 192 and plans[c1][0] == 1 and plans[c1][3] == 2, "a full and a ragged tile, variant 1"
    assert c2[0] == 32 and plans[c2][0] == 2 and c2[2] != c2[3]
    assert c3[2] % 2 == 1 and c3[3] % 2 == 1 and L.npvp_conv3x3s2_src(DC.out_extent(c3[2]) - 1, 2, c3[2]) == -1
    assert c4[2:4] == (1, 1) and plans[c4][6:8] == [1, 1]
    assert plans[c5][6:8] == [1, 2] and 128 // (plans[c5][6] * plans[c5][7]) >= 64 and DC.rows(c5) > 128
    assert c6[5] == "none" and c6[6] and plans[c6][6:8] == [15, 20] and all(not c[6] and c[5] == "relu" for c in DC.KERNEL_CASES if c is not c6)
    assert DC.SCALED_CASE is c7
    assert any(DC.rows(c) % 128 for c in DC.KERNEL_CASES) and any(DC.rows(c) > 128 for c in DC.KERNEL_CASES)


# ------------------------------------------------------------------------------------------------- index function and planner
def test_src_is_the_index_map_of_functional_pad_and_stride_two_slicing(L):
    """exhaustive: every extent 1..9, every output coordinate, every tap"""
    n = 0
    for extent in range(1, 10):
        want = DC.expected_src(extent)
        assert len(want) == DC.out_extent(extent)
        for o in range(len(want)):
            for tap in range(3):
                assert L.npvp_conv3x3s2_src(o, tap, extent) == want[o][tap], (extent, o, tap)
                n += 1
    assert n == 3 * sum((e + 1) // 2 for e in range(1, 10))
    assert [L.npvp_conv3x3s2_src(0, t, 1) for t in range(3)] == [-1, 0, -1]
    assert [L.npvp_conv3x3s2_src(2, t, 5) for t in range(3)] == [3, 4, -1], "odd extent: the last output's tap 2 is outside"
    assert [L.npvp_conv3x3s2_src(2, t, 6) for t in range(3)] == [3, 4, 5]


def test_src_refuses_what_is_outside_its_domain(L):
    for args in ((0, 3, 4), (0, -1, 4), (2, 0, 4), (3, 0, 5), (-1, 0, 4), (0, 0, 0), (1, 1, 1)):
        assert L.npvp_conv3x3s2_src(*args) == -2, args


def test_output_extents_are_conv2ds(L):
    out, p = _ints(8)
    w = torch.zeros(1, 1, 3, 3)
    for H in range(1, 10):
        for W in range(1, 10):
            assert L.npvp_conv3x3s2_route(2, H, W, 32, 64, p) == 0
            assert (out[6], out[7]) == tuple(F.conv2d(torch.zeros(1, 1, H, W), w, stride=2, padding=1).shape[2:]), (H, W)
            assert out[3] == -(-2 * out[6] * out[7] // 128) and out[5] == out[3] * out[4]


@pytest.mark.parametrize("case", DC.KERNEL_CASES, ids=DC.case_id)
def test_the_planners_tiles_are_a_partition(L, case):
    """every (row, column) of the [F Ho Wo][C_out] output belongs to exactly one workgroup of the plan"""
    Ci, Co, H, W, Fr = case[:5]
    out, p = _ints(8)
    assert L.npvp_conv3x3s2_route(Fr, H, W, Ci, Co, p) == 0
    variant, bm, bn, tm, tn, grid, Ho, Wo = list(out)
    M = Fr * Ho * Wo
    assert (variant, bn) == ((1, 128) if Co % 128 == 0 else (2, 64)) and bm == 128 and M == DC.rows(case)
    assert tm == -(-M // bm) and tn == Co // bn and grid == tm * tn
    count = torch.zeros(M, Co, dtype=torch.int32)
    t4, p4 = _ints(4)
    for b in range(grid):
        assert L.npvp_conv3x3s2_tile(Fr, H, W, Ci, Co, b, p4) == 0
        m0, m1, n0, n1 = list(t4)
        assert 0 <= m0 < m1 <= M and m1 - m0 <= bm and 0 <= n0 < n1 <= Co and n1 - n0 == bn
        count[m0:m1, n0:n1] += 1
    assert int(count.min()) == 1 and int(count.max()) == 1
    for bad in (-1, grid):
        assert L.npvp_conv3x3s2_tile(Fr, H, W, Ci, Co, bad, p4) == -1


def test_entry_points_are_declared_and_refuse_on_the_host(L):
    from npvp_amd import _lib
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    for name in ("npvp_conv3x3s2_planes_bytes", "npvp_conv3x3s2_planes", "npvp_conv3x3s2_f16", "npvp_conv3x3s2_route",
                 "npvp_conv3x3s2_tile", "npvp_conv3x3s2_src"):
        assert name in protos and hasattr(L._cdll, name), name
    assert protos["npvp_conv3x3s2_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_conv3x3s2_f16"][1]) == 17
    assert L.npvp_conv3x3s2_planes_bytes(32, 64) == 2 * 2 * 9 * 32 * 64 and L.npvp_conv3x3s2_planes_bytes(128, 256) == 2 * 2 * 9 * 128 * 256
    assert L.npvp_conv3x3s2_planes_bytes(48, 64) == -1 and L.npvp_conv3x3s2_planes_bytes(32, 32) == -1
    out, p = _ints(8)
    for shape in ((1, 8, 8, 48, 128), (1, 8, 8, 128, 32), (0, 8, 8, 64, 64), (1, 0, 8, 64, 64), (1, 8, 0, 64, 64),
                  (1 << 20, 128, 128, 64, 64)):
        assert L.npvp_conv3x3s2_route(*shape, p) == -1, shape
    assert L.npvp_conv3x3s2_route((1 << 19) - 1, 128, 128, 64, 64, p) == 0, "F Ho Wo just below 2^31 is taken"

    def args(**kw):
        a = dict(x=4096, planes=8192, bias=12288, res=None, y=16384, F=1, H=4, W=4, Ci=32, Co=64, act=1, xa=20480, wa=24576, ya=None,
                 ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)
    n0 = L.npvp_launch_count()
    for kw, what in ((dict(x=None), b"non-null"), (dict(planes=None), b"non-null"), (dict(bias=None), b"non-null"),
                     (dict(y=None), b"non-null"), (dict(xa=None), b"non-null"), (dict(wa=None), b"non-null"),
                     (dict(Ci=48), b"C_in a multiple of 32"), (dict(Co=32), b"C_out a multiple of 64"), (dict(F=0), b"F, H, W >= 1"),
                     (dict(H=0), b"F, H, W >= 1"), (dict(W=0), b"F, H, W >= 1"), (dict(F=1 << 20, H=128, W=128), b"F * Ho * Wo below 2^31"),
                     (dict(act=4), b"act in 0..3"), (dict(act=-1), b"act in 0..3"), (dict(y=16388), b"16-byte aligned"),
                     (dict(x=4100), b"16-byte aligned"), (dict(res=16392), b"16-byte aligned"), (dict(planes=8200), b"16-byte aligned")):
        assert L.npvp_conv3x3s2_f16(*args(**kw)) == -1, kw
        assert what in L.npvp_last_error() and b"conv3x3s2" in L.npvp_last_error(), (kw, L.npvp_last_error())
    assert L.npvp_conv3x3s2_planes(None, 64, 64, 8192, 4096, None) == -1 and b"non-null" in L.npvp_last_error()
    assert L.npvp_conv3x3s2_planes(4096, 48, 64, 8192, 4096, None) == -1 and b"multiple of 32" in L.npvp_last_error()
    assert L.npvp_conv3x3s2_planes(4096, 32, 96, 8192, 4096, None) == -1 and L.npvp_conv3x3s2_planes(4100, 32, 64, 8192, 4096, None) == -1
    # the stride-1 entry points keep their 64-multiple rule and their texts
    o6, p6 = _ints(6)
    assert L.npvp_conv3x3_planes_bytes(96, 128) == -1 and L.npvp_conv3x3_planes_bytes(32, 64) == -1 and L.npvp_conv3x3_planes_bytes(64, 32) == -1
    assert L.npvp_conv3x3_route(1, 8, 8, 96, 128, p6) == -1 and L.npvp_conv3x3_route(1, 8, 8, 32, 64, p6) == -1
    assert L.npvp_conv3x3_route(1, 8, 8, 128, 32, p6) == -1
    assert L.npvp_conv3x3_planes(4096, 96, 64, 8192, 4096, None) == -1 and b"multiples of 64" in L.npvp_last_error()
    assert L.npvp_conv3x3_planes(4096, 64, 32, 8192, 4096, None) == -1 and b"multiples of 64" in L.npvp_last_error()
    s1 = (4096, 8192, 12288, None, 16384, 1, 4, 4)
    for Ci, Co in ((96, 64), (32, 64), (64, 32)):
        assert L.npvp_conv3x3_f16(*s1, Ci, Co, 0, 1, 20480, 24576, None, None, 0, None) == -1 and b"multiples of 64" in L.npvp_last_error()
    assert L.npvp_launch_count() == n0, "a refused call launched something"


# ------------------------------------------------------------------------------------------------------------------ the switch
def _pair(AE=AE_SMALL, ci=1):
    import npvp_amd
    enc, dec = npvp_amd.build_frozen_autoencoder(AE, ci)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), 811)
    return enc, dec


def _folded(m):
    from npvp_amd.models.ResNetAutoEncoder import FoldedConvAct
    return [(n, c) for n, c in m.named_modules() if isinstance(c, FoldedConvAct)]


def test_the_switch_refuses_unknown_values_by_name():
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, CONV3X3_ROUTES, DOWN3X3_ROUTES
    assert DOWN3X3_ROUTES == ("stock", "hip") and CONV3X3_ROUTES == ("stock", "hip")
    enc, dec = _pair()
    before = [n for n, _ in enc.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="down3x3=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, down3x3=bad)
        with pytest.raises(ValueError, match="down3x3="):
            npvp_amd.to_device_layout(enc, dec, "cpu", down3x3=bad)
        with pytest.raises(ValueError, match="down3x3="):
            fuse_frozen_autoencoder(enc, dec, attn2d="hip", conv3x3="hip", down3x3=bad)
    assert [n for n, _ in enc.named_modules()] == before and isinstance(enc.block1[1], nn.BatchNorm2d), "a refused call changed the pair"


def test_stock_is_the_default_and_routes_nothing():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedConvAct
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, down3x3="stock")
    for a, b in ((e0, e1), (d0, d1)):
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        for (k0, v0), (k1, v1) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k0 == k1 and torch.equal(v0, v1), k0
        for n, c in _folded(a) + _folded(b):
            assert c.down3x3 is False and c.conv3x3_pad is None and not [k for k, _ in c.named_buffers() if k.startswith("_npvp_")], n
            assert set(dict(c.named_buffers())) == {"weight", "bias"} and type(c).forward is FoldedConvAct.forward and "forward" not in c.__dict__


@pytest.mark.parametrize("name", DC.AE_CONFIGS)
def test_hip_marks_exactly_the_downsampling_convolutions_of_the_configs(name):
    """the five configs' AE sections: block1 and every block{i}_conv, nothing else - not the 7 x 7, no stride-1 convolution, nothing in the
    decoder; the state dict does not change; conv3x3="hip" alone still marks no stride-2 convolution"""
    from npvp_amd import trainer
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    cfg = trainer.load_config(os.path.join(ROOT, "configs", f"config_{name}.yaml"))
    AE, ch = cfg["AE"], cfg["Dataset"]["img_channels"]
    (e0, d0), (e1, d1), (e2, d2), (e3, d3) = _pair(AE, ch), _pair(AE, ch), _pair(AE, ch), _pair(AE, ch)
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, down3x3="hip")
    fuse_frozen_autoencoder(e2, d2, conv3x3="hip")
    fuse_frozen_autoencoder(e3, d3, attn2d="hip", conv3x3="hip", down3x3="hip")
    assert list(e0.state_dict()) == list(e1.state_dict()) and list(d0.state_dict()) == list(d1.state_dict())
    want = {"block1.0"} | {f"block{i + 1}_conv.0" for i in range(1, AE["n_downsampling"])}
    assert len(want) == AE["n_downsampling"]
    assert {n for n, c in _folded(e1) if c.down3x3} == want
    for n, c in _folded(e1):
        assert c.conv3x3_pad is None
        if n in want:
            assert tuple(c.weight.shape[2:]) == (3, 3) and tuple(c.stride) == (2, 2) and c.weight.shape[1] % 32 == 0 and c.weight.shape[0] % 64 == 0
            assert c.weight.shape[0] == 2 * c.weight.shape[1] and c.act == 1 and c.pad is None
            assert "_npvp_planes" in c._buffers and "_npvp_planes" not in c.state_dict()
        else:
            assert tuple(c.stride) == (1, 1) and "_npvp_planes" not in c._buffers, n
    assert all(not c.down3x3 and c.conv3x3_pad is None for _, c in _folded(d1)) and len(_folded(d1)) == AE["n_downsampling"] + 1
    for (k0, v0), (k1, v1) in zip(list(e0.state_dict().items()) + list(d0.state_dict().items()),
                                  list(e1.state_dict().items()) + list(d1.state_dict().items())):
        assert k0 == k1 and torch.equal(v0, v1), k0
    # the switches are independent
    assert not [n for n, c in _folded(e2) if c.down3x3] and all(tuple(c.stride) == (1, 1) for _, c in _folded(e2) if c.conv3x3_pad)
    assert {n for n, c in _folded(e3) if c.down3x3} == want
    assert {n for n, c in _folded(e3) if c.conv3x3_pad} == {n for n, c in _folded(e2) if c.conv3x3_pad}
    assert not [n for n, c in _folded(e3) if c.down3x3 and c.conv3x3_pad]


def test_hip_routes_only_channel_counts_that_pass_the_rule():
    """ngf = 16: block1 is 16 -> 32 (refused twice over), block2_conv 32 -> 64 and block3_conv 64 -> 128 pass"""
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    enc, dec = _pair(dict(AE_SMALL, ngf=16, n_downsampling=3, learn_3d=False))
    fuse_frozen_autoencoder(enc, dec, down3x3="hip")
    marks = {n: c.down3x3 for n, c in _folded(enc) if tuple(c.stride) == (2, 2)}
    assert marks == {"block1.0": False, "block2_conv.0": True, "block3_conv.0": True}
    assert not any(c.down3x3 for n, c in _folded(enc) if tuple(c.stride) != (2, 2)) and not any(c.down3x3 for _, c in _folded(dec))


def test_routed_forward_keeps_stock_for_other_inputs_and_refuses_grad(monkeypatch):
    """on CPU tensors: NCHW memory runs the stock forward itself (the same bits, no op of the HIP route called); a channels-last input
    that requires grad is refused and the message names the switch; without a graph the route is taken with the module's activation"""
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    called = []
    monkeypatch.setattr(ops, "bias_act", lambda y, b, act=0, residual=None: (called.append("bias_act"), y)[1])
    monkeypatch.setattr(ops, "conv3x3s2_planes", lambda w: (called.append("planes"), (torch.zeros(1), torch.zeros(1)))[1])
    monkeypatch.setattr(ops, "conv3x3s2_packed", lambda x, p, wa, b, act, res: (called.append(("down3x3", act, res is not None)), x)[1])
    monkeypatch.setattr(ops, "conv3x3_packed", lambda *a, **k: called.append("conv3x3"))
    (e0, d0), (e1, d1) = _pair(dict(AE_SMALL, ngf=64, learn_3d=False)), _pair(dict(AE_SMALL, ngf=64, learn_3d=False))
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, down3x3="hip")
    assert not called, "CPU weights: the planes wait for the first routed forward"
    s, h = e0.block2_conv, e1.block2_conv
    assert h[0].down3x3 and h[0]._npvp_planes is None
    x = O.seeded_randn((2, 128, 4, 6), 1)
    with torch.no_grad():
        y = h(x)
        assert y.shape == (2, 256, 2, 3) and torch.equal(y, s(x))
    assert called == ["bias_act"] * 2
    del called[:]
    xcl = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    with pytest.raises(NotImplementedError, match='down3x3="hip"'):
        h(xcl)
    assert not called
    with torch.no_grad():
        h(xcl)
    assert called == ["planes", ("down3x3", 1, False)]
