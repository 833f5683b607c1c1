"""CPU: the host side of the frozen decoder's opt-in transposed 3 x 3 convolution route - the up3x3 switch of to_device_layout /
fuse_frozen_autoencoder and which convolutions it marks, the index functions and the planner the kernel calls (exported unchanged by the
C ABI), the refusals of the entry points, the backward identity the op's autograd node rests on, and the float64 reference of
tests/frozen_up3x3_cases.py against seven wrong restatements."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frozen_up3x3_cases as UC
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
    return {c: (UC.inputs(c), UC.ref64(c)) for c in UC.KERNEL_CASES}


def test_reference_is_the_transposed_convolution_of_the_modules(refs):
    """the reference equals what the module stack computes in float64: ConvTranspose2d(3, 2, 1, output_padding 1) -> activation"""
    for case in (UC.KERNEL_CASES[2], UC.KERNEL_CASES[4], UC.KERNEL_CASES[5]):
        Ci, Co, H, W, Fr, act = case
        i, ref = refs[case]
        conv = nn.ConvTranspose2d(Ci, Co, 3, stride=2, padding=1, output_padding=1).double()
        with torch.no_grad():
            conv.weight.copy_(i["w"]); conv.bias.copy_(i["bias"])
            y = UC.act64(conv(i["x"].double()), act)
        assert y.shape == ref.shape == (Fr, Co, 2 * H, 2 * W)
        assert UC.rel(y, ref) < 1e-12, case
    i, _ = refs[UC.SCALED_CASE]
    assert 1000 < float(i["x"].abs().max()) and float(i["w"].abs().max()) < 1e-2, "the scaled case is not scaled"


def test_every_mutant_misses_the_bar_by_two_orders(refs):
    worst = {m: 0.0 for m in UC.MUTANTS}
    for case in UC.KERNEL_CASES:
        ins, ref = refs[case]
        for m in UC.MUTANTS:
            mut = UC.ref64(case, m, ins)
            assert mut.shape == ref.shape, (m, UC.case_id(case))
            worst[m] = max(worst[m], UC.rel(mut, ref))
    print(worst)
    for m, e in worst.items():
        assert e > 100 * UC.F16X3_TOL, (m, e)


def test_case_table_reaches_what_it_claims(L):
    ids = [UC.case_id(c) for c in UC.KERNEL_CASES]
    assert len(set(ids)) == len(ids)
    assert UC.KERNEL_CASES == [(512, 256, 8, 8, 5, "relu"), (64, 64, 1, 1, 3, "relu"), (128, 64, 3, 5, 2, "relu"), (256, 128, 2, 3, 70, "relu"),
                               (32, 64, 4, 6, 3, "none"), (256, 128, 15, 20, 1, "sigmoid"), (128, 128, 16, 16, 1, "relu")]
    plans = {}
    for c in UC.KERNEL_CASES:
        out, p = _ints(8)
        assert L.npvp_convt3x3s2_route(c[4], c[2], c[3], c[0], c[1], p) == 0
        plans[c] = list(out)
        assert out[6:8] == [2 * c[2], 2 * c[3]] and out[5] == 4 * out[3] * out[4]
    assert {p[0] for p in plans.values()} == {1, 2}, "both tile variants are in the table"
    c0, c1, c2, c3, c4, c5, c6 = UC.KERNEL_CASES
    assert UC.rows(c0) == 320 and plans[c0][3] == 3 and 9 * c0[0] // 32 == 144, "two full tiles and a ragged one per class, long K"
    assert c1[2:4] == (1, 1) and plans[c1][0] == 2 and L.npvp_convt3x3s2_src(0, 1, 1, 1) == -1
    assert c2[2] % 2 == 1 and c2[3] % 2 == 1 and c2[2] != c2[3]
    assert 128 // (c3[2] * c3[3]) >= 20 and UC.rows(c3) > 128
    assert c4[0] == 32 and c4[5] == "none"
    assert c5[2:4] == (15, 20) and c5[5] == "sigmoid"
    assert UC.SCALED_CASE is c6
    from npvp_amd import ops
    assert all(ops.convt3x3s2_takes(c[0], c[1]) for c, _ in UC.GRAD_CASES) and len(UC.GRAD_CASES) == 3
    assert [a for _, a in UC.GRAD_CASES].count("none") == 1 and all(c in UC.KERNEL_CASES for c, _ in UC.GRAD_CASES)


# ------------------------------------------------------------------------------------------------ index functions and planner
def test_index_functions_are_the_index_map_of_conv_transpose1d(L):
    """exhaustive: every extent 1..9, every input-grid position, both parities, every tap - against one-hot conv_transpose1d calls"""
    assert [L.npvp_convt3x3s2_ntaps(p) for p in (0, 1)] == [1, 2]
    assert L.npvp_convt3x3s2_tap(0, 0) == 1 and [L.npvp_convt3x3s2_tap(1, t) for t in (0, 1)] == [2, 0]
    n = 0
    for extent in range(1, 10):
        want = UC.expected_taps(extent)
        assert len(want) == 2 * extent
        for i in range(extent):
            for parity in (0, 1):
                got = set()
                for t in range(L.npvp_convt3x3s2_ntaps(parity)):
                    s = L.npvp_convt3x3s2_src(i, parity, t, extent)
                    assert s == -1 or 0 <= s < extent, (extent, i, parity, t, s)
                    if s >= 0:
                        got.add((L.npvp_convt3x3s2_tap(parity, t), s))
                    n += 1
                assert got == want[2 * i + parity], (extent, i, parity)
    assert n == 3 * sum(range(1, 10))
    assert L.npvp_convt3x3s2_src(0, 1, 1, 1) == -1 and L.npvp_convt3x3s2_src(3, 1, 1, 5) == 4 and L.npvp_convt3x3s2_src(4, 1, 1, 5) == -1
    assert L.npvp_convt3x3s2_src(4, 1, 0, 5) == 4 and L.npvp_convt3x3s2_src(4, 0, 0, 5) == 4


def test_index_functions_refuse_what_is_outside_their_domain(L):
    for p in (-1, 2):
        assert L.npvp_convt3x3s2_ntaps(p) == -2 and L.npvp_convt3x3s2_tap(p, 0) == -2 and L.npvp_convt3x3s2_src(0, p, 0, 4) == -2
    for args in ((0, 1), (0, -1), (1, 2), (1, -1)):
        assert L.npvp_convt3x3s2_tap(*args) == -2, args
    for args in ((0, 0, 1, 4), (0, 1, 2, 4), (0, 1, -1, 4), (4, 0, 0, 4), (-1, 1, 0, 4), (0, 0, 0, 0)):
        assert L.npvp_convt3x3s2_src(*args) == -2, args


def _restated(L, case, ins):
    """the whole convolution in float64 from the exported index functions alone: classes, taps, source and kernel index"""
    Ci, Co, H, W, Fr, act = case
    x, w = ins["x"].double(), ins["w"].double()
    y = torch.zeros(Fr, Co, 2 * H, 2 * W, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            for th in range(L.npvp_convt3x3s2_ntaps(a)):
                for tw in range(L.npvp_convt3x3s2_ntaps(b)):
                    kh, kw = L.npvp_convt3x3s2_tap(a, th), L.npvp_convt3x3s2_tap(b, tw)
                    for i in range(H):
                        sh = L.npvp_convt3x3s2_src(i, a, th, H)
                        for j in range(W):
                            sw = L.npvp_convt3x3s2_src(j, b, tw, W)
                            if sh >= 0 and sw >= 0:
                                y[:, :, 2 * i + a, 2 * j + b] += x[:, :, sh, sw] @ w[:, :, kh, kw]
    return UC.act64(y + ins["bias"].double().view(1, Co, 1, 1), act)


@pytest.mark.parametrize("case", [UC.KERNEL_CASES[1], UC.KERNEL_CASES[2], UC.KERNEL_CASES[4], (64, 64, 4, 4, 1, "relu")], ids=UC.case_id)
def test_restatement_from_the_index_functions_is_conv_transpose2d(L, case, refs):
    if case in refs:
        ins, ref = refs[case]
    else:
        ins = dict(x=O.seeded_randn((1, 64, 4, 4), 3001), w=O.seeded_randn((64, 64, 3, 3), 3002) / 12, bias=O.seeded_randn((64,), 3003))
        ref = UC.act64(UC.convt64(ins["x"], ins["w"]) + ins["bias"].double().view(1, -1, 1, 1), "relu")
    assert UC.rel(_restated(L, case, ins), ref) < 1e-12


def test_restatement_at_kths_odd_grid(L, refs):
    """15 x 20, 4 output channels of the table's case (the loop above is per pixel)"""
    case = UC.KERNEL_CASES[5]
    ins, ref = refs[case]
    cut = dict(x=ins["x"], w=ins["w"][:, :4].contiguous(), bias=ins["bias"][:4])
    assert UC.rel(_restated(L, case[:1] + (4,) + case[2:], cut), ref[:, :4]) < 1e-12


@pytest.mark.parametrize("case", [c for c, _ in UC.GRAD_CASES], ids=UC.case_id)
def test_input_gradient_is_the_stride_two_convolution_with_the_weight_read_as_conv2d(case, refs):
    """autograd.grad(conv_transpose2d(x, w, None, 2, 1, 1), x, g) == conv2d(g, w, None, 2, 1) with w [C_in][C_out][3][3] read as a Conv2d
    weight [out = C_in][in = C_out][3][3]: what the op's backward launches"""
    Ci, Co, H, W, Fr, act = case
    ins, _ = refs[case]
    x = ins["x"].double().requires_grad_()
    w = ins["w"].double()
    g = O.seeded_randn((Fr, Co, 2 * H, 2 * W), 3010).double()
    (dx,) = torch.autograd.grad(F.conv_transpose2d(x, w, None, 2, 1, 1), x, g)
    want = F.conv2d(g, w, None, 2, 1)
    assert want.shape == dx.shape == (Fr, Ci, H, W) and UC.rel(want, dx) < 1e-12


@pytest.mark.parametrize("case", UC.KERNEL_CASES, ids=UC.case_id)
def test_the_planners_tiles_are_a_partition(L, case):
    """every (class, row, column) of the four [F H W][C_out] class matrices - every output element - belongs to exactly one workgroup of
    the plan, and the 4-tap class's workgroups come first, the 1-tap class's last"""
    Ci, Co, H, W, Fr = case[:5]
    out, p = _ints(8)
    assert L.npvp_convt3x3s2_route(Fr, H, W, Ci, Co, p) == 0
    variant, bm, bn, tm, tn, grid, Ho, Wo = list(out)
    M = Fr * H * W
    assert (variant, bn) == ((1, 128) if Co % 128 == 0 else (2, 64)) and bm == 128 and M == UC.rows(case) and (Ho, Wo) == (2 * H, 2 * W)
    assert tm == -(-M // bm) and tn == Co // bn and grid == 4 * tm * tn
    count = torch.zeros(2, 2, M, Co, dtype=torch.int32)
    t6, p6 = _ints(6)
    taps = []
    for blk in range(grid):
        assert L.npvp_convt3x3s2_tile(Fr, H, W, Ci, Co, blk, p6) == 0
        a, b, m0, m1, n0, n1 = list(t6)
        assert a in (0, 1) and b in (0, 1) and 0 <= m0 < m1 <= M and m1 - m0 <= bm and 0 <= n0 < n1 <= Co and n1 - n0 == bn
        count[a, b, m0:m1, n0:n1] += 1
        taps.append(L.npvp_convt3x3s2_ntaps(a) * L.npvp_convt3x3s2_ntaps(b))
    assert int(count.min()) == 1 and int(count.max()) == 1
    assert taps == sorted(taps, reverse=True) and taps[:tm * tn] == [4] * (tm * tn) and taps[-tm * tn:] == [1] * (tm * tn)
    # the pixel a row is stored at: (class, row) -> output pixel is a bijection onto the F x 2H x 2W output
    pix = torch.zeros(Fr * 4 * H * W, dtype=torch.int32)
    m = torch.arange(M)
    f, i, j = m // (H * W), (m % (H * W)) // W, m % W
    for a in (0, 1):
        for b in (0, 1):
            pix[(f * 2 * H + 2 * i + a) * 2 * W + 2 * j + b] += 1
    assert int(pix.min()) == 1 and int(pix.max()) == 1
    for bad in (-1, grid):
        assert L.npvp_convt3x3s2_tile(Fr, H, W, Ci, Co, bad, p6) == -1


def test_entry_points_are_declared_and_refuse_on_the_host(L):
    from npvp_amd import _lib
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    for name in ("npvp_convt3x3s2_planes_bytes", "npvp_convt3x3s2_planes", "npvp_convt3x3s2_f16", "npvp_convt3x3s2_route",
                 "npvp_convt3x3s2_tile", "npvp_convt3x3s2_src", "npvp_convt3x3s2_tap", "npvp_convt3x3s2_ntaps"):
        assert name in protos and hasattr(L._cdll, name), name
    assert protos["npvp_convt3x3s2_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_convt3x3s2_f16"][1]) == 16
    assert L.npvp_convt3x3s2_planes_bytes(32, 64) == 2 * 2 * 9 * 32 * 64 and L.npvp_convt3x3s2_planes_bytes(512, 256) == 2 * 2 * 9 * 512 * 256
    assert L.npvp_convt3x3s2_planes_bytes(48, 64) == -1 and L.npvp_convt3x3s2_planes_bytes(64, 32) == -1
    out, p = _ints(8)
    for shape in ((1, 8, 8, 48, 128), (1, 8, 8, 128, 32), (0, 8, 8, 64, 64), (1, 0, 8, 64, 64), (1, 8, 0, 64, 64),
                  (1 << 15, 128, 128, 64, 64)):
        assert L.npvp_convt3x3s2_route(*shape, p) == -1, shape
    assert L.npvp_convt3x3s2_route((1 << 15) - 1, 128, 128, 64, 64, p) == 0, "F 2H 2W just below 2^31 is taken"

    def args(**kw):
        a = dict(x=4096, planes=8192, bias=12288, y=16384, F=1, H=4, W=4, Ci=32, Co=64, act=1, xa=20480, wa=24576, ya=None, ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)
    n0 = L.npvp_launch_count()
    for kw, what in ((dict(x=None), b"non-null"), (dict(planes=None), b"non-null"), (dict(bias=None), b"non-null"),
                     (dict(y=None), b"non-null"), (dict(xa=None), b"non-null"), (dict(wa=None), b"non-null"),
                     (dict(Ci=48), b"C_in a multiple of 32"), (dict(Co=32), b"C_out a multiple of 64"), (dict(F=0), b"F, H, W >= 1"),
                     (dict(H=0), b"F, H, W >= 1"), (dict(W=0), b"F, H, W >= 1"), (dict(F=1 << 15, H=128, W=128), b"F * 2H * 2W below 2^31"),
                     (dict(act=4), b"act in 0..3"), (dict(act=-1), b"act in 0..3"), (dict(y=16388), b"16-byte aligned"),
                     (dict(x=4100), b"16-byte aligned"), (dict(planes=8200), b"16-byte aligned")):
        assert L.npvp_convt3x3s2_f16(*args(**kw)) == -1, kw
        assert what in L.npvp_last_error() and b"convt3x3s2" in L.npvp_last_error(), (kw, L.npvp_last_error())
    assert L.npvp_convt3x3s2_planes(None, 64, 64, 8192, 4096, None) == -1 and b"non-null" in L.npvp_last_error()
    assert L.npvp_convt3x3s2_planes(4096, 48, 64, 8192, 4096, None) == -1 and b"multiple of 32" in L.npvp_last_error()
    assert L.npvp_convt3x3s2_planes(4096, 32, 96, 8192, 4096, None) == -1 and L.npvp_convt3x3s2_planes(4100, 32, 64, 8192, 4096, None) == -1
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
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, UP3X3_ROUTES
    assert UP3X3_ROUTES == ("stock", "hip")
    enc, dec = _pair()
    before = [n for n, _ in dec.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="up3x3=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, up3x3=bad)
        with pytest.raises(ValueError, match="up3x3="):
            npvp_amd.to_device_layout(enc, dec, "cpu", up3x3=bad)
        with pytest.raises(ValueError, match="up3x3="):
            fuse_frozen_autoencoder(enc, dec, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3=bad)
    assert [n for n, _ in dec.named_modules()] == before and isinstance(dec.model[1], nn.BatchNorm2d), "a refused call changed the pair"


def test_stock_is_the_default_and_routes_nothing():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedConvAct, ResnetDecoder
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, up3x3="stock")
    for a, b in ((e0, e1), (d0, d1)):
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        for (k0, v0), (k1, v1) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k0 == k1 and torch.equal(v0, v1), k0
        for n, c in _folded(a) + _folded(b):
            assert c.up3x3 is False and not [k for k, _ in c.named_buffers() if k.startswith("_npvp_")], n
            assert set(dict(c.named_buffers())) == {"weight", "bias"} and type(c).forward is FoldedConvAct.forward and "forward" not in c.__dict__
    for d in (d0, d1):
        assert d.up3x3 is False and "up3x3" not in d.__dict__ and type(d).forward is ResnetDecoder.forward


@pytest.mark.parametrize("name", UC.AE_CONFIGS)
def test_hip_marks_exactly_the_upsampling_convolutions_of_the_configs(name):
    """the five configs' AE sections: every ConvTranspose2d of the decoder with 64-multiple channels - all of an ngf = 64 decoder, all
    but the last (64 -> 32) of an ngf = 32 one -, never the 7 x 7 tail, nothing in the encoder; the state dict does not change; the
    other three switches mark no decoder module"""
    from npvp_amd import trainer
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    cfg = trainer.load_config(os.path.join(ROOT, "configs", f"config_{name}.yaml"))
    AE, ch = cfg["AE"], cfg["Dataset"]["img_channels"]
    (e0, d0), (e1, d1), (e2, d2), (e3, d3) = _pair(AE, ch), _pair(AE, ch), _pair(AE, ch), _pair(AE, ch)
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, up3x3="hip")
    fuse_frozen_autoencoder(e2, d2, attn2d="hip", conv3x3="hip", down3x3="hip")
    fuse_frozen_autoencoder(e3, d3, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip")
    assert list(e0.state_dict()) == list(e1.state_dict()) and list(d0.state_dict()) == list(d1.state_dict())
    n_up = AE["n_downsampling"]
    assert len(_folded(d1)) == n_up + 1
    want = {f"model.{i}" for i in range(n_up) if (AE["ngf"] << (n_up - i)) % 64 == 0 and (AE["ngf"] << (n_up - i - 1)) % 64 == 0}
    assert len(want) == (n_up if AE["ngf"] % 64 == 0 else n_up - 1) and AE["ngf"] in (32, 64)
    assert {n for n, c in _folded(d1) if c.up3x3} == want and d1.up3x3 is True and d0.up3x3 is False
    for n, c in _folded(d1):
        if n in want:
            assert c.transposed and tuple(c.weight.shape[2:]) == (3, 3) and tuple(c.stride) == (2, 2) and tuple(c.output_padding) == (1, 1)
            assert c.weight.shape[0] == 2 * c.weight.shape[1] and c.weight.shape[1] % 64 == 0 and c.act == 1 and c.pad is None
            for k in c._UP3X3_BUFFERS:
                assert k in c._buffers and k not in c.state_dict()
        else:
            assert "_npvp_planes" not in c._buffers, n
            assert (c.transposed and tuple(c.weight.shape[:2]) == (64, 32)) or (not c.transposed and tuple(c.weight.shape[2:]) == (7, 7)), n
    assert not any(c.up3x3 for _, c in _folded(e1)) and not any("_npvp_" in k for k, _ in e1.named_buffers())
    for (k0, v0), (k1, v1) in zip(list(e0.state_dict().items()) + list(d0.state_dict().items()),
                                  list(e1.state_dict().items()) + list(d1.state_dict().items())):
        assert k0 == k1 and torch.equal(v0, v1), k0
    # the switches are independent
    assert not any(c.up3x3 or c.down3x3 or c.conv3x3_pad for _, c in _folded(d2)) and d2.up3x3 is False
    assert {n for n, c in _folded(d3) if c.up3x3} == want
    assert {n for n, c in _folded(e3) if c.down3x3} == {n for n, c in _folded(e2) if c.down3x3} != set()
    assert {n for n, c in _folded(e3) if c.conv3x3_pad} == {n for n, c in _folded(e2) if c.conv3x3_pad} != set()
    assert not any(c.up3x3 for _, c in _folded(e3)) and not any(c.down3x3 or c.conv3x3_pad for _, c in _folded(d3))


def test_hip_routes_only_channel_counts_that_pass_the_rule():
    """ngf = 32, three upsamplings: 256 -> 128 and 128 -> 64 pass, 64 -> 32 stays stock; ngf = 16: only 128 -> 64"""
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, _up3x3_takes_hip
    enc, dec = _pair(dict(AE_SMALL, ngf=32, n_downsampling=3, learn_3d=False))
    fuse_frozen_autoencoder(enc, dec, up3x3="hip")
    assert {n: c.up3x3 for n, c in _folded(dec)} == {"model.0": True, "model.1": True, "model.2": False, "model.3": False}
    enc, dec = _pair(dict(AE_SMALL, ngf=16, n_downsampling=3, learn_3d=False))
    fuse_frozen_autoencoder(enc, dec, up3x3="hip")
    assert {n: c.up3x3 for n, c in _folded(dec)} == {"model.0": True, "model.1": False, "model.2": False, "model.3": False}
    # a stride-2 forward convolution, a transposed convolution without output_padding, one with another stride: all refused
    from npvp_amd.models.ResNetAutoEncoder import FoldedConvAct
    assert _up3x3_takes_hip(FoldedConvAct(nn.ConvTranspose2d(128, 64, 3, 2, 1, 1)))
    for conv in (nn.Conv2d(128, 64, 3, 2, 1), nn.ConvTranspose2d(128, 64, 3, 2, 1, 0), nn.ConvTranspose2d(128, 64, 3, 1, 1, 0),
                 nn.ConvTranspose2d(128, 64, 4, 2, 1, 0), nn.ConvTranspose2d(128, 32, 3, 2, 1, 1), nn.ConvTranspose2d(96, 64, 3, 2, 1, 1)):
        assert not _up3x3_takes_hip(FoldedConvAct(conv)), conv


def test_stock_remainder_of_a_routed_decoder_keeps_nchw_weights():
    """UP3X3_TAIL = "nchw" (the measured choice): to_device_layout(up3x3="hip") puts the decoder in channels_last, and the modules the
    route does not take - the 64 -> 32 transposed convolution of an ngf = 32 decoder, the 7 x 7 tail - get their weights back in NCHW,
    which is what makes the routed forward copy the frames back once in front of them; under "stock" the decoder stays NCHW"""
    import npvp_amd
    from npvp_amd.models import ResNetAutoEncoder as RAE
    assert RAE.UP3X3_TAIL == "nchw"
    AE = dict(AE_SMALL, ngf=32, n_downsampling=3, learn_3d=False)
    enc, dec = _pair(AE, 3)
    npvp_amd.to_device_layout(enc, dec, "cpu", up3x3="hip")
    assert [m.up3x3 for m in dec.model] == [True, True, False, False]
    for m in dec.model:
        assert m.weight.is_contiguous() == (not m.up3x3), "routed: channels_last as moved; stock remainder: NCHW"
    enc, dec = _pair(AE, 3)
    npvp_amd.to_device_layout(enc, dec, "cpu")
    assert all(m.weight.is_contiguous() for m in dec.model)


def test_routed_forward_keeps_stock_for_other_inputs_and_hands_grad_inputs_to_the_op(monkeypatch):
    """on CPU tensors: NCHW memory at a routed FoldedConvAct runs the stock forward itself (the same bits, no op of the HIP route
    called); a channels-last input goes to the op with the module's activation, whether or not it requires grad (the op is
    differentiable); the routed decoder converts its NCHW input frames to channels-last once"""
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    called = []
    monkeypatch.setattr(ops, "bias_act", lambda y, b, act=0, residual=None: (called.append("bias_act"), y)[1])
    monkeypatch.setattr(ops, "convt3x3s2_planes", lambda w: (called.append("planes"), ops.ConvT3x3Planes(*(torch.zeros(1),) * 5))[1])

    def packed(x, planes, bias, act):
        called.append(("up3x3", act, x.is_contiguous(memory_format=torch.channels_last), x.requires_grad))
        return F.interpolate(x[:, :bias.shape[0]], scale_factor=2).contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(ops, "convt3x3s2_packed", packed)
    AE = dict(AE_SMALL, ngf=64, learn_3d=False)
    (e0, d0), (e1, d1) = _pair(AE), _pair(AE)
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, up3x3="hip")
    assert not called, "CPU weights: the planes wait for the first routed forward"
    s, h = d0.model[0], d1.model[0]
    assert h.up3x3 and h._npvp_planes is None
    x = O.seeded_randn((2, 256, 4, 6), 1)
    with torch.no_grad():
        y = h(x)
        assert y.shape == (2, 128, 8, 12) and torch.equal(y, s(x))
    assert called == ["bias_act"] * 2
    del called[:]
    xcl = x.contiguous(memory_format=torch.channels_last).requires_grad_()
    h(xcl)
    assert called == ["planes", ("up3x3", 1, True, True)]
    del called[:]
    with torch.no_grad():
        out = d1(x.view(1, 2, 256, 4, 6))
    assert out.shape == (1, 2, 1, 16, 24)
    assert called == [("up3x3", 1, True, False), "planes", ("up3x3", 1, True, False), "bias_act"]
