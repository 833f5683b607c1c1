"""CPU: the host side of the frozen encoder's opt-in 7 x 7 stem route - the stem7x7 switch of to_device_layout /
fuse_frozen_autoencoder and which convolution it marks, the K index and the planner the kernel calls (exported unchanged by the C ABI),
the refusals of the entry points, and the float64 reference of tests/frozen_stem7x7_cases.py against wrong restatements.

A wrong restatement is held to the bar on every case where it is a different statement at all (APPLIES): `frames_stacked` is the reference
itself on a single frame, `act_before_bias` where the activation is none, `planar_read_as_channels_last` where C_in = 1.  Every
restatement is caught on at least two cases.  No case is left out for more than two restatements - except (1, 32, 7, 130, 1, none), the
one case of the table that is one frame AND one channel AND has no activation: all three of the above are the reference itself there by
construction (test_every_wrong_restatement_misses_the_bar names it and holds it to exactly those three)."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn

import frozen_stem7x7_cases as SC
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE_SMALL = dict(ngf=32, n_downsampling=2, num_res_blocks=1, learn_3d=True, out_layer='Tanh')
APPLIES = {"frames_stacked": lambda c: c[4] > 1, "act_before_bias": lambda c: c[5] != "none",
           "planar_read_as_channels_last": lambda c: c[0] > 1}
ONE_FRAME_ONE_CHANNEL_NO_ACT = (1, 32, 7, 130, 1, "none")


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def _ints(n, fill=0):
    buf = (ctypes.c_int * n)(*([fill] * n))
    return buf, ctypes.addressof(buf)


# ------------------------------------------------------------------------------------------------------- the float64 reference
@pytest.fixture(scope="module")
def refs():
    out = {}
    for c in SC.KERNEL_CASES:
        ins = SC.inputs(c)
        out[c] = (ins, SC.ref64(c, ins=ins))
    return out


def test_reference_is_the_module_stack(refs):
    """the reference equals ReflectionPad2d(3) -> Conv2d(C_in, C_out, 7) -> activation in float64"""
    for case in SC.KERNEL_CASES:
        Ci, Co, H, W, Fr, act = case
        i, ref = refs[case]
        seq = nn.Sequential(*([nn.ReflectionPad2d(3), nn.Conv2d(Ci, Co, 7)] + ({"relu": [nn.ReLU()], "none": []}[act]))).double()
        with torch.no_grad():
            seq[1].weight.copy_(i["w"]); seq[1].bias.copy_(i["bias"])
            y = seq(i["x"].double())
        assert y.shape == ref.shape == (Fr, Co, H, W)
        assert SC.rel(y, ref) < 1e-12, case
    i, _ = refs[SC.SCALED_CASE]
    assert 1000 < float(i["x"].abs().max()) and float(i["w"].abs().max()) < 1e-2, "the scaled case is not scaled"
    _, ref = refs[SC.KERNEL_CASES[3]]
    assert float(ref.min()) < -1 and float(ref.max()) > 1, "the signed case is not signed"


def test_case_table_is_the_issues(L):
    assert SC.KERNEL_CASES == [(1, 64, 64, 64, 1, "relu"), (3, 64, 4, 4, 9, "relu"), (3, 32, 5, 9, 3, "relu"), (1, 32, 7, 130, 1, "none"),
                               (2, 64, 4, 7, 5, "none"), (4, 128, 8, 8, 2, "relu"), (3, 64, 8, 16, 2, "none")]
    assert SC.SCALED_CASE is SC.KERNEL_CASES[6] and len({SC.case_id(c) for c in SC.KERNEL_CASES}) == 7
    assert SC.F16X3_TOL == 1e-5 and SC.BAR == 1e-4
    assert ONE_FRAME_ONE_CHANNEL_NO_ACT in SC.KERNEL_CASES
    assert len(SC.MUTANTS) == 9 and "planar_read_as_channels_last" in SC.MUTANTS
    # every case is inside the kernel's shape rule, and reaches what the table says it reaches
    out, p = _ints(7)
    got = {}
    for case in SC.KERNEL_CASES:
        Ci, Co, H, W, Fr, act = case
        assert Fr >= 1 and H >= 4 and W >= 4 and 1 <= Ci <= 4 and Co % 32 == 0 and 0 < Co <= 4096 and Fr * H * W < 2 ** 31
        assert SC.ACT[act] in (0, 1)
        assert L.npvp_stem7x7_route(Fr, H, W, Ci, Co, p) == 0, case
        got[case] = list(out)
    C = SC.KERNEL_CASES
    assert got[C[1]][3] == 2 and 9 * 16 == 144 and got[C[1]][6] == 5, "a tile of 128 rows spans 8 frames of 16 pixels, the last tile is ragged"
    assert got[C[2]][:3] == [2, 128, 32] and 3 * 5 * 9 == 135 and got[C[2]][3] == 2
    assert 128 % 130 != 0 and got[C[3]][3] == 8 and got[C[3]][0] == 2, "tile boundaries inside image rows"
    assert got[C[4]][6] == 4 and 49 * 2 == 98
    assert got[C[5]][6] == 7 and 49 * 4 % 32 == 4 and got[C[5]][4] == 2, "two column tiles"
    assert 49 * 4 == 196 and L.npvp_stem7x7_planes_bytes(4, 128) == 2 * 224 * 128 * 2
    assert min(c[2] for c in C) == min(c[3] for c in C) == 4


def test_every_wrong_restatement_misses_the_bar(refs):
    seen = {m: 0 for m in SC.MUTANTS}
    left_out = {c: [] for c in SC.KERNEL_CASES}
    for case in SC.KERNEL_CASES:
        ins, ref = refs[case]
        for m in SC.MUTANTS:
            mut = SC.ref64(case, m, ins)
            e = SC.rel(mut, ref)
            print(SC.case_id(case), m, f"{e:.3e}")
            assert mut.shape == ref.shape
            if not APPLIES.get(m, lambda c: True)(case):
                assert e < 1e-12, ("left out, yet a different statement", m, SC.case_id(case), e)
                left_out[case].append(m)
                continue
            assert e > SC.BAR, (m, SC.case_id(case), e)
            seen[m] += 1
    assert all(n >= 2 for n in seen.values()), seen
    for case, ms in left_out.items():
        if case == ONE_FRAME_ONE_CHANNEL_NO_ACT:
            assert ms == ["frames_stacked", "act_before_bias", "planar_read_as_channels_last"], ms
        else:
            assert len(ms) <= 2, (case, ms)


# ------------------------------------------------------------------------------------------------------------------- the K index
@pytest.mark.parametrize("Ci", [1, 2, 3, 4])
def test_k_index_is_the_dense_order(L, Ci):
    want = SC.expected_k(Ci)
    kpad = -(-49 * Ci // 32) * 32
    assert len(want) == 49 * Ci and len(set(want)) == 49 * Ci and kpad == {1: 64, 2: 128, 3: 160, 4: 224}[Ci]
    out, p = _ints(3, 77)
    got = []
    for k in range(kpad):
        rc = L.npvp_stem7x7_k(Ci, k, p)
        if k < 49 * Ci:
            assert rc == 0, k
            got.append(tuple(out))
        else:
            assert rc == 1 and list(out) == [-1, -1, -1], (k, "the rest is padding")
    assert got == want
    assert sorted(got) == sorted((kh, kw, ci) for kh in range(7) for kw in range(7) for ci in range(Ci)), "every (kh, kw, ci) exactly once"
    out, p = _ints(3, 77)
    for bad in ((Ci, -1), (Ci, kpad), (0, 0), (5, 0), (-1, 3)):
        assert L.npvp_stem7x7_k(*bad, p) == -2 and list(out) == [77, 77, 77], bad
    assert L.npvp_stem7x7_k(Ci, 0, None) == -2


def test_planes_restated_from_the_k_index_multiply_like_the_convolution(L, refs):
    """A[m][k] gathered with npvp_tail7x7_src and npvp_stem7x7_k times B[k][n] placed with npvp_stem7x7_k is pad + conv (float64)"""
    case = SC.KERNEL_CASES[2]
    Ci, Co, H, W, Fr, act = case
    ins, ref = refs[case]
    kpad = -(-49 * Ci // 32) * 32
    out, p = _ints(3)
    x, w = ins["x"].double(), ins["w"].double()
    A = torch.zeros(Fr * H * W, kpad, dtype=torch.float64)
    B = torch.zeros(kpad, Co, dtype=torch.float64)
    for k in range(kpad):
        if L.npvp_stem7x7_k(Ci, k, p) != 0:
            continue
        kh, kw, ci = out
        B[k] = w[:, ci, kh, kw]
        sh = torch.tensor([L.npvp_tail7x7_src(h, kh, H) for h in range(H)])
        sw = torch.tensor([L.npvp_tail7x7_src(v, kw, W) for v in range(W)])
        A[:, k] = x[:, ci][:, sh][:, :, sw].reshape(-1)
    y = SC.act64((A @ B).view(Fr, H, W, Co).permute(0, 3, 1, 2) + ins["bias"].double().view(1, Co, 1, 1), act)
    assert SC.rel(y, ref) < 1e-12


# ------------------------------------------------------------------------------------------------------------- plan and tiles
PLAN_SHAPES = [c[:5] for c in SC.KERNEL_CASES] + [(3, 64, 5, w, 1) for w in SC.PLAN_WIDTHS]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tiles_cover_every_row_and_column_once(L, shape):
    Ci, Co, H, W, Fr = shape
    M = Fr * H * W
    out, p = _ints(7)
    assert L.npvp_stem7x7_route(Fr, H, W, Ci, Co, p) == 0
    variant, bm, bn, tm, tn, grid, ksteps = list(out)
    assert (variant, bn) == ((1, 64) if Co % 64 == 0 else (2, 32)) and bm == 128 and tm == -(-M // 128) and tn == Co // bn and grid == tm * tn
    assert ksteps == -(-49 * Ci // 32), "the dense K order: ceil(49 C_in / 32) K-steps"
    assert L.npvp_stem7x7_planes_bytes(Ci, Co) == 2 * (32 * ksteps) * Co * 2, "[2 terms][K_pad / 8][C_out][8] halves"
    count = torch.zeros(M, Co, dtype=torch.int32)
    t4, p4 = _ints(4)
    for blk in range(grid):
        assert L.npvp_stem7x7_tile(Fr, H, W, Ci, Co, blk, p4) == 0
        m0, m1, n0, n1 = list(t4)
        assert 0 <= m0 < m1 <= M and m1 - m0 <= bm and 0 <= n0 < n1 <= Co and n1 - n0 == bn
        count[m0:m1, n0:n1] += 1
    assert int(count.min()) == 1 and int(count.max()) == 1
    t4, p4 = _ints(4, 55)
    for bad in (-1, grid):
        assert L.npvp_stem7x7_tile(Fr, H, W, Ci, Co, bad, p4) == -1 and list(t4) == [55] * 4


# ----------------------------------------------------------------------------------------------------------------- entry points
NAMES = ("npvp_stem7x7_k", "npvp_stem7x7_planes_bytes", "npvp_stem7x7_planes", "npvp_stem7x7_f16", "npvp_stem7x7_route", "npvp_stem7x7_tile")


def test_entry_points_are_declared_and_refuse_on_the_host(L):
    from npvp_amd import _lib
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    for name in NAMES:
        assert name in protos and name in _lib.SIGNATURES and hasattr(L._cdll, name), name
    assert protos["npvp_stem7x7_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_stem7x7_f16"][1]) == 16
    assert protos["npvp_stem7x7_planes"][1][-1] == "npvp_stream_t" and len(protos["npvp_stem7x7_planes"][1]) == 6
    assert L.npvp_stem7x7_planes_bytes(1, 64) == 2 * 64 * 64 * 2 and L.npvp_stem7x7_planes_bytes(3, 32) == 2 * 160 * 32 * 2
    for bad in ((0, 64), (5, 64), (3, 0), (3, 48), (3, 8192), (64, 3)):
        assert L.npvp_stem7x7_planes_bytes(*bad) == -1, bad
    out, p = _ints(7, 55)
    for shape in ((1, 8, 8, 5, 64), (1, 8, 8, 0, 64), (1, 8, 8, 3, 48), (1, 8, 8, 3, 0), (0, 8, 8, 3, 64), (1, 3, 8, 3, 64), (1, 8, 3, 3, 64),
                  (1 << 11, 1 << 10, 1 << 10, 3, 64)):
        assert L.npvp_stem7x7_route(*shape, p) == -1 and L.npvp_stem7x7_tile(*shape, 0, p) == -1, shape
        assert list(out) == [55] * 7, "a refused shape leaves the output untouched"
    assert L.npvp_stem7x7_route((1 << 11) - 1, 1 << 10, 1 << 10, 3, 64, p) == 0, "F H W just below 2^31 is taken"

    def fwd(**kw):
        a = dict(x=4096, planes=8192, bias=12288, y=16384, F=1, H=4, W=4, Ci=3, Co=64, act=1, xa=20480, wa=24576, ya=None, ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)
    n0 = L.npvp_launch_count()
    for kw, what in ((dict(x=None), b"non-null"), (dict(planes=None), b"non-null"), (dict(bias=None), b"non-null"), (dict(y=None), b"non-null"),
                     (dict(xa=None), b"non-null"), (dict(wa=None), b"non-null"), (dict(act=2), b"act 0 (none) or 1 (ReLU)"),
                     (dict(act=3), b"act 0"), (dict(act=-1), b"act 0"), (dict(y=16388), b"16-byte aligned"), (dict(planes=8200), b"16-byte aligned"),
                     (dict(Ci=5), b"1 <= C_in <= 4"), (dict(Ci=0), b"1 <= C_in <= 4"), (dict(Co=48), b"C_out a multiple of 32"),
                     (dict(Co=0), b"C_out a multiple of 32"), (dict(Co=8192), b"up to 4096"), (dict(F=0), b"F >= 1"), (dict(H=3), b"H, W >= 4"),
                     (dict(W=3), b"H, W >= 4"), (dict(F=1 << 11, H=1 << 10, W=1 << 10), b"F * H * W below 2^31")):
        assert L.npvp_stem7x7_f16(*fwd(**kw)) == -1, kw
        assert what in L.npvp_last_error() and b"stem7x7" in L.npvp_last_error(), (kw, L.npvp_last_error())
    fn = L.npvp_stem7x7_planes
    assert fn(None, 3, 64, 8192, 4096, None) == -1 and b"non-null" in L.npvp_last_error()
    assert fn(4096, 3, 64, None, 4096, None) == -1 and fn(4096, 3, 64, 8192, None, None) == -1
    assert fn(4096, 5, 64, 8192, 4096, None) == -1 and b"1 <= C_in <= 4" in L.npvp_last_error()
    assert fn(4096, 3, 48, 8192, 4096, None) == -1 and b"multiple of 32" in L.npvp_last_error()
    assert fn(4100, 3, 64, 8192, 4096, None) == -1 and b"16-byte aligned" in L.npvp_last_error()
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


def test_the_switch_is_the_sixth_keyword_and_refuses_unknown_values_by_name():
    import inspect
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, to_device_layout, STEM7X7_ROUTES
    assert STEM7X7_ROUTES == ("stock", "hip")
    for fn, lead in ((fuse_frozen_autoencoder, 2), (to_device_layout, 3)):
        params = list(inspect.signature(fn).parameters.values())[lead:]
        assert [q.name for q in params] == ["attn2d", "conv3x3", "down3x3", "up3x3", "tail7x7", "stem7x7"], "appended last"
        assert all(q.default == "stock" for q in params)
    enc, dec = _pair()
    before = [n for n, _ in enc.named_modules()] + [n for n, _ in dec.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="stem7x7=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, stem7x7=bad)
        with pytest.raises(ValueError, match="stem7x7="):
            npvp_amd.to_device_layout(enc, dec, "cpu", stem7x7=bad)
        with pytest.raises(ValueError, match="stem7x7="):
            fuse_frozen_autoencoder(enc, dec, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip", tail7x7="hip", stem7x7=bad)
    assert [n for n, _ in enc.named_modules()] + [n for n, _ in dec.named_modules()] == before, "a refused call changed the pair"
    assert isinstance(enc.block0[2], nn.BatchNorm2d) and isinstance(dec.model[1], nn.BatchNorm2d)
    assert all(q.requires_grad is False for q in enc.parameters()), "(frozen by build_frozen_autoencoder, not by the refused call)"


def test_stock_is_the_default_and_routes_nothing():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedConvAct
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, stem7x7="stock")
    for a, b in ((e0, e1), (d0, d1)):
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        for (k0, v0), (k1, v1) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k0 == k1 and torch.equal(v0, v1), k0
        for n, c in _folded(a) + _folded(b):
            assert c.stem7x7 is False and not [k for k, _ in c.named_buffers() if k.startswith("_npvp_")], n
            assert set(dict(c.named_buffers())) == {"weight", "bias"} and type(c).forward is FoldedConvAct.forward and "forward" not in c.__dict__


@pytest.mark.parametrize("name", SC.AE_CONFIGS)
def test_hip_marks_exactly_the_stem_of_the_configs(name):
    """the five configs' AE sections: block0[0] of the encoder and nothing else, nothing in the decoder (its 7 x 7 tail has C_in = ngf and
    C_out = 1 or 3); the state dict does not change; the other five switches do not mark the stem"""
    from npvp_amd import trainer
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, _stem7x7_takes_hip, _tail7x7_takes_hip
    cfg = trainer.load_config(os.path.join(ROOT, "configs", f"config_{name}.yaml"))
    AE, ch = cfg["AE"], cfg["Dataset"]["img_channels"]
    (e0, d0), (e1, d1), (e2, d2), (e3, d3) = _pair(AE, ch), _pair(AE, ch), _pair(AE, ch), _pair(AE, ch)
    others = dict(attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip", tail7x7="hip")
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, stem7x7="hip")
    fuse_frozen_autoencoder(e2, d2, **others)
    fuse_frozen_autoencoder(e3, d3, stem7x7="hip", **others)
    want = {"block0.0"}
    assert AE["ngf"] in (32, 64) and ch in (1, 3)
    assert {n for n, c in _folded(e1) if c.stem7x7} == want
    for n, c in _folded(e1):
        if n in want:
            assert not c.transposed and tuple(c.weight.shape) == (AE["ngf"], ch, 7, 7) and c.act == 1 and type(c.pad) is nn.ReflectionPad2d
            for k in ("_npvp_planes", "_npvp_w_amax"):
                assert k in c._buffers and k not in c.state_dict()
        else:
            assert "_npvp_planes" not in c._buffers and not _stem7x7_takes_hip(c), n
    assert not any(c.stem7x7 for _, c in _folded(d1)) and not any("_npvp_" in k for k, _ in d1.named_buffers())
    tails = [c for _, c in _folded(d1) if tuple(c.weight.shape[2:]) == (7, 7)]
    assert len(tails) == 1 and not _stem7x7_takes_hip(tails[0]), "the decoder's tail is out of the rule"
    assert not _tail7x7_takes_hip(e1.block0[0]), "as the stem is out of the tail's"
    for (k0, v0), (k1, v1) in zip(list(e0.state_dict().items()) + list(d0.state_dict().items()),
                                  list(e1.state_dict().items()) + list(d1.state_dict().items())):
        assert k0 == k1 and torch.equal(v0, v1), k0
    assert list(e3.state_dict()) == list(e0.state_dict()) and list(d3.state_dict()) == list(d0.state_dict())
    # the switches are independent
    assert not any(c.stem7x7 for _, c in _folded(e2) + _folded(d2))
    assert {n for n, c in _folded(e3) if c.stem7x7} == want and not any(c.stem7x7 for _, c in _folded(d3))
    for flag in ("conv3x3_pad", "down3x3"):
        assert {n for n, c in _folded(e3) if getattr(c, flag)} == {n for n, c in _folded(e2) if getattr(c, flag)} != set()
    assert {n for n, c in _folded(d3) if c.up3x3} == {n for n, c in _folded(d2) if c.up3x3} != set()
    assert {n for n, c in _folded(d3) if c.tail7x7} == {n for n, c in _folded(d2) if c.tail7x7} != set()
    assert not e3.block0[0].down3x3 and e3.block0[0].conv3x3_pad is None and not e3.block1[0].stem7x7


def test_the_rule_takes_only_what_the_kernel_runs():
    from npvp_amd.models.ResNetAutoEncoder import FoldedConvAct, _stem7x7_takes_hip
    ok = lambda conv, act=None, pad=nn.ReflectionPad2d(3): _stem7x7_takes_hip(FoldedConvAct(conv, None, act, pad))
    assert ok(nn.Conv2d(1, 64, 7), nn.ReLU()) and ok(nn.Conv2d(3, 32, 7), nn.ReLU()) and ok(nn.Conv2d(4, 96, 7)) and ok(nn.Conv2d(2, 64, 7))
    assert not ok(nn.Conv2d(3, 64, 7), nn.Tanh()) and not ok(nn.Conv2d(3, 64, 7), nn.Sigmoid()), "the stem's activations are none and ReLU"
    assert not ok(nn.Conv2d(5, 64, 7), nn.ReLU()) and not ok(nn.Conv2d(3, 48, 7), nn.ReLU()) and not ok(nn.Conv2d(64, 3, 7), nn.ReLU())
    assert not ok(nn.Conv2d(3, 64, 7), nn.ReLU(), None) and not ok(nn.Conv2d(3, 64, 7, padding=3), nn.ReLU(), None)
    assert not ok(nn.Conv2d(3, 64, 7), nn.ReLU(), nn.ReplicationPad2d(3)) and not ok(nn.Conv2d(3, 64, 7), nn.ReLU(), nn.ReflectionPad2d(2))
    assert not ok(nn.Conv2d(3, 64, 7, padding=1), nn.ReLU()) and not ok(nn.Conv2d(3, 64, 7, stride=2), nn.ReLU())
    assert not ok(nn.Conv2d(3, 64, 7, dilation=2), nn.ReLU()) and not ok(nn.Conv2d(3, 64, 5), nn.ReLU())
    assert not ok(nn.ConvTranspose2d(3, 64, 7), nn.ReLU())


def test_routed_stem_keeps_the_stock_forward_for_what_the_op_does_not_take(monkeypatch):
    """on the CPU: the branch is taken for planar frames of at least 4 x 4 pixels with no residual, and for nothing else"""
    import npvp_amd
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    enc, dec = _pair(AE_SMALL, 3)
    fuse_frozen_autoencoder(enc, dec, stem7x7="hip")
    stem = enc.block0[0]
    assert stem.stem7x7 and stem._npvp_planes is None, "the planes are built at the first routed forward on the device"
    taken = []
    monkeypatch.setattr(type(stem), "_stem7x7", lambda self, x: taken.append(tuple(x.shape)) or torch.zeros(x.shape[0], 32, *x.shape[2:]))
    monkeypatch.setattr(npvp_amd.ops, "bias_act", lambda y, b, act, res: y)
    x = torch.zeros(2, 3, 8, 8)
    stem(x)
    assert taken == [(2, 3, 8, 8)]
    stem(x.contiguous(memory_format=torch.channels_last))
    stem(x, residual=torch.zeros(2, 32, 8, 8))
    stem(x[:, :, ::2])
    assert taken == [(2, 3, 8, 8)], "channels-last, with a residual, strided: the stock forward"
    one = torch.zeros(2, 1, 8, 8).contiguous(memory_format=torch.channels_last)
    assert one.is_contiguous(), "one channel: the channels-last memory is the planar memory"
