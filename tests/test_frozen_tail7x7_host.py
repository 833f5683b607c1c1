"""CPU: the host side of the frozen decoder's opt-in 7 x 7 tail route - the tail7x7 switch of to_device_layout /
fuse_frozen_autoencoder and which convolution it marks, the index functions and the planners the kernels call (exported unchanged by the
C ABI), the refusals of the entry points, and the float64 reference of tests/frozen_tail7x7_cases.py against wrong restatements of the
forward and of the input gradient.

A wrong restatement is held to the bar on every case where it is a different statement at all: `frames_stacked` is the reference itself
on a single frame, `act_before_bias` and `act_derivative_dropped` are the reference itself where the activation is none (APPLIES)."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import frozen_tail7x7_cases as TC
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE_SMALL = dict(ngf=32, n_downsampling=2, num_res_blocks=1, learn_3d=True, out_layer='Tanh')
APPLIES = {"frames_stacked": lambda c: c[4] > 1, "act_before_bias": lambda c: c[5] != "none",
           "act_derivative_dropped": lambda c: c[5] != "none"}


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
    out = {}
    for c in TC.KERNEL_CASES:
        ins = TC.inputs(c)
        out[c] = (ins, TC.ref64(c, ins=ins))
    return out


def test_reference_is_the_module_stack(refs):
    """the reference equals ReflectionPad2d(3) -> Conv2d(C_in, C_out, 7) -> activation in float64"""
    for case in TC.KERNEL_CASES:
        Ci, Co, H, W, Fr, act = case
        i, ref = refs[case]
        mods = [nn.ReflectionPad2d(3), nn.Conv2d(Ci, Co, 7)] + ({"tanh": [nn.Tanh()], "sigmoid": [nn.Sigmoid()], "none": []}[act])
        seq = nn.Sequential(*mods).double()
        with torch.no_grad():
            seq[1].weight.copy_(i["w"]); seq[1].bias.copy_(i["bias"])
            y = seq(i["x"].double())
        assert y.shape == ref.shape == (Fr, Co, H, W)
        assert TC.rel(y, ref) < 1e-12, case
    i, _ = refs[TC.SCALED_CASE]
    assert 1000 < float(i["x"].abs().max()) and float(i["w"].abs().max()) < 1e-2, "the scaled case is not scaled"


def test_case_table_is_the_issues():
    assert TC.KERNEL_CASES == [(64, 3, 64, 64, 1, "tanh"), (64, 1, 4, 4, 9, "sigmoid"), (32, 3, 5, 9, 2, "tanh"), (64, 3, 6, 150, 1, "none"),
                               (64, 4, 7, 128, 2, "tanh"), (64, 3, 8, 16, 2, "none")]
    assert TC.SCALED_CASE is TC.KERNEL_CASES[5] and len({TC.case_id(c) for c in TC.KERNEL_CASES}) == 6
    assert TC.F16X3_TOL == 1e-5 and TC.BAR == 1e-4 and TC.GRAD_BAR == 5e-3


def test_every_wrong_forward_restatement_misses_the_bar_by_two_orders(refs):
    seen = {m: 0 for m in TC.MUTANTS}
    for case in TC.KERNEL_CASES:
        ins, ref = refs[case]
        for m in TC.MUTANTS:
            if not APPLIES.get(m, lambda c: True)(case):
                continue
            mut = TC.ref64(case, m, ins)
            e = TC.rel(mut, ref)
            print(TC.case_id(case), m, f"{e:.3e}")
            assert mut.shape == ref.shape and e > 100 * TC.F16X3_TOL, (m, TC.case_id(case), e)
            seen[m] += 1
    assert all(n >= 4 for n in seen.values()), seen


def test_every_wrong_gradient_restatement_misses_the_bar_by_two_orders(refs):
    seen = {m: 0 for m in TC.GRAD_MUTANTS}
    for case in TC.KERNEL_CASES:
        ins, ref = refs[case]
        dref = TC.dgrad64(case, ins, y=ref)
        assert dref.shape == ins["x"].shape
        for m in TC.GRAD_MUTANTS:
            if not APPLIES.get(m, lambda c: True)(case):
                continue
            e = TC.rel(TC.dgrad64(case, ins, y=ref, mutant=m), dref)
            print(TC.case_id(case), m, f"{e:.3e}")
            assert e > 100 * TC.F16X3_TOL, (m, TC.case_id(case), e)
            seen[m] += 1
    assert all(n >= 4 for n in seen.values()), seen


# ------------------------------------------------------------------------------------------------------------ index functions
EXTENTS = tuple(range(4, 13)) + (64,)


def test_src_is_the_index_map_of_reflection_padding(L):
    for extent in EXTENTS:
        want = TC.expected_src(extent)
        for c in range(extent):
            for tap in range(7):
                assert L.npvp_tail7x7_src(c, tap, extent) == want[c][tap], (extent, c, tap)
    assert [L.npvp_tail7x7_src(0, t, 4) for t in range(7)] == [3, 2, 1, 0, 1, 2, 3]
    assert [L.npvp_tail7x7_src(3, t, 4) for t in range(7)] == [0, 1, 2, 3, 2, 1, 0]


def test_adj_src_is_the_adjoint_of_reflection_padding(L):
    """straight and mirror together are exactly the output coordinates autograd sends a one-hot gradient back from; they never
    coincide; the mirror exists only below tap 3 (low edge) or above it (high edge)"""
    for extent in EXTENTS:
        want = TC.expected_adj(extent)
        for s in range(extent):
            for tap in range(7):
                o0, o1 = L.npvp_tail7x7_adj_src(s, tap, extent, 0), L.npvp_tail7x7_adj_src(s, tap, extent, 1)
                assert o0 == -1 or 0 <= o0 < extent
                assert o1 == -1 or 0 <= o1 < extent
                assert o0 == -1 or o0 != o1
                assert o0 == (s + 3 - tap if 0 <= s + 3 - tap < extent else -1)
                assert tap != 3 or o1 == -1
                assert sorted(o for o in (o0, o1) if o >= 0) == want[s][tap], (extent, s, tap)
                for o in (o0, o1):
                    assert o < 0 or L.npvp_tail7x7_src(o, tap, extent) == s
    # the minimum extent: both mirrors reach the same pixels (source 1 is read through the low mirror and through the high one)
    assert L.npvp_tail7x7_adj_src(1, 0, 4, 1) == 2 and L.npvp_tail7x7_adj_src(1, 6, 4, 1) == 2


def test_index_functions_refuse_what_is_outside_their_domain(L):
    for args in ((0, -1, 8), (0, 7, 8), (-1, 0, 8), (8, 0, 8), (0, 0, 3), (0, 0, 0)):
        assert L.npvp_tail7x7_src(*args) == -2, args
        assert L.npvp_tail7x7_adj_src(*args, 0) == -2 and L.npvp_tail7x7_adj_src(*args, 1) == -2, args
    assert L.npvp_tail7x7_adj_src(0, 0, 8, 2) == -2 and L.npvp_tail7x7_adj_src(0, 0, 8, -1) == -2
    assert L.npvp_tail7x7_src(0, 0, 4) == 3 and L.npvp_tail7x7_adj_src(0, 0, 4, 0) == 3


def _restated(L, case, ins):
    """forward and input gradient in float64 from the exported index functions alone"""
    Ci, Co, H, W, Fr, act = case
    x, w, g = ins["x"].double(), ins["w"].double(), ins["g"].double()
    y = torch.zeros(Fr, Co, H, W, dtype=torch.float64)
    dx = torch.zeros(Fr, Ci, H, W, dtype=torch.float64)
    for kh in range(7):
        for kw in range(7):
            hs = [L.npvp_tail7x7_src(h, kh, H) for h in range(H)]
            ws = [L.npvp_tail7x7_src(v, kw, W) for v in range(W)]
            y += torch.einsum("fchw,oc->fohw", x[:, :, hs][:, :, :, ws], w[:, :, kh, kw])
            a = torch.zeros(Fr, Co, H, W, dtype=torch.float64)
            for wh in (0, 1):
                for wv in (0, 1):
                    oh = [L.npvp_tail7x7_adj_src(s, kh, H, wh) for s in range(H)]
                    ov = [L.npvp_tail7x7_adj_src(t, kw, W, wv) for t in range(W)]
                    mh = torch.tensor([o >= 0 for o in oh], dtype=torch.float64).view(1, 1, H, 1)
                    mv = torch.tensor([o >= 0 for o in ov], dtype=torch.float64).view(1, 1, 1, W)
                    a += g[:, :, [max(o, 0) for o in oh]][:, :, :, [max(o, 0) for o in ov]] * mh * mv
            dx += torch.einsum("fohw,oc->fchw", a, w[:, :, kh, kw])
    return y + ins["bias"].double().view(1, Co, 1, 1), dx


@pytest.mark.parametrize("case", [TC.KERNEL_CASES[1], TC.KERNEL_CASES[2], TC.KERNEL_CASES[5]], ids=TC.case_id)
def test_restatement_from_the_index_functions_is_pad_and_conv(L, case, refs):
    ins, _ = refs[case]
    x64 = ins["x"].double().requires_grad_()
    pre = TC.pre64(case, ins, x64)
    (dref,) = torch.autograd.grad(pre, x64, ins["g"].double())
    y, dx = _restated(L, case, ins)
    assert TC.rel(y, pre) < 1e-12 and TC.rel(dx, dref) < 1e-12


# --------------------------------------------------------------------------------------------------------------------- planners
PLAN_SHAPES = [c[:5] for c in TC.KERNEL_CASES] + [(64, 3, 5, w, 1) for w in TC.PLAN_WIDTHS]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_tiles_cover_every_pixel_once_and_hold_their_windows(L, shape):
    Ci, Co, H, W, Fr = shape
    out, p = _ints(8)
    assert L.npvp_tail7x7_route(Fr, H, W, Ci, Co, p) == 0
    rows, segs, seg_cols, tiles_r, grid, bm, bn, ksteps = list(out)
    assert (bm, bn, ksteps) == (128, 32, 7 * Ci // 32) and grid == tiles_r * segs
    assert rows == max(1, 128 // W) and tiles_r == -(-Fr * H // rows)
    assert (segs, seg_cols) == ((1, W) if W <= 128 else (-(-W // 122), 122))
    count = torch.zeros(Fr * H, W, dtype=torch.int32)
    t6, p6 = _ints(6)
    ragged = 0
    for blk in range(grid):
        assert L.npvp_tail7x7_tile(Fr, H, W, Ci, Co, blk, p6) == 0
        r0, r1, w0, w1, z0, z1 = list(t6)
        assert 0 <= r0 < r1 <= Fr * H and r1 - r0 <= rows and 0 <= w0 < w1 <= W and 0 <= z0 <= w0 and w1 <= z1 <= W
        assert (r1 - r0) * (z1 - z0) <= 128, "a tile's Z rows fit the 128-row GEMM tile"
        ragged += r1 - r0 < rows
        count[r0:r1, w0:w1] += 1
        # every image row of the tile gathers its kh taps inside its own frame
        for r in range(r0, r1):
            f, h = divmod(r, H)
            assert all(f * H <= f * H + L.npvp_tail7x7_src(h, kh, H) < (f + 1) * H for kh in range(7))
        # the Z window holds every column the shifted sum reads
        for w in sorted({w0, w0 + 1, w0 + 2, (w0 + w1) // 2, w1 - 3, w1 - 2, w1 - 1} & set(range(w0, w1))):
            assert all(z0 <= L.npvp_tail7x7_src(w, kw, W) < z1 for kw in range(7)), (blk, w)
    assert int(count.min()) == 1 and int(count.max()) == 1
    assert ragged == (1 if (Fr * H) % rows else 0)
    for bad in (-1, grid):
        assert L.npvp_tail7x7_tile(Fr, H, W, Ci, Co, bad, p6) == -1


def test_case_table_reaches_what_it_claims(L):
    def plan(c):
        out, p = _ints(8)
        assert L.npvp_tail7x7_route(c[4], c[2], c[3], c[0], c[1], p) == 0
        return list(out)
    c0, c1, c2, c3, c4, c5 = TC.KERNEL_CASES
    assert plan(c0)[0] == 2, "two image rows per tile at the configs' frame"
    assert plan(c1)[0] == 32 and 32 // c1[2] == 8 and (c1[4] * c1[2]) % 32 != 0, "a tile spans 8 frames, the last tile is ragged"
    assert c2[0] == 32 and c2[2] % 2 == 1 and c2[3] % 2 == 1 and (c2[4] * c2[1] * c2[2] * c2[3]) % 4 != 0
    assert plan(c3)[1] == 2 and plan(c3)[0] == 1, "two column segments"
    assert c4[3] == 128 and plan(c4)[1] == 1 and plan(c4)[0] == 1 and c4[1] == 4
    out, p = _ints(6)
    assert L.npvp_tail7x7_dgrad_route(c2[4], c2[2], c2[3], c2[0], c2[1], p) == 0 and list(out)[:3] == [2, 128, 32]
    assert L.npvp_tail7x7_dgrad_route(c0[4], c0[2], c0[3], c0[0], c0[1], p) == 0 and list(out)[:3] == [1, 128, 64]


@pytest.mark.parametrize("shape", PLAN_SHAPES + [(128, 3, 4, 4, 3), (96, 2, 4, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_dgrad_tiles_cover_every_row_and_column_once(L, shape):
    Ci, Co, H, W, Fr = shape
    M = Fr * H * W
    out, p = _ints(6)
    assert L.npvp_tail7x7_dgrad_route(Fr, H, W, Ci, Co, p) == 0
    variant, bm, bn, tm, tn, grid = list(out)
    assert (variant, bn) == ((1, 64) if Ci % 64 == 0 else (2, 32)) and bm == 128 and tm == -(-M // 128) and tn == Ci // bn and grid == tm * tn
    count = torch.zeros(M, Ci, dtype=torch.int32)
    t4, p4 = _ints(4)
    for blk in range(grid):
        assert L.npvp_tail7x7_dgrad_tile(Fr, H, W, Ci, Co, blk, p4) == 0
        m0, m1, n0, n1 = list(t4)
        assert 0 <= m0 < m1 <= M and m1 - m0 <= bm and 0 <= n0 < n1 <= Ci and n1 - n0 == bn
        count[m0:m1, n0:n1] += 1
    assert int(count.min()) == 1 and int(count.max()) == 1
    for bad in (-1, grid):
        assert L.npvp_tail7x7_dgrad_tile(Fr, H, W, Ci, Co, bad, p4) == -1


# ----------------------------------------------------------------------------------------------------------------- entry points
NAMES = ("npvp_tail7x7_src", "npvp_tail7x7_adj_src", "npvp_tail7x7_route", "npvp_tail7x7_tile", "npvp_tail7x7_dgrad_route",
         "npvp_tail7x7_dgrad_tile", "npvp_tail7x7_planes_bytes", "npvp_tail7x7_planes", "npvp_tail7x7_dgrad_planes", "npvp_tail7x7_f16",
         "npvp_tail7x7_dgrad_f16")


def test_entry_points_are_declared_and_refuse_on_the_host(L):
    from npvp_amd import _lib
    protos = _lib.parse_header(open(_lib.HEADER_PATH).read())
    for name in NAMES:
        assert name in protos and hasattr(L._cdll, name), name
    assert protos["npvp_tail7x7_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_tail7x7_f16"][1]) == 15
    assert protos["npvp_tail7x7_dgrad_f16"][1][-1] == "npvp_stream_t" and len(protos["npvp_tail7x7_dgrad_f16"][1]) == 13
    assert L.npvp_tail7x7_planes_bytes(64, 3) == L.npvp_tail7x7_planes_bytes(64, 1) == 2 * 2 * 7 * 64 * 32
    assert L.npvp_tail7x7_planes_bytes(32, 4) == 2 * 2 * 7 * 32 * 32
    for bad in ((48, 3), (0, 3), (64, 0), (64, 5), (8192, 3)):
        assert L.npvp_tail7x7_planes_bytes(*bad) == -1, bad
    out, p = _ints(8)
    for shape in ((1, 8, 8, 48, 3), (1, 8, 8, 64, 5), (1, 8, 8, 64, 0), (0, 8, 8, 64, 3), (1, 3, 8, 64, 3), (1, 8, 3, 64, 3),
                  (1 << 11, 1 << 10, 1 << 10, 64, 3)):
        assert L.npvp_tail7x7_route(*shape, p) == -1 and L.npvp_tail7x7_dgrad_route(*shape, p) == -1, shape
    assert L.npvp_tail7x7_route((1 << 11) - 1, 1 << 10, 1 << 10, 64, 3, p) == 0, "F H W just below 2^31 is taken"

    def fwd(**kw):
        a = dict(x=4096, planes=8192, bias=12288, y=16384, F=1, H=4, W=4, Ci=32, Co=3, act=2, xa=20480, wa=24576, ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)

    def bwd(**kw):
        a = dict(dz=4096, planes=8192, dx=16384, F=1, H=4, W=4, Ci=32, Co=3, da=20480, wa=24576, ws=None, wsb=0)
        a.update(kw)
        return tuple(a.values()) + (None,)
    n0 = L.npvp_launch_count()
    shape_refusals = ((dict(Ci=48), b"C_in a multiple of 32"), (dict(Co=5), b"1 <= C_out <= 4"), (dict(Co=0), b"1 <= C_out <= 4"),
                      (dict(F=0), b"F >= 1"), (dict(H=3), b"H, W >= 4"), (dict(W=3), b"H, W >= 4"),
                      (dict(F=1 << 11, H=1 << 10, W=1 << 10), b"F * H * W below 2^31"))
    for kw, what in ((dict(x=None), b"non-null"), (dict(planes=None), b"non-null"), (dict(bias=None), b"non-null"), (dict(y=None), b"non-null"),
                     (dict(xa=None), b"non-null"), (dict(wa=None), b"non-null"), (dict(act=1), b"act 0 (none), 2 (tanh) or 3 (sigmoid)"),
                     (dict(act=4), b"act 0"), (dict(act=-1), b"act 0"), (dict(y=16388), b"16-byte aligned"), (dict(x=4100), b"16-byte aligned"),
                     (dict(planes=8200), b"16-byte aligned")) + shape_refusals:
        assert L.npvp_tail7x7_f16(*fwd(**kw)) == -1, kw
        assert what in L.npvp_last_error() and b"tail7x7" in L.npvp_last_error(), (kw, L.npvp_last_error())
    for kw, what in ((dict(dz=None), b"non-null"), (dict(planes=None), b"non-null"), (dict(dx=None), b"non-null"), (dict(da=None), b"non-null"),
                     (dict(wa=None), b"non-null"), (dict(dz=4100), b"16-byte aligned"), (dict(dx=16388), b"16-byte aligned"),
                     (dict(planes=8200), b"16-byte aligned")) + shape_refusals:
        assert L.npvp_tail7x7_dgrad_f16(*bwd(**kw)) == -1, kw
        assert what in L.npvp_last_error() and b"tail7x7_dgrad" in L.npvp_last_error(), (kw, L.npvp_last_error())
    for fn in (L.npvp_tail7x7_planes, L.npvp_tail7x7_dgrad_planes):
        assert fn(None, 64, 3, 8192, 4096, None) == -1 and b"non-null" in L.npvp_last_error()
        assert fn(4096, 64, 3, None, 4096, None) == -1 and fn(4096, 64, 3, 8192, None, None) == -1
        assert fn(4096, 48, 3, 8192, 4096, None) == -1 and b"multiple of 32" in L.npvp_last_error()
        assert fn(4096, 64, 5, 8192, 4096, None) == -1 and b"C_out <= 4" in L.npvp_last_error()
        assert fn(4100, 64, 3, 8192, 4096, None) == -1 and b"16-byte aligned" in L.npvp_last_error()
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
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, TAIL7X7_ROUTES
    assert TAIL7X7_ROUTES == ("stock", "hip")
    enc, dec = _pair()
    before = [n for n, _ in dec.named_modules()]
    for bad in ("rocm", "HIP", None, True):
        with pytest.raises(ValueError, match="tail7x7=.*'stock', 'hip'"):
            fuse_frozen_autoencoder(enc, dec, tail7x7=bad)
        with pytest.raises(ValueError, match="tail7x7="):
            npvp_amd.to_device_layout(enc, dec, "cpu", tail7x7=bad)
        with pytest.raises(ValueError, match="tail7x7="):
            fuse_frozen_autoencoder(enc, dec, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip", tail7x7=bad)
    assert [n for n, _ in dec.named_modules()] == before and isinstance(dec.model[1], nn.BatchNorm2d), "a refused call changed the pair"


def test_stock_is_the_default_and_routes_nothing():
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, FoldedConvAct, ResnetDecoder
    (e0, d0), (e1, d1) = _pair(), _pair()
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, tail7x7="stock")
    for a, b in ((e0, e1), (d0, d1)):
        assert [(n, type(m)) for n, m in a.named_modules()] == [(n, type(m)) for n, m in b.named_modules()]
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
        for (k0, v0), (k1, v1) in zip(a.state_dict().items(), b.state_dict().items()):
            assert k0 == k1 and torch.equal(v0, v1), k0
        for n, c in _folded(a) + _folded(b):
            assert c.tail7x7 is False and not [k for k, _ in c.named_buffers() if k.startswith("_npvp_")], n
            assert set(dict(c.named_buffers())) == {"weight", "bias"} and type(c).forward is FoldedConvAct.forward and "forward" not in c.__dict__
    for d in (d0, d1):
        assert d.tail7x7 is False and "tail7x7" not in d.__dict__ and type(d).forward is ResnetDecoder.forward


@pytest.mark.parametrize("name", TC.AE_CONFIGS)
def test_hip_marks_exactly_the_tail_of_the_configs(name):
    """the five configs' AE sections: the decoder's last FoldedConvAct and nothing else, nothing in the encoder (its 7 x 7 stem has
    C_in = 1 or 3); the state dict does not change; the other four switches do not mark the tail"""
    from npvp_amd import trainer
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, _tail7x7_takes_hip
    cfg = trainer.load_config(os.path.join(ROOT, "configs", f"config_{name}.yaml"))
    AE, ch = cfg["AE"], cfg["Dataset"]["img_channels"]
    (e0, d0), (e1, d1), (e2, d2), (e3, d3) = _pair(AE, ch), _pair(AE, ch), _pair(AE, ch), _pair(AE, ch)
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, tail7x7="hip")
    fuse_frozen_autoencoder(e2, d2, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip")
    fuse_frozen_autoencoder(e3, d3, attn2d="hip", conv3x3="hip", down3x3="hip", up3x3="hip", tail7x7="hip")
    n_up = AE["n_downsampling"]
    want = {f"model.{n_up}"}
    assert len(_folded(d1)) == n_up + 1 and AE["ngf"] in (32, 64) and ch in (1, 3)
    assert {n for n, c in _folded(d1) if c.tail7x7} == want and d1.tail7x7 is True and d0.tail7x7 is False and d1.up3x3 is False
    for n, c in _folded(d1):
        if n in want:
            assert not c.transposed and tuple(c.weight.shape) == (ch, AE["ngf"], 7, 7) and c.act in (2, 3) and type(c.pad) is nn.ReflectionPad2d
            for k in c._TAIL7X7_BUFFERS:
                assert k in c._buffers and k not in c.state_dict()
        else:
            assert "_npvp_planes" not in c._buffers and not _tail7x7_takes_hip(c), n
    assert not any(c.tail7x7 for _, c in _folded(e1)) and not any("_npvp_" in k for k, _ in e1.named_buffers())
    stems = [c for _, c in _folded(e1) if tuple(c.weight.shape[2:]) == (7, 7)]
    assert len(stems) == 1 and not _tail7x7_takes_hip(stems[0]), "the encoder's stem is out of the rule"
    for (k0, v0), (k1, v1) in zip(list(e0.state_dict().items()) + list(d0.state_dict().items()),
                                  list(e1.state_dict().items()) + list(d1.state_dict().items())):
        assert k0 == k1 and torch.equal(v0, v1), k0
    # the switches are independent
    assert not any(c.tail7x7 for _, c in _folded(d2)) and d2.tail7x7 is False and d2.up3x3 is True
    assert {n for n, c in _folded(d3) if c.tail7x7} == want and d3.tail7x7 is True
    assert {n for n, c in _folded(d3) if c.up3x3} == {n for n, c in _folded(d2) if c.up3x3} != set()
    assert {n for n, c in _folded(e3) if c.conv3x3_pad} == {n for n, c in _folded(e2) if c.conv3x3_pad} != set()
    assert not any(c.tail7x7 for _, c in _folded(e3))


def test_the_rule_takes_only_what_the_kernels_run():
    from npvp_amd.models.ResNetAutoEncoder import FoldedConvAct, _tail7x7_takes_hip
    ok = lambda conv, act=None, pad=nn.ReflectionPad2d(3): _tail7x7_takes_hip(FoldedConvAct(conv, None, act, pad))
    assert ok(nn.Conv2d(64, 3, 7), nn.Tanh()) and ok(nn.Conv2d(32, 1, 7), nn.Sigmoid()) and ok(nn.Conv2d(96, 4, 7))
    assert not ok(nn.Conv2d(64, 3, 7), nn.ReLU()), "ReLU is not one of the tail's activations"
    assert not ok(nn.Conv2d(64, 5, 7), nn.Tanh()) and not ok(nn.Conv2d(48, 3, 7), nn.Tanh()) and not ok(nn.Conv2d(3, 64, 7), nn.Tanh())
    assert not ok(nn.Conv2d(64, 3, 7), nn.Tanh(), None) and not ok(nn.Conv2d(64, 3, 7, padding=3), nn.Tanh(), None)
    assert not ok(nn.Conv2d(64, 3, 7), nn.Tanh(), nn.ReplicationPad2d(3)) and not ok(nn.Conv2d(64, 3, 7), nn.Tanh(), nn.ReflectionPad2d(2))
    assert not ok(nn.Conv2d(64, 3, 7, padding=1), nn.Tanh()) and not ok(nn.Conv2d(64, 3, 7, stride=2), nn.Tanh())
    assert not ok(nn.Conv2d(64, 3, 7, dilation=2), nn.Tanh()) and not ok(nn.Conv2d(64, 3, 5), nn.Tanh())
    assert not ok(nn.ConvTranspose2d(64, 3, 7), nn.Tanh())


def test_layouts_of_the_routed_decoders_weights():
    """up3x3="hip", tail7x7="stock": the stock tail keeps NCHW weights (UP3X3_TAIL, unchanged); both routed: what stays stock between the
    routed convolutions (the 64 -> 32 transposed convolution of an ngf = 32 decoder) keeps the channels-last weights it was moved to,
    so no copy back to NCHW remains; tail alone: the decoder stays NCHW"""
    import npvp_amd
    from npvp_amd.models import ResNetAutoEncoder as RAE
    assert RAE.UP3X3_TAIL == "nchw"
    AE = dict(AE_SMALL, ngf=32, n_downsampling=3, learn_3d=False)
    enc, dec = _pair(AE, 3)
    npvp_amd.to_device_layout(enc, dec, "cpu", up3x3="hip", tail7x7="stock")
    assert [m.up3x3 for m in dec.model] == [True, True, False, False] and not any(m.tail7x7 for m in dec.model)
    assert [m.weight.is_contiguous() for m in dec.model] == [False, False, True, True]
    enc, dec = _pair(AE, 3)
    npvp_amd.to_device_layout(enc, dec, "cpu", up3x3="hip", tail7x7="hip")
    assert [m.up3x3 for m in dec.model] == [True, True, False, False] and [m.tail7x7 for m in dec.model] == [False, False, False, True]
    assert [m.weight.is_contiguous() for m in dec.model[:3]] == [False, False, False]
    enc, dec = _pair(AE, 3)
    npvp_amd.to_device_layout(enc, dec, "cpu", tail7x7="hip")
    assert all(m.weight.is_contiguous() for m in dec.model) and dec.tail7x7 and not dec.up3x3


def test_routed_forward_hands_the_tail_channels_last_frames(monkeypatch):
    """on CPU tensors with the ops replaced: NCHW memory at the routed tail module runs the stock forward itself; a channels-last input
    goes to the op with the module's activation; the decoder with up3x3="stock" makes ONE copy to channels-last in front of the tail, and
    with up3x3="hip" the tail takes the channels-last tensor as it comes (ngf = 64: no copy back to NCHW anywhere)"""
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder
    called = []
    monkeypatch.setattr(ops, "bias_act", lambda y, b, act=0, residual=None: (called.append("bias_act"), y)[1])
    monkeypatch.setattr(ops, "tail7x7_planes", lambda w: (called.append("planes"), ops.Tail7x7Planes(*(torch.zeros(1),) * 3))[1])
    monkeypatch.setattr(ops, "convt3x3s2_planes", lambda w: ops.ConvT3x3Planes(*(torch.zeros(1),) * 5))

    def tail(x, planes, bias, act):
        called.append(("tail7x7", act, x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous(), x.requires_grad))
        return x[:, :bias.shape[0]].contiguous()
    monkeypatch.setattr(ops, "tail7x7_packed", tail)
    monkeypatch.setattr(ops, "convt3x3s2_packed", lambda x, planes, bias, act: (
        called.append("up3x3"), F.interpolate(x[:, :bias.shape[0]], scale_factor=2).contiguous(memory_format=torch.channels_last))[1])
    AE = dict(AE_SMALL, ngf=64, learn_3d=False)
    (e0, d0), (e1, d1), (e2, d2) = _pair(AE), _pair(AE), _pair(AE)
    fuse_frozen_autoencoder(e0, d0)
    fuse_frozen_autoencoder(e1, d1, tail7x7="hip")
    fuse_frozen_autoencoder(e2, d2.to(memory_format=torch.channels_last), up3x3="hip", tail7x7="hip")
    assert not called, "CPU weights: the planes wait for the first routed forward"
    s, h = d0.model[-1], d1.model[-1]
    assert h.tail7x7 and h._npvp_planes is None and h.act == 2
    x = O.seeded_randn((2, 64, 5, 6), 1)
    with torch.no_grad():
        y = h(x)
        assert y.shape == (2, 1, 5, 6) and torch.equal(y, s(x))
    assert called == ["bias_act"] * 2, "NCHW memory: the stock forward, no silent copy"
    del called[:]
    h(x.contiguous(memory_format=torch.channels_last).requires_grad_())
    assert called == ["planes", ("tail7x7", 2, True, True)]
    del called[:]
    feats = x[:, :, :2, :2].repeat(1, 4, 1, 1).reshape(1, 2, 256, 2, 2)
    with torch.no_grad():
        out = d1(feats)
    assert out.shape == (1, 2, 1, 8, 8) and called == ["bias_act", "bias_act", ("tail7x7", 2, True, False)]
    del called[:]
    with torch.no_grad():
        out = d2(feats)
    assert out.shape == (1, 2, 1, 8, 8) and called == ["up3x3", "up3x3", "planes", ("tail7x7", 2, True, False)]
