"""CPU: the learn_3d=True autoencoder on clips of more than 32 frames without a GPU - the C ABI of the key-tiled temporal attention
(npvp_temporal_attn_long_fwd / _bwd) and its refusals, the argument checks of ops.temporal_attn_long_packed, the choice between the
one-tile and the key-tiled op by T alone, and the float64 restatement of tests/ae3d_cases.py against the reference fixture of a
50-frame clip (tests/golden/ae3d_long_block_*.npz)."""
import copy

import pytest
import torch

import ae3d_cases as AC
import ae3d_long_cases as LC
import golden_cases as GC
from oracle import ops as O

TOL = 1e-5          # the project's oracle-versus-reference bar (measured worst: tests/golden/AE3D_LONG_VS_REFERENCE.txt)


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


# ------------------------------------------------------------------------------------------------------------------ C ABI
def _fwd(N=2, T=40, HW=5, A=8, V=32, ld=48, ptr=4096):
    return (ptr, ld, ptr + 4 * A, ld, ptr + 8 * A, ld, 8192, V, 8192, N, T, HW, A, V, None)


def _bwd(N=2, T=40, HW=5, A=8, V=32, ld=48, ptr=4096, D=1 << 16):
    return (ptr, ld, ptr + 4 * A, ld, ptr + 8 * A, ld, 8192, V, 8192, D, 1 << 20, ld, (1 << 20) + 4 * A, ld, (1 << 20) + 8 * A, ld,
            N, T, HW, A, V, None)


REFUSALS = ((dict(T=0), b"T = 0"), (dict(A=12, V=48), b"(12, 48)"), (dict(A=8, V=64), b"(8, 64)"), (dict(ld=50), b"50"),
            (dict(ptr=4100), b"aligned"), (dict(ptr=0), b"null"), (dict(HW=0), b"HW = 0"),
            (dict(N=1 << 15, T=64, HW=1 << 10), b"2147483648"))


@pytest.mark.parametrize("name,args", [("npvp_temporal_attn_long_fwd", _fwd), ("npvp_temporal_attn_long_bwd", _bwd)])
def test_exports_and_argument_errors_do_not_need_a_gpu(L, name, args):
    """both exports are declared (the header the binding parses), defined (the library) and reachable through _npvp_fast; every
    refusal is made on the host before anything is launched: -1, the entry point's name and the offending value in npvp_last_error"""
    from npvp_amd import _lib, _npvp_fast as Fast
    assert name in _lib.parse_header(open(_lib.HEADER_PATH).read())
    fn = getattr(L, name)
    assert hasattr(L._cdll, name) and fn is getattr(Fast, name)
    n0 = L.npvp_launch_count()
    for kw, what in REFUSALS:
        assert fn(*args(**kw)) == -1, kw
        err = L.npvp_last_error()
        assert name.encode() in err and what in err, (kw, err)
    assert L.npvp_launch_count() == n0


def test_backward_refuses_a_null_or_misaligned_D(L):
    name = b"npvp_temporal_attn_long_bwd"
    for D, what in ((0, b"null buffer D"), ((1 << 16) + 4, b"aligned")):
        assert L.npvp_temporal_attn_long_bwd(*_bwd(D=D)) == -1
        err = L.npvp_last_error()
        assert name in err and what in err and b"D" in err, err
    # the old entry points keep their bound, by name
    assert L.npvp_temporal_attn_fwd(*_fwd(T=33)) == -1 and b"npvp_temporal_attn_fwd: T = 33" in L.npvp_last_error()


def test_op_argument_checks():
    from npvp_amd import ops
    with pytest.raises(RuntimeError, match=r"temporal_attn_long: .*\(12, 48\)"):
        ops.temporal_attn_long_packed(torch.zeros(40 * 4, 72), 1, 40, 4, 12, 48)
    with pytest.raises(RuntimeError, match="temporal_attn_long: qkv must be"):
        ops.temporal_attn_long_packed(torch.zeros(40 * 4 - 1, 48), 1, 40, 4, 8, 32)
    with pytest.raises(RuntimeError, match="temporal_attn_long: qkv must be"):
        ops.temporal_attn_long_packed(torch.zeros(40 * 4, 44), 1, 40, 4, 8, 32)
    with pytest.raises(RuntimeError, match="temporal_attn_long: the row length of qkv .* multiple of 4"):
        ops.temporal_attn_long_packed(torch.zeros(40 * 4, 50), 1, 40, 4, 8, 32)
    with pytest.raises(RuntimeError, match="temporal_attn_long: T = 0"):
        ops.temporal_attn_long_packed(torch.zeros(0, 48), 1, 0, 4, 8, 32)
    with pytest.raises(RuntimeError, match="temporal_attn_long: q / k"):
        ops.temporal_attn_long(torch.zeros(4, 40, 8), torch.zeros(4, 39, 8), torch.zeros(4, 40, 32), 40)
    with pytest.raises(RuntimeError, match="MI355X"):          # a CPU tensor never reaches a kernel
        ops.temporal_attn_long(torch.zeros(4, 40, 8), torch.zeros(4, 40, 8), torch.zeros(4, 40, 32), 40)
    with pytest.raises(RuntimeError, match="T = 33"):          # the one-tile op keeps its bound
        ops.temporal_attn_packed(torch.zeros(33 * 4, 48), 1, 33, 4, 8, 32)
    assert ops.TEMPORAL_ATTN_MAX_T == LC.MAX_T


# --------------------------------------------------------------------------------------------------------------- selection
def test_selection_goes_by_T_alone(monkeypatch):
    """_fused_attn1d of a fused AE_SMALL pair on CPU tensors, the two ops replaced by stand-ins that compute AC.temporal_attn_ref and
    record their name: T = 32 takes temporal_attn_packed, T = 33 the long op; both results are the unfused float64 block's attn1d.
    The trainable path's _attn1d chooses through the same ops.temporal_attn_any_packed."""
    import npvp_amd
    from npvp_amd import ops
    from npvp_amd.models.ResNetAutoEncoder import fuse_frozen_autoencoder, _fused_attn1d
    taken = []

    def stand_in(name):
        def op(qkv, N, T, HW, A, V):
            taken.append(name)
            return AC.temporal_attn_ref(qkv[:, :A], qkv[:, A:2 * A], qkv[:, 2 * A:2 * A + V], N, T, HW)
        return op
    monkeypatch.setattr(ops, "temporal_attn_packed", stand_in("temporal_attn_packed"))
    monkeypatch.setattr(ops, "temporal_attn_long_packed", stand_in("temporal_attn_long_packed"))
    enc, dec = npvp_amd.build_frozen_autoencoder(AC.AE_SMALL, 1)
    O.key_hashed_fill(npvp_amd.AEPair(enc, dec), LC.PAIR_SEED)
    ref = copy.deepcopy(enc).double().eval().res_3dConvAttn_0
    fuse_frozen_autoencoder(enc, dec)
    a = enc.res_3dConvAttn_0.attn1d
    N, H, W = 2, 2, 3
    for T, want_op in ((LC.MAX_T, "temporal_attn_packed"), (LC.MAX_T + 1, "temporal_attn_long_packed")):
        del taken[:]
        x = O.seeded_randn((N * T, 64, H, W), 610 + T)
        with torch.no_grad():
            got = _fused_attn1d(a, x.contiguous(memory_format=torch.channels_last), T)
            # the reference's route (ref/models/submodules.py:86-91): (N*H*W, C, T) sequences through attn1d and back
            seq = x.double().reshape(N, T, 64, H, W).permute(0, 3, 4, 2, 1).flatten(0, 2)
            want = ref.attn1d(seq).reshape(N, H, W, 64, T).permute(0, 4, 3, 1, 2).flatten(0, 1)
        assert taken == [want_op], (T, taken)
        assert AC.rel(got, want) < TOL, (T, AC.rel(got, want))
    del taken[:]
    for T in (LC.MAX_T, LC.MAX_T + 1):
        ops.temporal_attn_any_packed(torch.zeros(T * 4, 48), 1, T, 4, 8, 32)
    assert taken == ["temporal_attn_packed", "temporal_attn_long_packed"]


# --------------------------------------------------------------------------------------------------------------------- golden
def _check(name, got, want, worst):
    e = AC.rel(got, want)
    worst.append((e, name))
    assert e < TOL, (name, e)


@pytest.mark.parametrize("cf", [True, False], ids=["conv", "attn"])
def test_float64_restatement_matches_the_reference_on_a_long_clip(cf):
    """AC.block_ref in float64 against the reference's Factorized3DConvAttn(64, learn_3d=True) on one clip of 50 frames: every entry
    of the fixture at the 1e-5 bar of tests/test_ae3d_host.py"""
    from npvp_amd.models import Factorized3DConvAttn
    N, T, H, W = LC.LONG_BLOCK
    gold, tag = GC.load(LC.long_block_file(cf)), LC.long_block_tag(cf)
    assert int(gold["seed"]) == LC.BLOCK_SEED
    x, cot = LC.long_block_input()
    blk, worst = O.key_hashed_fill(Factorized3DConvAttn(AC.BLOCK_C, conv_first=cf, learn_3d=True), LC.BLOCK_SEED), []
    p = AC.block_params(blk)
    with torch.no_grad():
        _check("eval", AC.block_ref(p, x.double(), T, cf, False)[0], gold[f"{tag}.eval"], worst)
    xd = x.double().requires_grad_()
    y, stats = AC.block_ref(p, xd, T, cf, True)
    names = [n for n, _ in blk.named_parameters()]
    gs = torch.autograd.grad((y * cot.double()).sum(), [xd] + [p[n] for n in names])
    _check("y", y, gold[f"{tag}.y"], worst)
    _check("dx", gs[0], gold[f"{tag}.dx"], worst)
    for n, g in zip(names, gs[1:]):
        if n.endswith(AC.ZERO_GRAD):
            assert float(g.abs().max()) < 1e-6, n
        else:
            _check("grad." + n, g, gold[f"{tag}.grad.{n}"], worst)
    assert len(stats) == 8
    for k, v in stats.items():
        _check("stat." + k, v, gold[f"{tag}.stat.{k}"], worst)
    assert len(worst) == sum(not k.endswith(AC.ZERO_GRAD) for k in gold if k != "seed")
    print("worst", max(worst))
