"""CPU: the host layer around the autoencoder's attention kernels - the (attn dim, value dim) table of csrc/ae_attn_dims.h against
ops._NL_GRID, and the route ops.nonlocal_attn_any_packed takes.  Every C call here fails a host-side check: nothing is launched."""
import pytest
import torch

DIMS = [(A, V) for A in (4, 8, 12, 16, 24, 32, 48, 64, 128) for V in (4 * A, 4 * A + 4, 2 * A)]


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_python_and_c_agree_on_the_attn_dims_table(L):
    """npvp_nonlocal_attn_grid_fwd on dummy host addresses with every leading dimension 0: refused at the (A, V) check where the C
    table has no such pair, at the leading-dimension check (after it, before any launch) where it has.  npvp_temporal_attn_long_fwd
    on null buffers: refused at the (A, V) check, or at the first operand check after it."""
    from npvp_amd import ops
    err = L.npvp_last_error
    assert {(A, V) for A, V in DIMS if ops.nonlocal_attn_dims(A, V)} == set(ops.temporal_attn_dims()) == {(8, 32), (16, 64), (32, 128), (64, 256)}
    for A, V in DIMS:
        assert L.npvp_nonlocal_attn_grid_fwd(16, 0, 16, 0, 16, 0, 16, 0, 16, 1, 2, 2, A, V, None) == -1
        msg = err()
        assert (b"leading dimensions" in msg) == ops.nonlocal_attn_dims(A, V) and (b"attn dim" in msg) != ops.nonlocal_attn_dims(A, V), (A, V, msg)
        assert L.npvp_temporal_attn_long_fwd(None, 0, None, 0, None, 0, None, 0, None, 1, 1, 1, A, V, None) == -1
        msg, known = err(), (A, V) in ops.temporal_attn_dims()
        assert (b"null buffer q" in msg) == known and (b"(attn dim, value dim)" in msg) != known, (A, V, msg)


@pytest.mark.parametrize("A,V,H,W,want", [(8, 32, 64, 64, "config"), (64, 256, 8, 8, "config"), (16, 64, 16, 64, "config"),
                                          (8, 32, 6, 6, "grid"), (8, 32, 3, 5, "grid"), (8, 32, 32, 32, "grid"),
                                          (12, 48, 8, 8, "config")])
def test_nonlocal_attn_any_packed_picks_its_op(monkeypatch, A, V, H, W, want):
    """config shapes -> nonlocal_attn_packed, every other grid of a known (A, V) -> nonlocal_attn_grid_packed, an (A, V) no kernel has
    -> nonlocal_attn_packed, which refuses it; both ops are looked up at call time (recorders here)"""
    from npvp_amd import ops
    calls = []
    rec = lambda tag: lambda *a: calls.append((tag,) + a[1:]) or a[0]
    qkv = torch.zeros(2 * H * W, 2 * A + V)
    with monkeypatch.context() as m:
        m.setattr(ops, "nonlocal_attn_packed", rec("config"))
        m.setattr(ops, "nonlocal_attn_grid_packed", rec("grid"))
        assert ops.nonlocal_attn_any_packed(qkv, 2, H, W, A, V) is qkv
    assert calls == [(want, 2, H, W, A, V)]
    if not ops.nonlocal_attn_dims(A, V):
        with pytest.raises(RuntimeError, match=r"nonlocal_attn: \(attn dim, value dim\) = \(12, 48\) is not one of the AE configs'"):
            ops.nonlocal_attn_any_packed(qkv, 2, H, W, A, V)
