"""CPU: the host side of the centre-pad route of spatial window attention (ref/models/VidHRFormer.py:488-511): the geometry
helper, the declaration and argument checks of npvp_grid_center_pad / npvp_grid_center_cut, AttnCfg's default, and the committed
fixture against the CPU restatement ("pad keys are attended, not masked")."""
import math
import os
import re

import pytest
import torch

import golden_cases as GC
import window_pad_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["npvp_grid_center_pad", "npvp_grid_center_cut"]


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_geometry_helper_equals_padblock():
    from npvp_amd.ops import window_pad_geometry
    seen_odd = seen_big_window = False
    for ws in (4, 7, 8):
        for H in range(1, 21):
            for W in range(1, 21):
                # ref PadBlock.pad_if_needed / depad_if_needed, restated here
                pad_h = math.ceil(H / ws) * ws - H
                pad_w = math.ceil(W / ws) * ws - W
                top, bottom, left, right = pad_h // 2, pad_h - pad_h // 2, pad_w // 2, pad_w - pad_w // 2
                assert window_pad_geometry(H, W, ws) == (H + top + bottom, W + left + right, top, left), (H, W, ws)
                seen_odd |= top < bottom
                seen_big_window |= ws > H
    assert seen_odd and seen_big_window


def test_declared_in_the_header_and_bound():
    from npvp_amd._lib import SIGNATURES, c_int, c_ll, c_p
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npvp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(npvp_[a-z0-9_]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/npvp_hip.h"
        assert n in SIGNATURES, f"{n} has no signature in npvp_amd/_lib.py"
    geom = [c_int] * 8          # F, H, W, Hp, Wp, top, left, C
    assert SIGNATURES["npvp_grid_center_pad"] == (c_int, [c_p, c_ll, c_p, c_ll] + geom + [c_ll, c_p, c_p])
    assert SIGNATURES["npvp_grid_center_cut"] == (c_int, [c_p, c_ll, c_p, c_ll, c_p, c_ll] + geom + [c_p, c_p])


def pad_args(ld_src=512, ld_dst=512, F=2, H=5, W=6, Hp=8, Wp=8, top=1, left=1, C=512, rows_out=128):
    return (None, ld_src, None, ld_dst, F, H, W, Hp, Wp, top, left, C, rows_out, None, None)


def cut_args(ld_src=512, ld_add=512, ld_dst=512, F=2, H=5, W=6, Hp=8, Wp=8, top=1, left=1, C=512):
    return (None, ld_src, None, ld_add, None, ld_dst, F, H, W, Hp, Wp, top, left, C, None, None)


def test_argument_errors_do_not_need_a_gpu(L):
    """every check of the issue's list answers before a launch (the buffers here are NULL: a call that got past its checks would
    say "null buffer", which is the last check)"""
    for fn, args in ((L.npvp_grid_center_pad, pad_args), (L.npvp_grid_center_cut, cut_args)):
        for kw, msg in ((dict(Hp=4), b"smaller"), (dict(Wp=5), b"smaller"), (dict(top=4), b"inside"), (dict(top=-1), b"inside"),
                        (dict(left=3), b"inside"), (dict(left=-1), b"inside"), (dict(C=510), b"multiple of 4"),
                        (dict(ld_src=514), b"strides"), (dict(ld_dst=510), b"strides"), (dict(ld_dst=8), b"strides"),
                        (dict(F=1 << 26), b"32 bits"), (dict(H=0), b"bad shape")):
            assert fn(*args(**kw)) == -1 and msg in L.npvp_last_error(), (kw, L.npvp_last_error())
        assert fn(*args()) == -1 and b"null buffer" in L.npvp_last_error()
    assert L.npvp_grid_center_pad(*pad_args(rows_out=127)) == -1 and b"rows_out" in L.npvp_last_error()
    assert L.npvp_grid_center_pad(*pad_args(rows_out=1 << 31)) == -1 and b"rows_out" in L.npvp_last_error()


def test_attncfg_with_the_old_arguments_tiles():
    from npvp_amd.ops import AttnCfg
    cfg = AttnCfg(0, 6, 64, 8, 4, 0, 0, 8, 0, 0.0)
    assert cfg.tiles and cfg.grid is None and (cfg.P, cfg.W, cfg.ws) == (64, 8, 4)
    assert AttnCfg.spatial(6, 8, 8, 4, 8, 0.0).tiles
    pad = AttnCfg.spatial(2, 5, 6, 4, 8, 0.0)
    assert not pad.tiles and (pad.P, pad.W) == (64, 8) and pad.pad_args() == (2, 5, 6, 8, 8, 1, 1) and pad.padded_rows == 128
    assert AttnCfg.spatial(2, 5, 6, 7, 8, 0.0).padded_rows == 128         # 98 rows, rounded up to the GEMM's 32


def test_module_returns_the_padded_configuration():
    import npvp_amd
    m = npvp_amd.SpatialLocalMultiheadAttention(512, 8, 4, 0.0)
    assert m._cfg(2, 4, 8, 8).tiles
    cfg = m._cfg(2, 4, 6, 10)
    assert not cfg.tiles and cfg.dim0 == 8 and cfg.pad_args() == (8, 6, 10, 8, 12, 1, 1)


@pytest.mark.parametrize("i", range(len(WC.SLMHSA_CASES)))
def test_fixture_agrees_with_the_cpu_restatement(i):
    """pins the fixture (generated from the reference's own module) and the semantics on the CPU: zero rows are projected to the
    biases and attended as ordinary keys; a key mask would move y by O(1)"""
    golden = GC.load("window_pad")
    got = WC.case_slmhsa_restated(*WC.fixture_case(i))
    for k in WC.SLMHSA_KEYS:
        e = GC.rel_err(WC.view(got[k]), golden[f"c{i}_{k}"])
        assert e < 1e-5, f"case {i} {k}: {e:.3e}"
    C = 512
    assert float(torch.as_tensor(golden[f"c{i}_gb"][2 * C:]).norm()) > 1.0          # the value-bias gradient the pad keys feed
