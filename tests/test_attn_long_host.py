"""CPU: the host side of the streaming attention entry points (npvp_attn_long_fwd / npvp_attn_long_bwd /
npvp_attn_long_bwd_workspace_bytes): declared, bound, argument checks before any launch, workspace size - and the guard that the
existing pair still ends at 128."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["npvp_attn_long_fwd", "npvp_attn_long_bwd_workspace_bytes", "npvp_attn_long_bwd"]


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


def test_declared_in_the_header_and_bound():
    from npvp_amd._lib import SIGNATURES, c_ll, c_p
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "npvp_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(npvp_[a-z0-9_]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, f"{n} is not declared in include/npvp_hip.h"
        assert n in SIGNATURES, f"{n} has no signature in npvp_amd/_lib.py"
    # the arguments of the existing pair; backward plus (workspace, ws_bytes) in front of the stream
    assert SIGNATURES["npvp_attn_long_fwd"] == SIGNATURES["npvp_attn_fwd"]
    res, args = SIGNATURES["npvp_attn_bwd"]
    assert SIGNATURES["npvp_attn_long_bwd"] == (res, args[:-1] + [c_p, c_ll] + args[-1:])


def fwd_args(Tq=200, Tk=200, head_dim=64, drop_p=0.0):
    return (None, 512, None, 512, None, 512, None, 512, 1, 1, 64, 8, 0, Tq, Tk, 8, head_dim, 0, drop_p, None, 0, None, None)


def test_argument_errors_do_not_need_a_gpu(L):
    assert L.npvp_attn_long_fwd(*fwd_args(head_dim=32)) == -1 and b"head_dim" in L.npvp_last_error()
    assert L.npvp_attn_long_fwd(*fwd_args(drop_p=0.5)) == -1 and b"dropout" in L.npvp_last_error()       # no seed
    assert L.npvp_attn_long_fwd(*fwd_args(Tq=0)) == -1 and b"at least 1" in L.npvp_last_error()
    a = fwd_args()
    assert L.npvp_attn_long_fwd(*(a[:1] + (510,) + a[2:])) == -1 and b"multiples of 4" in L.npvp_last_error()
    # spatial mode: a window of more than 1024 x 1024 tokens is refused (the window-local row arithmetic of attn_row)
    w = (None, 512, None, 512, None, 512, None, 512, 0, 1, 1025 * 1025, 1025, 1025, 0, 0, 8, 64, 0, 0.0, None, 0, None, None)
    assert L.npvp_attn_long_fwd(*w) == -1 and b"window size must be at most 1024" in L.npvp_last_error()
    # backward: the workspace is checked on the host too
    b = (None, 512, None, 512, None, 512, None, 512, None, 512, None, 512, None, 512, 1, 1, 64, 8, 0, 200, 200, 8, 64, 0, 0.0, None, 0,
         None, None, None)
    assert L.npvp_attn_long_bwd(*b, None, 0, None) == -3 and b"workspace" in L.npvp_last_error()
    assert L.npvp_attn_long_bwd(*(b[:22] + (32,) + b[23:]), None, 0, None) == -1 and b"head_dim" in L.npvp_last_error()


def test_workspace_is_linear_in_the_query_rows_and_independent_of_the_keys(L):
    wsb = L.npvp_attn_long_bwd_workspace_bytes
    base = wsb(1, 1, 64, 8, 0, 200, 200, 8)
    assert base == 3 * 4 * 64 * 8 * 200                              # three statistics per (group, head, query row)
    assert wsb(1, 1, 64, 8, 0, 200, 3, 8) == base and wsb(1, 1, 64, 8, 0, 200, 1000, 8) == base
    assert wsb(1, 2, 64, 8, 0, 200, 200, 8) == 2 * base              # groups
    assert wsb(1, 1, 64, 8, 0, 400, 200, 8) == 2 * base              # L
    assert wsb(1, 1, 64, 8, 0, 200, 200, 4) == base // 2             # heads
    assert wsb(1, 1, 8, 8, 0, 200, 200, 8) == base // 8              # pixels
    # spatial windows: groups = frames x windows, L = ws * ws
    assert wsb(0, 2, 144, 12, 12, 0, 0, 8) == 3 * 4 * 2 * 8 * 144
    assert wsb(0, 1, 288, 24, 12, 0, 0, 8) == 3 * 4 * 2 * 8 * 144


def test_the_existing_entry_points_still_end_at_128(L):
    assert L.npvp_attn_fwd(*fwd_args(Tq=129, Tk=129)) == -1
    assert b"attn: sequence length must be in [1,128]" in L.npvp_last_error()
    assert L.npvp_attn_fwd(*fwd_args(Tq=128, Tk=129)) == -1 and b"[1,128]" in L.npvp_last_error()


def test_ops_routes_at_the_module_constant():
    from npvp_amd import ops
    assert ops.ATTN_LONG_MIN == 129
    assert not ops._attn_long(ops.AttnCfg(1, 1, 64, 8, 0, 128, 128, 8, 0, 0.0))
    assert ops._attn_long(ops.AttnCfg(1, 1, 64, 8, 0, 129, 2, 8, 0, 0.0)) and ops._attn_long(ops.AttnCfg(1, 1, 64, 8, 0, 2, 129, 8, 0, 0.0))
    assert not ops._attn_long(ops.AttnCfg(0, 1, 64, 8, 8, 0, 0, 8, 0, 0.0)) and ops._attn_long(ops.AttnCfg(0, 1, 144, 12, 12, 0, 0, 8, 0, 0.0))
