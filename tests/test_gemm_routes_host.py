"""CPU: tests/gemm_route_cases.py covers the GEMM dispatcher.  npvp_gemm_route (a pure function of the built library, no device)
must send every case of the table to the leaf the table names, and the table must reach every leaf - at a ragged row tile and
a ragged column tile wherever the leaf's tile can be ragged, and with an odd and an even number of K-steps per split on the two
hand-pipelined weight-gradient kernels.  A routing threshold that moves a shape to another leaf fails here, with the leaf's name."""
import ctypes

import pytest

import gemm_route_cases as T


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    from npvp_amd._lib import lib
    build.build(verbose=False)
    return lib()


def route_of(L, case, plain=1):
    out = (ctypes.c_int * 4)()
    a_kc, b_kc = T.ROLES[case["role"]]
    rc = L.npvp_gemm_route(a_kc, b_kc, case["M"], case["N"], case["K"], T.MODES[case["mode"]], int(case["planes"]), plain,
                           ctypes.addressof(out))
    assert rc == 0, L.npvp_last_error()
    return tuple(out)


def uncovered(cases, routes):
    """-> the list of coverage conditions the (cases, their routes) leave open, each naming its leaf / kernel"""
    hit, ragged_m, ragged_n, parities = set(), set(), set(), {k: set() for k in T.BOTH_PARITIES}
    for c, r in zip(cases, routes):
        leaf = T.leaf_of(c["mode"], c["role"], c["planes"], c.get("rowstats", False), r)
        tm, tn = T.LEAVES[leaf][1]
        hit.add(leaf)
        if c["M"] % tm:
            ragged_m.add(leaf)
        if c["N"] % tn:
            ragged_n.add(leaf)
        if r[0] in parities:
            parities[r[0]].add(r[3] % 2)
    missing = []
    for leaf, (_, _, can_m, can_n) in T.LEAVES.items():
        if leaf not in hit:
            missing.append(f"leaf '{leaf}' is reached by no case")
            continue
        if can_m and leaf not in ragged_m:
            missing.append(f"leaf '{leaf}' has no case with a ragged row tile")
        if can_n and leaf not in ragged_n:
            missing.append(f"leaf '{leaf}' has no case with a ragged column tile")
    for kid, name in T.BOTH_PARITIES.items():
        for par, word in ((1, "odd"), (0, "even")):
            if par not in parities[kid]:
                missing.append(f"{name} has no case with an {word} number of K-steps per split")
    return missing


@pytest.mark.parametrize("case", T.CASES, ids=[c["name"] for c in T.CASES])
def test_case_takes_the_route_the_table_names(L, case):
    r = route_of(L, case)
    kid, variant, cls, parity = case["route"]
    assert (r[0], r[1]) == (kid, variant), f"kernel id / variant {r[:2]}, the table says {(kid, variant)}"
    assert T.split_class(r[0], r[2]) == cls, f"{r[2]} splits, the table says class {cls}"
    assert ("odd" if r[3] % 2 else "even") == parity, f"{r[3]} K-steps per split, the table says {parity}"
    assert r[2] * r[3] * (32 if r[0] == 0 else 16) == case["K"]
    assert T.leaf_of(case["mode"], case["role"], case["planes"], case.get("rowstats", False), r) == case["leaf"]
    assert case["leaf"] in T.LEAVES
    assert case["M"] % 4 == 0 and case["N"] % 4 == 0 and case["K"] % 32 == 0


def test_the_table_covers_every_leaf(L):
    """zero uncovered leaves: a condition, not a measurement"""
    missing = uncovered(T.CASES, [route_of(L, c) for c in T.CASES])
    assert not missing, "\n".join(missing)
    assert len({c["name"] for c in T.CASES}) == len(T.CASES)


@pytest.mark.parametrize("leaf", ["f16 v3", "wgrad wide >8", "db3<pre> dgrad", "wgrad f16 1", "f32<0,0> split"])
def test_the_closure_check_names_a_leaf_that_lost_its_cases(L, leaf):
    rest = [c for c in T.CASES if c["leaf"] != leaf]
    assert len(rest) < len(T.CASES)
    missing = uncovered(rest, [route_of(L, c) for c in rest])
    assert any(f"'{leaf}'" in m for m in missing), missing


def test_the_closure_check_sees_a_lost_parity_and_a_lost_ragged_edge(L):
    rest = [c for c in T.CASES if not (c["leaf"].startswith("wgrad wide") and c["route"][3] == "odd")]
    assert any("gemm_wgrad_wide_kernel has no case with an odd" in m for m in uncovered(rest, [route_of(L, c) for c in rest]))
    rest = [c for c in T.CASES if not (c["leaf"] == "wide v1")] + [dict(T.CASES[0], mode="bf16x6", role="fwd", M=6016, N=2056, K=64, planes=True)]
    assert "leaf 'wide v1' has no case with a ragged row tile" in uncovered(rest, [route_of(L, c) for c in rest])


def test_kernel_id_is_the_first_word_of_the_route(L):
    """npvp_gemm_kernel_id answers what it always answered: pinned for the shapes tests/test_abi.py names and for the shipped
    layer shapes, and equal to the route's kernel id (plain epilogue) over the whole table, with and without planes"""
    assert L.npvp_gemm_kernel_id(1, 1, 114688, 512, 512, 6, 1) == 5 and L.npvp_gemm_kernel_id(1, 1, 8192, 512, 512, 6, 0) == 1
    pinned = {(1, 1, 20480, 2048, 512, 4, 1): 2, (1, 1, 20480, 512, 512, 4, 1): 1, (1, 1, 8192, 512, 512, 4, 1): 4,
              (0, 0, 512, 512, 114688, 4, 0): 3, (0, 0, 512, 512, 20480, 4, 0): 1, (0, 0, 512, 512, 8192, 6, 0): 6,
              (1, 0, 8192, 512, 2048, 6, 1): 7, (1, 1, 2048, 512, 512, 6, 1): 7, (1, 1, 64, 512, 512, 6, 1): 1,
              (1, 1, 20480, 512, 512, 0, 1): 0, (0, 0, 512, 512, 114688, 5, 0): 1}
    for args, kid in pinned.items():
        assert L.npvp_gemm_kernel_id(*args) == kid, args
    out = (ctypes.c_int * 4)()
    for c in T.CASES:
        for role, (a_kc, b_kc) in T.ROLES.items():
            for prec in T.MODES.values():
                for planes in (0, 1):
                    assert L.npvp_gemm_route(a_kc, b_kc, c["M"], c["N"], c["K"], prec, planes, 1, ctypes.addressof(out)) == 0
                    assert out[0] == L.npvp_gemm_kernel_id(a_kc, b_kc, c["M"], c["N"], c["K"], prec, planes), (role, c["name"], prec, planes)
    # an epilogue keeps a launch off the split-K and weight-gradient kernels (the dispatcher's `plain`)
    assert L.npvp_gemm_route(0, 0, 512, 512, 8192, 6, 0, 0, ctypes.addressof(out)) == 0 and tuple(out) == (1, 0, 1, 512)
    assert L.npvp_gemm_route(0, 0, 512, 512, 8192, 6, 0, 1, ctypes.addressof(out)) == 0 and tuple(out) == (6, 0, 32, 16)
    assert L.npvp_gemm_route(1, 1, 128, 128, 33, 4, 0, 1, ctypes.addressof(out)) == -1
    assert L.npvp_gemm_route(1, 1, 128, 128, 32, 4, 0, 1, None) == -1
