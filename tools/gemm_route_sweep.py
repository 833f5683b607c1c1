"""CPU: a fingerprint of the GEMM dispatcher's plan.  Walks a lattice of (a_kc, b_kc, M, N, K, precision, has_planes, plain_epilogue)
and prints the number of tuples and a SHA-256 over (tuple, the four words of npvp_gemm_route, npvp_gemm_kernel_id,
npvp_gemm_workspace_bytes).  Two builds of the library that print the same hash plan every launch of the lattice alike: run it before
and after a change of npvp_amd/csrc/gemm*.hip that is meant to move no route.  No device is needed.

    python tools/gemm_route_sweep.py [--lib path/to/libnpvp_hip.so] [--dump lines.txt]
"""
import argparse
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import gemm_route_cases as T  # noqa: E402
from npvp_amd import _lib  # noqa: E402  (the argument types of include/npvp_hip.h; the library is the one --lib names)


def around(values):
    return {v + d for v in values for d in (-4, 0, 4)}


def lattice():
    """(M values, N values, K values): the table's, the shipped layer widths, 4 below / at / 4 above the tile edges (64, 128, 256)
    and, for M, the row counts at which an [M x 512] output (the model's width: 4 tile columns of 128) reaches the tile counts the
    planners name (64, 128, 256, 512, 768); K: every multiple of 32 up to 4096, then the table's and the shipped token-row counts
    with their +-32 neighbours, the 1024 / 2048 / 32 768 thresholds among them"""
    widths, edges = {128, 512, 2048}, around((64, 128, 256))
    ms = {c["M"] for c in T.CASES} | widths | edges | around(t * 128 // 4 for t in (64, 128, 256, 512, 768))
    ns = {c["N"] for c in T.CASES} | widths | edges
    rows = {c["K"] for c in T.CASES} | {1024, 2048, 4096, 8192, 20480, 32768, 114688}
    ks = set(range(32, 4097, 32)) | {k + d for k in rows for d in (-32, 0, 32) if 0 < k + d <= 114688}
    return sorted(ms), sorted(ns), sorted(ks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "npvp_amd", "libnpvp_hip.so"))
    ap.add_argument("--dump", help="write one line per tuple to this file")
    a = ap.parse_args()
    L = _lib.bind(ctypes.CDLL(a.lib), ("npvp_gemm_workspace_bytes",))
    ms, ns, ks = lattice()
    out = (ctypes.c_int * 4)()
    ref = ctypes.byref(out)
    h, count = hashlib.sha256(), 0
    dump = open(a.dump, "w") if a.dump else None
    for M in ms:
        for N in ns:
            for K in ks:
                ws = L.npvp_gemm_workspace_bytes(M, N, K)
                for a_kc, b_kc in sorted(T.ROLES.values()):
                    for prec in sorted(T.MODES.values()):
                        for planes in (0, 1):
                            kid = L.npvp_gemm_kernel_id(a_kc, b_kc, M, N, K, prec, planes)
                            for plain in (0, 1):
                                rc = L.npvp_gemm_route(a_kc, b_kc, M, N, K, prec, planes, plain, ref)
                                assert rc == 0, (a_kc, b_kc, M, N, K, prec, planes, plain)
                                line = f"{a_kc} {b_kc} {M} {N} {K} {prec} {planes} {plain} | {out[0]} {out[1]} {out[2]} {out[3]} | {kid} {ws}\n"
                                h.update(line.encode())
                                count += 1
                                if dump:
                                    dump.write(line)
    if dump:
        dump.close()
    print(f"{len(ms)} M x {len(ns)} N x {len(ks)} K values, {count} tuples, sha256 {h.hexdigest()}")


if __name__ == "__main__":
    main()
