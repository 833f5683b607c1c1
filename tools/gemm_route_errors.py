"""Summarise the NPVP_ERR_LOG of tests/test_hip_gemm_routes.py: worst whole-tensor rel-L2 and worst row per dispatcher leaf and GEMM
mode, next to the bar each was held to.

    NPVP_ERR_LOG=/tmp/routes.log python -m pytest tests/test_hip_gemm_routes.py -q -m gpu
    python tools/gemm_route_errors.py /tmp/routes.log > profiles/gemm_route_errors.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gemm_route_cases as T  # noqa: E402  (the bars live with the case table)

MODE = {"0": "f32", "4": "bf16x6", "5": "bf16x3", "6": "f16x3"}
LINE = re.compile(r"^ops\[(\d)\] (\S+) (.*) (\S+) row (\S+)$")


def main(path):
    worst = {}
    for line in open(path):
        m = LINE.match(line.rstrip("\n"))
        if not m or " | " not in m.group(3):
            continue
        mode = MODE[m.group(1)]
        parts = m.group(3).split(" | ")
        leaf, case, what = parts[0], parts[1] if len(parts) > 2 else "", parts[-1]
        tol = T.MEAN_TOL if what == "mean" else T.RSTD_TOL if what == "rstd" else T.TOL[mode]
        e, er = float(m.group(4)), float(m.group(5))
        w = worst.setdefault((mode, leaf), [0.0, "", 0.0, "", 0, tol])
        w[4] += 1
        if e / tol > w[0] / w[5]:
            w[0], w[1], w[5] = e, f"{case} / {what}", tol
        if er > w[2]:
            w[2], w[3] = er, f"{case} / {what}"
    print("# tests/test_hip_gemm_routes.py: worst error per dispatcher leaf and GEMM mode against the fp64 product of the same operands")
    print("# (every launch of every case: ragged tiles, padded leading dimensions, all epilogues).  Bars (tests/gemm_route_cases.py): whole-tensor")
    print(f"# rel-L2 {T.TOL['f16x3']:.0e} ({T.TOL['f32']:.0e} for f32 / bf16x3; frame mean {T.MEAN_TOL:.0e}, rstd {T.RSTD_TOL:.0e}), worst row {T.ROW_TOL:.0e}.")
    print(f"# {'mode':7s} {'leaf':24s} {'checks':>6s} {'rel-L2':>10s} {'bar':>8s} {'worst row':>10s}   where")
    bad = 0
    for (mode, leaf), (e, we, er, wr, n, tol) in sorted(worst.items()):
        flag = "" if e < tol and er < T.ROW_TOL else "   ABOVE ITS BAR"
        bad += bool(flag)
        print(f"  {mode:7s} {leaf:24s} {n:6d} {e:10.3e} {tol:8.0e} {er:10.3e}   {we}; row: {wr}{flag}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
