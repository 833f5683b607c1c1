"""Are the kernels of two builds the same kernels?  Compares two gfx950 assembly files of one translation unit, kernel by kernel:

    hipcc -O3 -fPIC -std=c++17 --offload-arch=gfx950 -fno-gpu-rdc --cuda-device-only -S npvp_amd/csrc/gemm.hip -o new.s
    (the same on the other tree -> old.s)
    python tools/asm_kernel_diff.py old.s new.s

Comments and .file / .loc / .cfi directives are dropped; labels lose the number of the function's position in the file (.LBB7_4 ->
.LBB_4) and the compilation-unit id its hash, so that a moved template instantiation or an edit of host code does not show.  Every
function body and every .amdhsa_kernel descriptor block is compared under its own symbol, the metadata (kernel arguments, registers,
LDS) as a sorted set of lines.  Prints the number of differing symbols; exit status 1 if any."""
import re
import sys


def symbols(path):
    out, cur = {}, None
    for line in open(path):
        t = re.sub(r"\s*;.*$", "", line.rstrip("\n")).strip()
        if not t:
            continue
        t = re.sub(r"\.L(BB|func_begin|func_end|JTI)\d+", r".L\1", t)
        t = re.sub(r"__hip_cuid_\w+", "__hip_cuid", t)
        if t.startswith((".file", ".loc", ".cfi", ".ident", ".Ltmp", ".Lfunc")):
            continue
        if t.startswith(".amdgpu_metadata"):
            cur = "[metadata]"
        elif t.startswith(".amdhsa_kernel "):
            cur = t.split()[1] + " [descriptor]"
        elif t.startswith((".section", ".text")):           # the preamble of whatever comes next belongs to nobody
            cur = None
            continue
        elif re.match(r"^[A-Za-z_]\w*:$", t):
            cur = t[:-1]
        elif cur:
            out[cur].append(t)
            continue
        else:
            continue
        out[cur] = []
    out["[metadata]"] = sorted(out.get("[metadata]", []))       # (kernel entries follow the order of instantiation)
    return out


def main():
    a, b = symbols(sys.argv[1]), symbols(sys.argv[2])
    names = sorted(set(a) | set(b))
    diff = [n for n in names if a.get(n) != b.get(n)]
    kernels = [n for n in names if n.endswith(" [descriptor]")]
    print(f"{sys.argv[1]} vs {sys.argv[2]}: {len(kernels)} kernels, {len(names)} symbols, {sum(map(len, a.values()))} / "
          f"{sum(map(len, b.values()))} lines compared, differing symbols: {len(diff)}")
    for n in diff:
        print(f"  DIFFERS {n}: {len(a.get(n, []))} / {len(b.get(n, []))} lines")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
