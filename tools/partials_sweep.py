"""A fingerprint of the parameter-gradient partials: where each family's partial rows lie in its workspace and how they are summed.

CPU part (default; no device needed: the *_reduce_job entry points launch nothing and write their 48-byte record to host memory).
Walks a lattice of shapes and prints the number of tuples and a SHA-256 over (return code, the record with `in` as an offset from
the workspace argument, the four *_workspace_bytes queries).  Two builds of the library that print the same line lay every set of
partials out alike: run it before and after a change of npvp_amd/csrc that is meant to move none.

--device: for one shape of each class of the sum-rows plan, fills a workspace from a fixed seed, sums it with the direct form
(*_reduce, npvp_mlpdw_mid_bwd_reduce_into) and the queued form (*_reduce_job + npvp_sum_rows_multi, one job per call and all jobs
in one call), accumulate off and on, and prints a SHA-256 of the output bytes per (family, shape, form).

    python tools/partials_sweep.py [--lib path/to/libnpvp_hip.so] [--dump lines.txt] [--device]
"""
import argparse
import ctypes
import hashlib
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from npvp_amd import _lib  # noqa: E402  (the argument types of include/npvp_hip.h; the library is the one --lib names)
RECORD = "<QQQiiiiii"                       # in, out, out_b, nb, stride, ncols, split, accum, mode
WS, OUT, OUT_B = 0x7f0000000000, 0x7e0000000000, 0x7d0000000000          # made-up 16-byte aligned addresses: never dereferenced


def load(path):
    return _lib.bind(ctypes.CDLL(path), (
        "npvp_layernorm_bwd_workspace_bytes", "npvp_frameln_act_bwd_workspace_bytes", "npvp_mlpdw_mid_bwd_workspace_bytes",
        "npvp_dwconv3x3_wgrad_workspace_bytes", "npvp_layernorm_bwd_reduce_job", "npvp_frameln_act_bwd_reduce_job",
        "npvp_mlpdw_mid_bwd_reduce_job", "npvp_layernorm_bwd_reduce", "npvp_frameln_act_bwd_reduce", "npvp_mlpdw_mid_bwd_reduce",
        "npvp_mlpdw_mid_bwd_reduce_into", "npvp_sum_rows_multi"))


def around(values, d=(-1, 0, 1)):
    return {v + k for v in values for k in d if v + k > 0}


def lattice():
    """(LayerNorm rows, C values, frame counts, per_frame values, Ch values).  Rows: every count up to 4 x 10 (one backward block per
    four rows), around the 252 / 256 rows at which the partial rows reach 64 and the 2048 at which the blocks stop growing, and the
    shipped token-row counts; frames: 1 .. 70, around the chunk thresholds 128 / 256 / 512, and the shipped frame counts."""
    rows = set(range(1, 41)) | around((252, 256, 2048), (-5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5)) | {f * 64 for f in (160, 560, 1792, 2240, 3584)}
    frames = set(range(1, 71)) | around((128, 256, 512), (-2, -1, 0, 1, 2)) | {160, 560, 1792, 2240, 3584}
    return sorted(rows), [256, 512, 768, 1024], sorted(frames), [1024 << k for k in range(8)], [512, 1024, 2048]


def record(L, family, shape, accumulate, ws=WS, job=True):
    """-> (return code, (in offset, out, out_b, nb, stride, ncols, split, accum, mode) or None, workspace bytes of the family)"""
    buf = ctypes.create_string_buffer(48)
    to = ctypes.addressof(buf) if job else None
    if family == "layernorm":
        rc = L.npvp_layernorm_bwd_reduce_job(ws, OUT, OUT_B, shape[0], shape[1], accumulate, to)
        nbytes = L.npvp_layernorm_bwd_workspace_bytes(shape[0], shape[1])
    elif family == "frameln":
        rc = L.npvp_frameln_act_bwd_reduce_job(ws, OUT, OUT_B, shape[0], shape[1], accumulate, to)
        nbytes = L.npvp_frameln_act_bwd_workspace_bytes(shape[0], shape[1])
    else:
        rc = L.npvp_mlpdw_mid_bwd_reduce_job(ws, OUT, OUT_B, shape[0], shape[1], to)
        nbytes = L.npvp_mlpdw_mid_bwd_workspace_bytes(shape[0], shape[1])
    if rc != 0:
        return rc, None, nbytes
    r = struct.unpack(RECORD, buf.raw)
    return rc, (r[0] - ws,) + r[1:], nbytes


def cases():
    """every (family, shape, accumulate, workspace given, job given) of the lattice, the bad-argument cases last"""
    rows, cs, frames, pfs, chs = lattice()
    for r in rows:
        for c in cs:
            for acc in (0, 1):
                yield "layernorm", (r, c), acc, True, True
    for f in frames:
        for pf in pfs:
            for acc in (0, 1):
                yield "frameln", (f, pf), acc, True, True
        for ch in chs:
            yield "middle", (f, ch), 1, True, True
    for family, good, empty in (("layernorm", (200, 512), (0, 512)), ("frameln", (160, 32768), (0, 32768)), ("middle", (160, 2048), (0, 2048))):
        yield family, empty, 1, True, True
        yield family, good, 1, False, True
        yield family, good, 1, True, False


def host_sweep(L, dump=None):
    h, count = hashlib.sha256(), 0
    for family, shape, acc, has_ws, has_job in cases():
        rc, rec, nbytes = record(L, family, shape, acc, WS if has_ws else None, has_job)
        dw = L.npvp_dwconv3x3_wgrad_workspace_bytes(*shape) if family == "middle" else 0
        line = f"{family} {shape[0]} {shape[1]} {acc} {int(has_ws)} {int(has_job)} | {rc} {rec} | {nbytes} {dw}\n"
        h.update(line.encode())
        count += 1
        if dump:
            dump.write(line)
    return count, h.hexdigest()


# one shape (or two) per class of the plan: (family, shape, class)
DEVICE_SHAPES = [("frameln", (160, 32768), "wide float4"), ("frameln", (560, 2048), "wide float4"),
                 ("layernorm", (2048, 512), "16-column"), ("layernorm", (253, 1024), "16-column"), ("middle", (160, 512), "16-column"),
                 ("middle", (160, 1024), "64-column at 1024 threads"), ("middle", (160, 2048), "64-column at 1024 threads"),
                 ("layernorm", (200, 512), "64-column at 256 threads"), ("layernorm", (252, 256), "64-column at 256 threads"),
                 ("frameln", (160, 1024), "64-column at 256 threads")]


def device_sweep(L):
    import torch
    dev = "cuda"
    gen = torch.Generator().manual_seed(20240)
    rnd = lambda n: torch.randn(n, generator=gen).to(dev)
    sha = lambda *ts: hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in ts)).hexdigest()[:32]
    for acc in (0, 1):
        queued = []                                                # (label, job bytes, outputs) of every set, for the one-call form
        for family, shape, cls in DEVICE_SHAPES:
            rc, rec, nbytes = record(L, family, shape, acc)
            assert rc == 0 and rec[0] + rec[3] * rec[4] * 4 <= nbytes, (family, shape, rec, nbytes)
            ws = rnd(nbytes // 4)
            n_out, n_b = (rec[6], rec[5] - rec[6]) if family != "middle" else (9 * shape[1], shape[1])
            base, base_b = rnd(n_out), rnd(n_b)
            label = f"{family} {shape[0]}x{shape[1]} [{cls}] accumulate {acc}"

            def run(form):
                out, out_b, job = base.clone(), base_b.clone(), ctypes.create_string_buffer(48)
                a = (ws.data_ptr(), out.data_ptr(), out_b.data_ptr(), shape[0], shape[1])
                if family == "layernorm":
                    rc = L.npvp_layernorm_bwd_reduce(*a, acc, None) if form == "direct" else L.npvp_layernorm_bwd_reduce_job(*a, acc, ctypes.addressof(job))
                elif family == "frameln":
                    rc = L.npvp_frameln_act_bwd_reduce(*a, acc, None) if form == "direct" else L.npvp_frameln_act_bwd_reduce_job(*a, acc, ctypes.addressof(job))
                elif form == "direct":                             # the middle's two direct forms: [10][Ch] and the Conv2d layout
                    both = torch.cat([base, base_b])
                    rc = L.npvp_mlpdw_mid_bwd_reduce(ws.data_ptr(), both.data_ptr(), shape[0], shape[1], acc, None)
                    rc = rc or L.npvp_mlpdw_mid_bwd_reduce_into(*a, None)
                    out = torch.cat([both, out])
                else:
                    rc = L.npvp_mlpdw_mid_bwd_reduce_job(*a, ctypes.addressof(job))
                assert rc == 0, (label, form, rc)
                if form == "queued":
                    assert L.npvp_sum_rows_multi(ctypes.addressof(job), 1, None) == 0
                torch.cuda.synchronize()
                return job.raw, out, out_b

            _, out, out_b = run("direct")
            print(f"{label} direct  {sha(out, out_b)}")
            _, out, out_b = run("queued")
            print(f"{label} queued  {sha(out, out_b)}")
            queued.append((label, ws) + run("job only"))
        jobs = ctypes.create_string_buffer(b"".join(q[2] for q in queued))
        assert L.npvp_sum_rows_multi(ctypes.addressof(jobs), len(queued), None) == 0
        torch.cuda.synchronize()
        for label, _, _, out, out_b in queued:
            print(f"{label} queued, {len(queued)} jobs in one call  {sha(out, out_b)}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "npvp_amd", "libnpvp_hip.so"))
    ap.add_argument("--dump", help="write one line per tuple of the CPU part to this file")
    ap.add_argument("--device", action="store_true", help="run the device part (needs a GPU) instead of the CPU part")
    a = ap.parse_args()
    if a.device:
        import torch  # noqa: F401  (before the library: both must use the HIP runtime that torch loads)
        return device_sweep(load(a.lib))
    L = load(a.lib)
    dump = open(a.dump, "w") if a.dump else None
    count, digest = host_sweep(L, dump)
    if dump:
        dump.close()
    print(f"{count} tuples, sha256 {digest}")


if __name__ == "__main__":
    main()
