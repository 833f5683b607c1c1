"""The reference side of the one-term fp16 arithmetic ("f16x1", precision 7 of npvp_gemm_f32): what the kernels must compute, written
without them.  Plain helpers; tests/test_f16x1_host.py checks them on the CPU, tests/test_hip_f16x1.py holds the GPU against them.

r11(x) rounds to 11 significant bits, ties to even - the value of "scale by a power of two, convert to fp16, scale back" wherever
the scaled number is a NORMAL fp16 (the kernels scale by the tensor's amax, or in the row guard's second pass by the row's, so that
it is), with no exponent range of its own.  The product the kernels must deliver is the fp64 product of the r11-rounded operands;
what is left between the two is the fp32 accumulation, which the suite's own bars (gemm_route_cases.TOL / ROW_TOL) bound.

rounded_gemms() is the same rounding applied to a whole model on the CPU: inside it F.linear and the 1 x 1 F.conv2d round input and
weight with r11 when the call has ROWS_MIN token rows or more (the device keeps smaller GEMMs in the two-term arithmetic: the fp16
kernels take 128 rows or more).  Run on the float64 oracle it gives the deviation the arithmetic itself causes, e_emu, a
reference-side number the sampler's test bounds the device's deviation with."""
import contextlib

import torch
import torch.nn.functional as F

# The fp64 product of r11-rounded N(0,1) operands and N(0,1)/sqrt(K) weights against the exact fp64 product: 2.9e-4 rel-L2, per row
# 2.1e-4 .. 4.0e-4 (256 x 32 x 256, 256 x 512 x 256, 384 x 2048 x 512).  A single one-term GEMM therefore lies in [FLOOR, CEIL] of the
# UNROUNDED product - 3 x either side -, and a two-term (f16x3) result, at <= 1e-5, fails the floor.
ONE_TERM_REL = 2.9e-4
FLOOR, CEIL = 1e-4, 1e-3
ROWS_MIN = 128
# the small stochastic predictor of golden_cases (2 + 2 blocks, float64, CPU): e_emu was measured at 8.97e-4 with 71 rounded GEMMs
# (1.09e-3 with 203 at 4 + 8 blocks); the bracket the host test holds it in
EMU_LO, EMU_HI = 3e-4, 3e-3


def r11(x):
    """x (any float dtype) -> float64, rounded to 11 significant bits, ties to even"""
    m, e = torch.frexp(x.double())
    return torch.ldexp(torch.round(m * 2048) / 2048, e)


def rel(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Rounded:
    """state of one rounded_gemms() block: `count` = GEMMs rounded so far"""
    count = 0


@contextlib.contextmanager
def rounded_gemms(rows_min=ROWS_MIN):
    """F.linear and 1 x 1 F.conv2d with r11-rounded input and weight (bias untouched) for calls of `rows_min` token rows or more; every
    other call, and everything outside the block, is the original function.  Operands keep their dtype (float64 models: exact)."""
    lin0, conv0 = F.linear, F.conv2d
    st = Rounded()

    def lin(x, w, b=None):
        if x.numel() // x.shape[-1] >= rows_min:
            st.count += 1
            return lin0(r11(x).to(x.dtype), r11(w).to(w.dtype), b)
        return lin0(x, w, b)

    def conv(x, w, b=None, *a, **k):
        if w.shape[-1] == 1 and w.shape[-2] == 1 and w.shape[1] == x.shape[1] and x.numel() // x.shape[1] >= rows_min:
            st.count += 1
            return conv0(r11(x).to(x.dtype), r11(w).to(w.dtype), b, *a, **k)
        return conv0(x, w, b, *a, **k)

    F.linear, F.conv2d = lin, conv
    try:
        yield st
    finally:
        F.linear, F.conv2d = lin0, conv0


def emulated_deviation(model, run):
    """run(model) -> tensor, evaluated plain and inside rounded_gemms(): (rel-L2 of the rounded result against the plain one, the
    plain result, the rounded result, GEMMs rounded)"""
    with torch.no_grad():
        y0 = run(model)
        with rounded_gemms() as st:
            y1 = run(model)
    return rel(y1, y0), y0, y1, st.count
