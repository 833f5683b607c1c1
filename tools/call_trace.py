"""GPU: a fingerprint of the library calls the autograd glue makes.  Every bound entry point of npvp_amd._lib.lib() is replaced by
a recorder; fixed-seed cases of tests/golden_cases.py run under the three scheduling modes that select the three arms of
ops._reduce_partials, plus one GraphedTrainStep capture; one step with 4 096 decoder token rows - where the fp16 weight-gradient
kernel, the chained split-K reductions and the fused dgrad + weight-gradient launch run - under those modes and the knobs of the
linear backward (LINEAR_MODES); per case the number of calls and a SHA-256 over the sequence of (entry
point, every scalar argument; an address reduced to null / non-null) are printed.  Two trees that print the same lines make the
same calls with the same arguments in the same order: run it before and after a change of npvp_amd/ops.py that is meant to move none.

    python tools/call_trace.py [--dump DIR]        # DIR: one file per case, one line per call
"""
import argparse
import ctypes
import gc
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402
import npvp_amd as impl  # noqa: E402
from npvp_amd import _lib, ops  # noqa: E402
import golden_cases as GC  # noqa: E402

DEV = "cuda:0"
CALLS = []
# (gradient stream, ReduceQueue) -> the arm of the partial-sum dispatch: queue job / closure on the gradient stream / inline
MODES = {"default": (True, True), "closure": (True, False), "inline": (False, False)}
FAMILIES = ("npvp_layernorm_bwd_reduce", "npvp_frameln_act_bwd_reduce", "npvp_mlpdw_mid_bwd_reduce")
JOB = {f + "_job" for f in FAMILIES}
DIRECT = {FAMILIES[0], FAMILIES[1], FAMILIES[2] + "_into"}
# shape queries answered on the host and remembered per shape by the glue: WHEN one is first asked is no property of the launch sequence
QUERIES = {"npvp_gemm_kernel_id", "npvp_gemm_workspace_bytes", "npvp_linear_bwd_f16_takes", "npvp_wgrad_f16_chainable",
           "npvp_wgrad_f16_chain_workspace_bytes"}
# the knobs of the linear backward, beside (gradient stream, ReduceQueue) of MODES: fused beside a gradient stream, chain, range guard
LINEAR_MODES = {"fused": dict(with_gradient_stream=True), "nochain": dict(chain=False), "strict": dict(strict=True),
                "fallback": dict(fallback=True)}
LINEAR_CALLS = ("npvp_linear_bwd_f16_skip", "npvp_wgrad_f16_chained_skip", "npvp_splitk_reduce_job", "npvp_splitk_reduce_multi")    # (the glue's one call per launch site)


def install():
    L = _lib.lib()
    for name, (_, argtypes) in _lib.SIGNATURES.items():
        if name in QUERIES:
            continue

        def rec(*a, _f=getattr(L, name), _n=name, _t=argtypes):
            CALLS.append((_n,) + tuple(bool(getattr(v, "value", v)) if t is ctypes.c_void_p else (float(v) if t is ctypes.c_float else int(v))
                                       for v, t in zip(a, _t)))
            return _f(*a)
        setattr(L, name, rec)


def graphed_step():
    m = GC._small_predictor(impl, False, 101, DEV)
    m.train()
    past, fut = GC.O.synth_features((2, 3, 512, 8, 8), 92).to(DEV), GC.O.synth_features((2, 4, 512, 8, 8), 93).to(DEV)
    step = impl.GraphedTrainStep(m, make_opt(m), past, fut, 0.01, 1e-6, 1.0, warmup=1)
    step(past, fut, lr=1e-4)


def shard_step():
    """the step of tests/test_hip_golden.py::test_chained_split_k_reductions_are_bit_identical: forward, backward, join"""
    N, To, Tp = 8, 2, 8
    past, fut = GC.O.synth_features((N, To, 512, 8, 8), 92).to(DEV), GC.O.synth_features((N, Tp, 512, 8, 8), 93).to(DEV)
    m = GC._small_predictor(impl, False, 101, DEV, To=To, Tp=Tp, dropout=0.1, drop_path=0.1)
    m.train()
    opt = make_opt(m)
    ops.rng.manual_seed(777, torch.device(DEV))
    ops.rng.begin_step(torch.device(DEV))
    opt.zero_grad()
    (m(past) - fut).abs().mean().backward()
    ops.WgradStream.join()


def make_opt(m):
    return impl.FlatAdamW(m, lr=1e-4, clip_module=m.transformer, max_grad_norm=1.0)


def cases():
    inst = types.SimpleNamespace(**vars(impl))          # the same modules, every positional fuser built as 'instance'
    inst.PosFeatFuser = lambda C, norm: impl.PosFeatFuser(C, "instance")
    return [("train_step_D", lambda: GC.case_train_step(impl, DEV, "D", make_opt=make_opt)),
            ("train_step_S", lambda: GC.case_train_step(impl, DEV, "S", make_opt=make_opt)),
            ("block_dec", lambda: GC.case_block_dec(impl, DEV)), ("block_enc", lambda: GC.case_block_enc(impl, DEV)),
            ("posfuse_layer", lambda: GC.case_posfuse(impl, DEV)), ("posfuse_instance", lambda: GC.case_posfuse(impl, DEV, "instance")),
            ("block_dec_instance", lambda: GC.case_block_dec(inst, DEV)), ("mlpdwbn", lambda: GC.case_mlpdwbn(impl, DEV))]


def run(mode, name, fn, dump):
    gc.collect()                # (models of earlier cases: their weight planes would be re-split with the next optimiser step)
    del CALLS[:]
    ops.rng.manual_seed(9, torch.device(DEV))
    torch.manual_seed(3)
    fn()
    torch.cuda.synchronize()
    lines = [repr(c) for c in CALLS]
    print(f"{mode:8s} {name:20s} calls {len(lines):6d}  sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}", flush=True)
    if dump:
        with open(os.path.join(dump, f"{mode}.{name}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    # (job form, direct form, neither: a LayerNorm backward told to accumulate into the gradient slices itself)
    return [sum(c[0] in JOB for c in CALLS), sum(c[0] in DIRECT for c in CALLS), sum(c[0] == "npvp_layernorm_bwd" and c[14] == 1 for c in CALLS)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--dump", help="write the call sequences into this directory")
    a = ap.parse_args()
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
    install()
    for mode, (grad_stream, queue) in MODES.items():
        ops.WgradStream.enabled, ops.ReduceQueue.enabled = grad_stream, queue
        arms = [sum(col) for col in zip(*[run(mode, name, fn, a.dump) for name, fn in cases()])]
        print(f"{mode:8s} dispatch arms hit: job {arms[0]}, direct {arms[1]}, accumulated in the kernel {arms[2]}", flush=True)
        want = {"default": (True, False, False), "closure": (False, True, False), "inline": (False, True, True)}[mode]
        assert tuple(n > 0 for n in arms) == want, (mode, arms)
    ops.WgradStream.enabled = ops.ReduceQueue.enabled = True
    run("graph", "graphed_step_D", graphed_step, a.dump)
    hit = dict.fromkeys(LINEAR_CALLS, 0)
    for mode, knobs in list(MODES.items()) + list(LINEAR_MODES.items()):
        ops.WgradStream.join()
        ops.WgradStream.enabled, ops.ReduceQueue.enabled = knobs if isinstance(knobs, tuple) else (True, True)
        k = dict(with_gradient_stream=False, chain=True, strict=False, fallback=False)
        k.update({} if isinstance(knobs, tuple) else knobs)
        ops.FusedLinearBwd.with_gradient_stream, ops.WgradChain.enabled, ops.RangeGuard.strict = k["with_gradient_stream"], k["chain"], k["strict"]
        ops.RangeGuard.reset()
        ops.RangeGuard.fallback = k["fallback"]
        run(mode, "shard_step", shard_step, a.dump)
        for n in LINEAR_CALLS:
            hit[n] += sum(c[0] == n for c in CALLS)
    ops.RangeGuard.reset()
    ops.WgradStream.enabled = ops.ReduceQueue.enabled = ops.WgradChain.enabled = True
    ops.FusedLinearBwd.with_gradient_stream = ops.RangeGuard.strict = False
    print("linear backward calls over the shard_step modes: " + ", ".join(f"{n} {hit[n]}" for n in LINEAR_CALLS), flush=True)
    assert all(hit.values()), hit


if __name__ == "__main__":
    main()
