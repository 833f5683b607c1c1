"""CPU: where the weight gradient of a linear layer goes is decided by two pure functions of npvp_amd.ops - linear_bwd_plan when the
layer's backward runs, wgrad_plan when the weight-gradient launch is enqueued.  Both are checked against a hand-written table; the
built library answers the shape queries (no device).  The shape facts the table rests on are asserted first, so that a change of
the C planner shows up as that and not as a plan failure."""
import pytest

# (R, N, K): fp16 weight-gradient kernel (id 6), chainable, the library's fused launch takes it
SHAPE_FACTS = {
    (1024, 128, 128): (6, True, True),
    (1040, 128, 128): (6, False, False),        # one split: nothing to hand on
    (1008, 512, 512): (1, False, False),
    (1056, 520, 264): (6, True, False),
    (16448, 512, 512): (6, True, True),         # ... but more rows than FusedLinearBwd.MAX_ROWS
    (114688, 512, 512): (6, True, False),       # (its dgrad runs on the 128 x 256 tiles)
}
S = (1024, 128, 128)

# name, shape, facts that differ from the defaults (precision 6, matching sink, unit strides, planes, guard quiet, chain and fused
# enabled, no gradient stream, no listener, no mask, outside the flush), expected fields of linear_bwd_plan, of wgrad_plan
TWO = dict(fused=False, reduction=None)
HERE = dict(TWO, sunk=True, on_grad_stream=False, urgent=False, fill_slots=True)
TABLE = [
    ("no gradient stream", S, {}, dict(fused=True, reduction="chained"), None),
    ("gradient stream", S, dict(grad_stream=True), dict(TWO, sunk=True, on_grad_stream=True, urgent=False, fill_slots=True),
     dict(route="gemm", precision=None, watch=True)),
    ("gradient stream, inside the flush", S, dict(grad_stream=True, in_flush=True), dict(TWO, sunk=True, on_grad_stream=True),
     dict(route="chained", precision=None, watch=True)),
    ("gradient stream, fused beside it", S, dict(grad_stream=True, fused_with_stream=True), dict(fused=True, reduction="queued"), None),
    ("fused off", S, dict(fused_on=False), HERE, dict(route="chained", precision=None, watch=True)),
    ("fused off, data-parallel listener", S, dict(fused_on=False, listener=True), HERE, dict(route="gemm", precision=None, watch=True)),
    ("fused off, chain off", S, dict(fused_on=False, chain_on=False), HERE, dict(route="gemm", precision=None, watch=True)),
    ("no matching sink", S, dict(sunk=False), dict(TWO, sunk=False, on_grad_stream=False, urgent=False, fill_slots=False),
     dict(route="gemm", precision=None, watch=True)),
    ("no matching sink, gradient stream, in a flush", S, dict(sunk=False, grad_stream=True, in_flush=True),
     dict(TWO, sunk=False, on_grad_stream=False, fill_slots=False), dict(route="gemm", precision=None, watch=True)),
    ("fallback", S, dict(fallback=True), HERE, dict(route="gemm", precision=4, watch=False)),
    ("fallback, row-group mask", S, dict(fallback=True, masked=True), HERE, dict(route="chained", precision=None, watch=True)),
    ("strict", S, dict(strict=True), HERE, dict(route="strict", watch=True)),
    ("strict, row-group mask", S, dict(strict=True, masked=True), HERE, dict(route="chained", precision=None, watch=True)),
    ("inner stride of dy not 1", S, dict(unit_strides=False), HERE, dict(route="gemm", precision=None, watch=True)),
    ("no D-planes", S, dict(planes=False), HERE, dict(route="chained", precision=None, watch=True)),
    ("bf16x6", S, dict(precision=4), dict(HERE, fill_slots=False), dict(route="gemm", precision="WGRAD_PRECISION", watch=False)),
    ("one split", (1040, 128, 128), {}, HERE, dict(route="gemm", precision=None, watch=True)),
    ("not the fp16 kernel", (1008, 512, 512), {}, dict(HERE, fill_slots=False), dict(route="gemm", precision=None, watch=False)),
    ("dgrad shape the fused launch leaves", (1056, 520, 264), {}, HERE, dict(route="chained", precision=None, watch=True)),
    ("more rows than MAX_ROWS", (16448, 512, 512), {}, HERE, dict(route="chained", precision=None, watch=True)),
    ("large GEMM beside a gradient stream", (114688, 512, 512), dict(grad_stream=True),
     dict(TWO, sunk=True, on_grad_stream=True, urgent=True, fill_slots=True), dict(route="gemm", precision=None, watch=True)),
]


@pytest.fixture(scope="module")
def ops():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd import ops
    return ops


def test_shape_facts(ops):
    from npvp_amd._lib import lib
    for (R, N, K), (kid, chainable, fused) in SHAPE_FACTS.items():
        assert ops._gemm_kernel_id(0, 0, N, K, R, 6, False) == kid, (R, N, K)
        assert bool(lib().npvp_wgrad_f16_chainable(N, K, R)) == chainable, (R, N, K)
        assert bool(lib().npvp_linear_bwd_f16_takes(R, N, K)) == fused, (R, N, K)
    assert ops.FusedLinearBwd.takes(*S) and not ops.FusedLinearBwd.takes(16448, 512, 512)
    assert not ops.FusedLinearBwd.takes(1056, 520, 264)


@pytest.mark.parametrize("name,shape,facts,want_bwd,want_wgrad", TABLE, ids=[t[0] for t in TABLE])
def test_plan_table(ops, name, shape, facts, want_bwd, want_wgrad):
    f = dict(precision=6, sunk=True, grad_stream=False, fallback=False, strict=False, unit_strides=True, planes=True, fused_on=True,
             fused_with_stream=False, listener=False, chain_on=True, masked=False, in_flush=False)
    f.update(facts)
    R, N, K = shape
    bwd = ops.linear_bwd_plan(R, N, K, f["precision"], f["sunk"], f["grad_stream"], guard_quiet=not (f["fallback"] or f["strict"]),
                              unit_strides=f["unit_strides"], planes=f["planes"], fused_on=f["fused_on"],
                              fused_with_stream=f["fused_with_stream"], max_rows=ops.FusedLinearBwd.MAX_ROWS)
    for k, v in want_bwd.items():
        assert getattr(bwd, k) == v, (name, k, bwd)
    assert (want_wgrad is None) == bwd.fused, (name, bwd)         # a fused launch has no weight-gradient launch of its own
    if want_wgrad is not None:
        wg = ops.wgrad_plan(N, K, R, f["precision"], ops.WGRAD_PRECISION, bwd.sunk, f["masked"], f["fallback"], f["strict"], f["in_flush"],
                            f["grad_stream"], f["listener"], f["chain_on"], f["unit_strides"])
        for k, v in want_wgrad.items():
            assert getattr(wg, k) == (ops.WGRAD_PRECISION if v == "WGRAD_PRECISION" else v), (name, k, wg)
