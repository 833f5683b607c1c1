"""CPU: where the parameter-gradient partials of each family lie in its workspace.  The *_reduce_job entry points launch nothing:
they write the 48-byte record that npvp_sum_rows_multi takes (in, out, out_b, nb, stride, ncols, split, accum, mode) to host memory,
so the layout each family's producer, workspace query and reductions share (csrc/partials.h and the one *_partials function per
family) is read here without a device.  Pinned: the records of the shipped shapes; a condition over tools/partials_sweep.py's
lattice: no record reaches past the workspace its query reports."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import partials_sweep as S  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    return S.load(build.build(verbose=False))


@pytest.mark.parametrize("family,shape,nb,ncols,split,mode,offset,nbytes", [
    ("layernorm", (200, 512), 50, 1024, 512, 0, 0, 204800),
    ("frameln", (160, 32768), 16, 65536, 32768, 0, 5120, 4199424),
    ("middle", (160, 2048), 80, 20480, 2048, 1, 0, 10485760),
    ("frameln", (1, 1024), 1, 2048, 1024, 0, 32, 8224)])
def test_the_record_of_a_shipped_shape(L, family, shape, nb, ncols, split, mode, offset, nbytes):
    rc, rec, got_bytes = S.record(L, family, shape, 1)
    assert rc == 0
    assert rec == (offset, S.OUT, S.OUT_B, nb, ncols, ncols, split, 1, mode)
    assert got_bytes == nbytes
    if family != "middle":                                         # (the middle's queued form always accumulates)
        assert S.record(L, family, shape, 0)[1] == rec[:7] + (0, mode)


def test_the_depthwise_weight_gradient_workspace(L):
    assert L.npvp_dwconv3x3_wgrad_workspace_bytes(160, 2048) == 13107200


@pytest.mark.parametrize("family,good,empty", [("layernorm", (200, 512), (0, 512)), ("frameln", (160, 32768), (0, 32768)),
                                               ("middle", (160, 2048), (0, 2048))])
def test_bad_arguments_are_refused(L, family, good, empty):
    assert S.record(L, family, empty, 1)[0] == -1                  # no rows / no frames
    assert S.record(L, family, good, 1, ws=None)[0] == -1          # no workspace
    assert S.record(L, family, good, 1, job=False)[0] == -1        # nowhere to write the record
    assert S.record(L, family, good, 1)[0] == 0


def test_no_record_reaches_past_its_workspace(L):
    """a condition, not a measurement: in offset + nb * stride * 4 <= the family's workspace bytes, over the sweep's lattice"""
    checked, bad = 0, []
    for family, shape, acc, has_ws, has_job in S.cases():
        rc, rec, nbytes = S.record(L, family, shape, acc, S.WS if has_ws else None, has_job)
        assert (rc == 0) == (has_ws and has_job and shape[0] > 0), (family, shape)
        if rc == 0:
            checked += 1
            if not (rec[0] >= 0 and rec[3] >= 1 and rec[4] >= rec[5] and rec[0] + rec[3] * rec[4] * 4 <= nbytes):
                bad.append((family, shape, rec, nbytes))
    assert checked > 1255 and not bad, bad[:5]
