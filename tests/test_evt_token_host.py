"""CPU: the host side of the learned event token (ref/models/VidHRFormer.py:22-23, 35-42; ref/models/Predictor.py:343-344): the committed
fixtures against the CPU restatement, the wrong readings of the reference's branch told apart, the modules' keys and parameters, the
declarations and argument checks of npvp_evt_token_join / npvp_evt_token_split, and the config switch."""
import functools
import json
import os
import re

import pytest
import torch

import evt_token_cases as EC
import golden_cases as GC
from test_oracle_golden import TOL           # 2e-5: the oracle's blocks against reference-generated vectors, fp32 on the CPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_TOL = 1e-4                               # the bar of tests/test_hip_evt_token.py (test_hip_golden.TOL)


@pytest.fixture(scope="module")
def L():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd._lib import lib
    return lib()


# ------------------------------------------------------------------ the restatement and the fixtures
@functools.lru_cache(maxsize=None)
def _restated_encoder(variant=None):
    return {k: v.detach() for k, v in EC.case_encoder_restated(torch.float32, variant).items()}


def test_encoder_fixture_agrees_with_the_cpu_restatement():
    golden = GC.load("evt_token_encoder")
    got = _restated_encoder()
    errs = {k: GC.rel_err(EC.view(got[k]), golden[k]) for k in EC.ENC_KEYS}
    print(f"evt token encoder, restatement vs fixture: {errs}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < TOL}
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"
    assert float(torch.as_tensor(golden["g_EVT"]).norm()) > 0


@pytest.mark.parametrize("variant", EC.WRONG_VARIANTS)
def test_wrong_readings_are_rejected(variant):
    """each wrong variant misses the reference's event coding by at least 10 x the bar the GPU tests hold the kernels to (the
    prepended token also moves the memory): a fixture comparison at that bar tells them apart"""
    golden = GC.load("evt_token_encoder")
    got = _restated_encoder(variant)
    e_evt, e_mem = GC.rel_err(EC.view(got["evt"]), golden["evt"]), GC.rel_err(EC.view(got["memory"]), golden["memory"])
    print(f"variant {variant}: event coding off by {e_evt:.3e}, memory by {e_mem:.3e}")
    assert e_evt >= 10 * GPU_TOL
    if variant in ("prepend", "no_mask"):
        assert e_mem >= 10 * GPU_TOL
    if variant in ("clip0", "mean_T1", "mean_T", "last_pos"):
        assert e_mem < TOL          # the frames never see the token or its table rows: only the event coding moves


def test_memory_does_not_depend_on_the_token():
    """the frames never see the token (the encoder's temporal mask): the memory is independent of its value, bit for bit"""
    import oracle
    e = EC.ENC
    enc = oracle.VidHRFormerEncoder(e["layers"], EC.H, EC.W, EC.C, 8, 4, 0.0, 0.0, 4, 1024, torch.nn.LayerNorm(EC.C), False)
    EC.fill(enc, e["fill"], e["token"])
    holder = EC._Holder(enc, oracle.PosFeatFuser(EC.C, 'layer'))
    x, beta, gamma, _, _ = EC.encoder_inputs()
    tok = EC.O.seeded_randn((1, EC.H, EC.W, EC.C), e["token"])
    with torch.no_grad():
        m1, e1 = EC.restated_encode(holder, x, (beta, gamma), tok)
        m2, e2 = EC.restated_encode(holder, x, (beta, gamma), 3 * tok + 1)
    assert torch.equal(m1, m2) and GC.rel_err(e2, e1) > 0.1


@pytest.mark.parametrize("variant", ["D", "S"])
def test_predictor_fixture_agrees_with_the_cpu_restatement(variant):
    import oracle
    golden = GC.load(f"predictor_evt_token_{variant}")
    stochastic = variant == "S"
    m = EC.restated_predictor(stochastic, int(golden["meta"][3]))
    got = EC.run_predictor(m, stochastic, *EC.predictor_inputs(), oracle.Div_KL(1e-2))
    keys = EC.PRED_KEYS + (EC.PRED_KEYS_S if stochastic else ())
    assert set(golden) - {"meta"} == set(keys)
    errs = {k: GC.rel_err(EC.view(got[k]), golden[k]) for k in keys}
    print(f"predictor[{variant}] with the token, restatement vs fixture: {errs}")
    bad = {k: f"{e:.3e}" for k, e in errs.items() if not e < TOL}
    assert not bad, f"rel-L2 above {TOL:.1e}: {bad}"


# ------------------------------------------------------------------ the modules
def _stored_keys():
    with open(os.path.join(GC.GOLDEN_DIR, "predictor_evt_token_keys.json")) as f:
        return json.load(f)


def test_state_dict_keys_are_the_references():
    import npvp_amd
    stored = _stored_keys()
    assert len(stored) == 604 and stored == sorted(stored)
    with_token = EC.full_predictor(npvp_amd, True)
    without = EC.full_predictor(npvp_amd, False)
    assert sorted(with_token.state_dict().keys()) == stored
    assert sorted(without.state_dict().keys()) == [k for k in stored if k != "EVT_Former.EVT"] and len(without.state_dict()) == 603
    # the parameter comes first in its module, as in the reference (ref/models/VidHRFormer.py:23): the position of its Adam moments in
    # an optimiser state list written in module.parameters() order
    names = [n for n, _ in with_token.named_parameters()]
    assert names.index("EVT_Former.EVT") == names.index("EVT_Former.layers.0.SLMHSA.attn.in_proj_weight") - 1
    assert [n for n in names if n != "EVT_Former.EVT"] == [n for n, _ in without.named_parameters()]
    p = with_token.EVT_Former.EVT
    assert tuple(p.shape) == (1, 8, 8, 512) and p.requires_grad and 0.9 < float(p.detach().std()) < 1.1          # randn, like the reference


def test_encoder_module_registers_the_token_only_when_asked():
    import npvp_amd
    enc = npvp_amd.VidHRFormerEncoder(1, 8, 8, 512, 8, 4, evt_token=True)
    assert enc.evt_token and tuple(enc.EVT.shape) == (1, 8, 8, 512)
    plain = npvp_amd.VidHRFormerEncoder(1, 8, 8, 512, 8, 4)
    assert not plain.evt_token and not hasattr(plain, "EVT")
    assert set(enc.state_dict()) - set(plain.state_dict()) == {"EVT"}


def test_evt_former_false_still_raises_and_says_why():
    import npvp_amd
    with pytest.raises(NotImplementedError, match=r"(?s)evt_former=False.*permutation.*H = W = 8"):
        EC.build_predictor(npvp_amd, False, evt_former=False)
    with pytest.raises(NotImplementedError, match="evt_former=False"):
        EC.build_predictor(npvp_amd, False, learn_evt_token=True, evt_former=False)


def test_row_count_rule_is_named():
    """6 x 10 tokens per frame, N (T + 1) = 2 * 3 frames: 360 rows are no multiple of 32 - refused before any kernel is reached"""
    import npvp_amd
    enc = npvp_amd.VidHRFormerEncoder(1, 6, 10, 512, 8, 4, evt_token=True)
    x = torch.zeros(2, 2, 6, 10, 512)
    tables = (torch.zeros(2 * 60, 512), None)
    with pytest.raises(ValueError, match=r"N\*\(T\+1\)\*H\*W % 32"):
        enc.forward_canonical(x, tables, npvp_amd.PosFeatFuser(512, 'layer'))


def test_build_predictor_from_cfg_with_and_without_the_key():
    import npvp_amd
    from npvp_amd import trainer
    cfg = trainer.load_config(os.path.join(ROOT, "configs", "config_KTH_VFP_NPVP-S.yaml"), num_past=2, num_future=2)
    P = cfg["Predictor"]
    assert "learn_evt_token" not in P
    small = dict(evt_former_num_layers=1, transformer_layers=1)
    P.update(small)
    assert not trainer.build_predictor_from_cfg(npvp_amd.Predictor, P, 2, 2).EVT_Former.evt_token          # absent means False
    assert trainer.build_predictor_from_cfg(npvp_amd.Predictor, P, 2, 2, learn_evt_token=True).EVT_Former.evt_token
    assert trainer.build_predictor_from_cfg(npvp_amd.Predictor, dict(P, learn_evt_token=True), 2, 2).EVT_Former.evt_token
    assert not trainer.build_predictor_from_cfg(npvp_amd.Predictor, dict(P, learn_evt_token=True), 2, 2,
                                                learn_evt_token=False).EVT_Former.evt_token                  # the override wins


# ------------------------------------------------------------------ the two entry points
NAMES = ["npvp_evt_token_join", "npvp_evt_token_split"]


def test_declared_in_the_header_with_reference_lines_and_bound():
    from npvp_amd._lib import SIGNATURES, c_int, c_ll, c_p
    text = open(os.path.join(ROOT, "include", "npvp_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(npvp_[a-z0-9_]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared and n in SIGNATURES, n
    comment = [c for c in re.findall(r"/\*.*?\*/", text, flags=re.S) if "learned event token" in c]
    assert len(comment) == 1 and "ref/models/VidHRFormer.py:36" in comment[0] and "ref/models/Predictor.py:344" in comment[0]
    assert SIGNATURES["npvp_evt_token_join"] == (c_int, [c_p, c_ll, c_p, c_ll, c_ll, c_p, c_ll] + [c_int] * 4 + [c_p, c_p])
    assert SIGNATURES["npvp_evt_token_split"] == (c_int, [c_p, c_ll, c_p, c_ll, c_p, c_ll] + [c_int] * 4 + [c_p, c_p, c_p])


def join_args(x=None, ld_x=512, token=None, ld_token=512, clip=0, y=None, ld_y=512, N=2, T=2, P=64, C=512):
    return (x, ld_x, token, ld_token, clip, y, ld_y, N, T, P, C, None, None)


def split_args(y=None, ld_y=512, x=None, ld_x=512, last=None, ld_last=512, N=2, T=2, P=64, C=512):
    return (y, ld_y, x, ld_x, last, ld_last, N, T, P, C, None, None, None)


def test_argument_errors_do_not_need_a_gpu(L):
    """every refusal answers before a launch (the buffers are NULL or small integers that are never dereferenced: a call that got past
    its shape and stride checks says "null buffer", or "aligned" for an odd address)"""
    for fn, args in ((L.npvp_evt_token_join, join_args), (L.npvp_evt_token_split, split_args)):
        for kw, msg in ((dict(C=510), b"multiple of 4"), (dict(C=0), b"bad shape"), (dict(T=0), b"bad shape"), (dict(N=-1), b"bad shape"),
                        (dict(N=1 << 20, T=31, P=64), b"32 bits"), (dict(ld_y=514), b"strides"), (dict(ld_y=8), b"strides")):
            assert fn(*args(**kw)) == -1 and msg in L.npvp_last_error(), (kw, L.npvp_last_error())
        assert fn(*args()) == -1 and b"null buffer" in L.npvp_last_error()
    for kw in (dict(x=16, ld_x=510), dict(token=16, ld_token=8), dict(x=16, ld_x=516, y=None, ld_y=516, C=516 + 4)):
        assert L.npvp_evt_token_join(*join_args(**kw)) == -1 and b"strides" in L.npvp_last_error(), kw
    assert L.npvp_evt_token_join(*join_args(token=16, clip=64 * 512 - 4)) == -1 and b"clip stride" in L.npvp_last_error()
    assert L.npvp_evt_token_join(*join_args(token=16, clip=6)) == -1 and b"clip stride" in L.npvp_last_error()
    assert L.npvp_evt_token_join(*join_args(x=16, y=24)) == -1 and b"aligned" in L.npvp_last_error()
    assert L.npvp_evt_token_join(*join_args(x=8, y=32)) == -1 and b"aligned" in L.npvp_last_error()
    assert L.npvp_evt_token_join(*join_args(token=4, y=32)) == -1 and b"aligned" in L.npvp_last_error()
    for kw in (dict(x=16, ld_x=510), dict(last=16, ld_last=8)):
        assert L.npvp_evt_token_split(*split_args(y=16, **kw)) == -1 and b"strides" in L.npvp_last_error(), kw
    assert L.npvp_evt_token_split(*split_args(y=16)) == -1 and b"null buffer" in L.npvp_last_error()          # neither output
    assert L.npvp_evt_token_split(*split_args(y=16, x=24)) == -1 and b"aligned" in L.npvp_last_error()
    assert L.npvp_evt_token_split(*split_args(y=16, last=20)) == -1 and b"aligned" in L.npvp_last_error()


@pytest.mark.parametrize("N, T, P, C", [(EC.ENC["N"], EC.ENC["T"], 64, 512), (1, EC.ENC["T"], 64, 512), (EC.PRED["N"], EC.PRED["Tp"], 64, 512),
                                        (2, 32, 16, 512)])
def test_shapes_of_the_cases_meet_the_predicates_on_both_sides(L, N, T, P, C):
    """the launches of the fixture cases (features with the token, a table with N = 1, the generic-route case): contiguous fp32 rows of
    C floats meet C % 4, stride and 32-bit row-count predicates of the join (x, token -> y) and of the split (y -> x, last) - with NULL
    buffers both entry points get as far as their null-buffer check, the one that follows the shape checks"""
    assert C % 4 == 0 and N * (T + 1) * P < 1 << 31 and N * (T + 1) * P % 32 == 0
    assert L.npvp_evt_token_join(*join_args(N=N, T=T, P=P, C=C, ld_x=C, ld_token=C, ld_y=C, clip=P * C)) == -1
    assert b"null buffer" in L.npvp_last_error()
    assert L.npvp_evt_token_split(*split_args(N=N, T=T, P=P, C=C, ld_x=C, ld_last=C, ld_y=C)) == -1
    assert b"null buffer" in L.npvp_last_error()
