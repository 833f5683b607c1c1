"""CPU: which launches of a node leave out the samples its per-sample DropPath drops is decided by one pure function of
npvp_amd.ops - skip_roles - and carried by one object - SampleSkip.  The function is checked against the table of DESIGN.md
("DropPath skip"), written out by hand here; the object's two derived forms - row groups for the GEMM
entry points, (p, salt, frames per sample) for the frame kernels - on three sites, one of which does not cover its rows.  No device."""
import pytest

ALL = dict(frames=True, forward=True, dgrad=True, wgrad=True, fused=True)
NONE = dict(frames=False, forward=False, dgrad=False, wgrad=False, fused=False)
# node, DROP_PATH_SKIP, WGRAD_ROW_SKIP -> frame kernels, forward GEMMs, unfused dgrad, unfused weight gradient, fused dgrad + wgrad launch
TABLE = [
    ("mlpdwbn", False, False, NONE),
    ("mlpdwbn", False, True, NONE),
    ("mlpdwbn", True, True, ALL),
    ("mlpdwbn", True, False, dict(ALL, wgrad=False)),          # (the fused launch keeps the spec for both halves)
    ("self_attn", False, True, dict(NONE, wgrad=True, fused=True)),
    ("self_attn", True, True, dict(NONE, wgrad=True, fused=True)),
    ("self_attn", False, False, NONE),
    ("self_attn", True, False, NONE),
]
# p, salt, T frames per sample, frames -> covers its rows
SITES = [(0.25, 7, 4, 32, True), (0.5, 9, 3, 6, True), (0.1, 1, 2, 7, False)]
HALVES = ("forward", "dgrad", "wgrad", "fused")


@pytest.fixture(scope="module")
def ops():
    from npvp_amd import build
    build.build(verbose=False)
    from npvp_amd import ops
    return ops


def _site(ops, p, salt):
    d = ops.Drop.__new__(ops.Drop)
    d.p, d.mode, d.g1, d.g2, d.salt = p, 1, 1, 1, salt
    return d


@pytest.mark.parametrize("node,dp_skip,wg_skip,want", TABLE, ids=[f"{t[0]}-{int(t[1])}{int(t[2])}" for t in TABLE])
def test_role_table(ops, node, dp_skip, wg_skip, want):
    assert ops.skip_roles(node, dp_skip, wg_skip)._asdict() == want


def test_switch_defaults(ops):
    assert ops.DROP_PATH_SKIP is True and ops.WGRAD_ROW_SKIP is True


def _rows(d):
    return (d.p, d.g1, d.g2, d.salt)


@pytest.mark.parametrize("p,salt,T,frames,covers", SITES)
def test_derived_forms(ops, p, salt, T, frames, covers):
    skip = ops.SampleSkip.of(ops.skip_roles("mlpdwbn", True, True), _site(ops, p, salt), T * 64, frames // T, frames * 64)
    assert skip.frame == (p, salt, T)
    for half in HALVES:
        rows = getattr(skip, half)
        if covers:
            assert _rows(rows) == (p, T * 64, frames // T, salt), half          # (= Drop._like(site, 1, rows per sample, samples))
        else:
            assert rows is ops.NO_DROP and rows.p == 0.0, half


def test_roles_gate_the_forms(ops):
    p, salt, T, frames, _ = SITES[0]
    site, args = _site(ops, p, salt), (T * 64, frames // T, frames * 64)
    no_wgrad = ops.SampleSkip.of(ops.skip_roles("mlpdwbn", True, False), site, *args)
    assert no_wgrad.frame == (p, salt, T) and no_wgrad.wgrad is ops.NO_DROP
    assert all(_rows(getattr(no_wgrad, h)) == (p, T * 64, frames // T, salt) for h in ("forward", "dgrad", "fused"))
    attn = ops.SampleSkip.of(ops.skip_roles("self_attn", False, True), site, *args)
    assert attn.frame == (0.0, 0, 1) and attn.dgrad is ops.NO_DROP and attn.forward is ops.NO_DROP
    assert all(_rows(getattr(attn, h)) == (p, T * 64, frames // T, salt) for h in ("wgrad", "fused"))
    # nothing to take: the switches off, a site that is off, a site that is no per-sample (row-group) one
    elem = _site(ops, p, salt)
    elem.mode = 0
    for roles, s in ((ops.skip_roles("mlpdwbn", False, True), site), (ops.skip_roles("self_attn", True, False), site),
                     (ops.skip_roles("mlpdwbn", True, True), ops.NO_DROP), (ops.skip_roles("mlpdwbn", True, True), elem)):
        assert ops.SampleSkip.of(roles, s, *args) == ops.NO_SKIP
    off = ops.NO_SKIP
    assert all(_rows(getattr(off, h)) == (0.0, 1, 1, 0) for h in HALVES) and off.frame == (0.0, 0, 1)     # what the plain C entry points pass on
    with pytest.raises(AttributeError):
        off.fused = site
