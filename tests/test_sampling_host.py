"""Host side of the sampler (no GPU): the two entry points are declared in include/npvp_hip.h and reach the ctypes table, the numpy
restatement of the counter hash that tests/test_hip_sampling.py holds the kernel against agrees with csrc/common.h's own rng_u32
(host-compiled from the header), best_of_samples' index selection and tie rule on CPU tensors with a plain Python per-image
metric, and the refusals that must not need the library."""
import os
import subprocess

import numpy as np
import pytest
import torch

import sampling_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prototypes_are_in_the_header_and_the_ctypes_table():
    from npvp_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    for name, nargs in (("npvp_reparam_samples", 10), ("npvp_attn_samples_fwd", 18)):
        assert f"int {name}(" in text
        assert name in _lib.PROTOTYPES and name in _lib.SIGNATURES
        assert _lib.PROTOTYPES[name][0] == "int" and len(_lib.SIGNATURES[name][1]) == nargs
    for cite in ("Predictor.py:320-322", "submodules.py:408-410", "VidHRFormer.py:229-239"):
        assert cite in text, f"the header comment cites ref {cite}"
    # the device seed is a pointer, the salt a 32-bit value, sample_base 64 bits: the convention of the dropout kernels
    assert _lib.PROTOTYPES["npvp_reparam_samples"][1][6:9] == ["long long", "const unsigned long long*", "unsigned int"]


def test_numpy_hash_is_the_headers_hash(tmp_path):
    src = tmp_path / "hash_dump.hip"
    src.write_text(r'''#include "common.h"
#include <cstdio>
#include <cstdlib>
// usage: prog seed salt stride offset count  -> count raw 32-bit hashes of idx = offset + i * stride on stdout
int main(int argc, char** argv) {
  const unsigned long long seed = strtoull(argv[1], nullptr, 0), stride = strtoull(argv[3], nullptr, 0), off = strtoull(argv[4], nullptr, 0);
  const unsigned int salt = (unsigned int)strtoul(argv[2], nullptr, 0);
  const long n = atol(argv[5]);
  unsigned int* buf = (unsigned int*)malloc(n * 4);
  for (long i = 0; i < n; ++i) buf[i] = npvp::rng_u32(seed, salt, off + (unsigned long long)i * stride);
  fwrite(buf, 4, n, stdout);
  return 0;
}
''')
    exe = tmp_path / "hash_dump"
    csrc = os.path.join(ROOT, "npvp_amd", "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O2", "-std=c++17", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n = 4096
    for seed, salt, stride, off in ((0x1234567887654321, 77, 1, 0), (5, 0x53414D50, 2, (1 << 33) + 7), (0x7FFFFFFFFFFFFFFF, 0xFFFFFFFF, 3, (1 << 40) - 100)):
        out = subprocess.run([str(exe), str(seed), str(salt), str(stride), str(off), str(n)], capture_output=True, timeout=120)
        assert out.returncode == 0
        want = np.frombuffer(out.stdout, dtype=np.uint32)
        with np.errstate(over="ignore"):
            got = SC.rng_u32(seed, salt, np.uint64(off) + np.arange(n, dtype=np.uint64) * np.uint64(stride))
        assert np.array_equal(got.astype(np.uint32), want)


def test_gauss_ref_is_a_bounded_standard_normal():
    g = SC.gauss_ref(99, 3, 1 << 16, 2, 5)
    assert g.shape == (2, 1 << 16) and np.isfinite(g).all() and np.abs(g).max() <= np.sqrt(48 * np.log(2))
    n = g.size
    assert abs(g.mean()) <= 5 / np.sqrt(n) and abs(g.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.array_equal(SC.gauss_ref(99, 3, 1 << 16, 1, 6)[0], g[1])          # sample 6 whatever S and sample_base


def _neg_mse(x, y, mean_flag=True):
    """a plain per-image metric with the calling convention of npvp_amd.metrics.PSNR / MSEScore"""
    v = -((x - y) ** 2).flatten(1).mean(1)
    return v.mean().item() if mean_flag else v


def test_best_of_samples_index_selection_and_ties_on_cpu():
    from npvp_amd.metrics import best_of_samples
    g = torch.Generator().manual_seed(3)
    N, S, T = 3, 4, 2
    target = torch.rand((N, T, 1, 4, 4), generator=g)
    pred = target[:, None] + 0.3 * torch.randn((N, S, T, 1, 4, 4), generator=g)
    pred[0, 2], pred[1, 3] = target[0], target[1]               # clip 0: sample 2, clip 1: sample 3
    pred[2, 3] = pred[2, 1] = target[2]                         # clip 2: samples 1 and 3 tie -> the lower index
    idx, best, every = best_of_samples(pred, target, _neg_mse)
    assert idx.tolist() == [2, 3, 1] and best.shape == (N, T) and every.shape == (N, S, T)
    for s in range(S):
        for t in range(T):
            assert torch.equal(every[:, s, t], _neg_mse(pred[:, s, t], target[:, t], mean_flag=False))
    assert torch.equal(best, torch.stack([every[n, i] for n, i in enumerate(idx.tolist())]))
    # lower is better: the same clips through the positive error
    idx2, best2, _ = best_of_samples(pred, target, lambda x, y, mean_flag=True: -_neg_mse(x, y, mean_flag=False), higher_is_better=False)
    assert idx2.tolist() == [2, 3, 1] and torch.equal(best2, -best)
    # the choice is by the MEAN over T: a sample that wins one step but loses on average is not chosen
    pred[0, 0, 0] = target[0, 0]; pred[0, 0, 1] = target[0, 1] + 10.0
    assert best_of_samples(pred, target, _neg_mse)[0].tolist() == [2, 3, 1]
    with pytest.raises(ValueError):
        best_of_samples(pred[:, 0], target, _neg_mse)


def _tiny(stochastic):
    import npvp_amd
    h = torch.linspace(0, 7, 8)
    return npvp_amd.Predictor(8, 8, 5, h, h, torch.linspace(0, 1, 2), torch.linspace(2, 4, 3), 512, 'Add', 'layer', 256, 1, stochastic, 1,
                              evt_former=True, learn_evt_token=False, evt_former_num_layers=1, dropout=0.0, drop_path=0.0)


def test_deterministic_predictor_is_refused_on_the_cpu_without_the_library():
    import npvp_amd
    m = _tiny(False)
    x = torch.zeros(1, 2, 512, 8, 8)
    with pytest.raises(ValueError, match="stochastic"):
        m.sample(x, 2)
    with pytest.raises(ValueError, match="stochastic"):
        npvp_amd.predictor_sample_step(m, x, 2)
    assert m.training                                            # nothing was touched


def test_new_names_are_exported():
    import npvp_amd
    for name in ("predictor_sample_step", "full_sample_step"):
        assert name in npvp_amd.__all__ and callable(getattr(npvp_amd, name))
    assert callable(npvp_amd.metrics.best_of_samples) and callable(npvp_amd.metrics.pred_best_metrics)
    assert callable(npvp_amd.ops.reparam_samples) and callable(npvp_amd.ops.cross_attn_samples)
    assert hasattr(npvp_amd.Predictor, "sample")
