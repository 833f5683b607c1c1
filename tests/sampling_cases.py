"""The counter hash and the Box-Muller lines of csrc/sample.hip's header comment, restated in numpy (float64): what
tests/test_hip_sampling.py holds the kernel's eps against, and what tests/test_sampling_host.py holds against csrc/common.h's own
rng_u32, host-compiled."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def _mix32(h):
    h = h & M32
    h ^= h >> np.uint64(16); h = (h * np.uint64(0x85ebca6b)) & M32
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xc2b2ae35)) & M32
    h ^= h >> np.uint64(16)
    return h


def rng_u32(seed, salt, idx):
    """csrc/common.h rng_u32 on uint64 arrays holding 32-bit values"""
    seed, salt = np.uint64(seed), np.uint64(salt)
    k0 = _mix32((seed & M32) ^ _mix32((salt * np.uint64(0x9e3779b9) + np.uint64(0x7f4a7c15)) & M32))
    k1 = _mix32(((seed >> np.uint64(32)) + _mix32(salt ^ np.uint64(0x85ebca6b))) & M32)
    h = _mix32((idx & M32) ^ k0)
    return _mix32((h + k1 + ((idx >> np.uint64(32)) * np.uint64(0x9e3779b9) & M32)) & M32)


def gauss_ref(seed, salt, numel, S, sample_base):
    """the header comment of csrc/sample.hip in float64: g[s, i]"""
    with np.errstate(over="ignore"):
        ctr = (np.arange(S, dtype=np.uint64)[:, None] + np.uint64(sample_base)) * np.uint64(numel) + np.arange(numel, dtype=np.uint64)[None, :]
        r1 = rng_u32(seed, salt, np.uint64(2) * ctr)
        r2 = rng_u32(seed, salt, np.uint64(2) * ctr + np.uint64(1))
    u1 = ((r1 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (r2 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
