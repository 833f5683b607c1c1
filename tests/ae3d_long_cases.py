"""Shared cases of the long-clip (T > 32) temporal attention tests (tests/test_ae3d_long_host.py, tests/test_hip_ae3d_long.py) and of
their fixture generator (tests/golden/make_ae3d_long_golden.py).  Inputs, restatements and error measures are those of
tests/ae3d_cases.py; this file adds the shapes."""
import ae3d_cases as AC

MAX_T = 32                           # ops.TEMPORAL_ATTN_MAX_T: up to here the one-tile kernels, above the key-tiled ones
BLOCK_SEED, PAIR_SEED = 310, 410     # the seeds of tests/test_ae3d_host.py
# Factorized3DConvAttn(64, learn_3d=True) on one clip of 50 frames (KTH's 10 past + 40 future) of a 2 x 2 grid.  ((1, 40, 2, 4) is not
# taken: there the reference's own fp32 gradient of attn1d.gamma is 1.15e-5 from float64, over the 1e-5 bar before any kernel runs.)
LONG_BLOCK = (1, 50, 2, 2)           # (N, T, H, W)
# kernel cases (A, V, T) at N = 2, HW = 5
# (the kernels cut a clip into the fewest equal tiles of at most 32 frames, 16 at (64, 256); the last tile may be shorter)
KERNEL_CASES = ([(A, V, 33) for A, V in AC.DIMS]                 # one frame past one tile: 17 + 16 ((64, 256): 11 + 11 + 11)
                + [(8, 32, 64), (64, 256, 64)]                   # exact tiles: 2 x 32, 4 x 16
                + [(16, 64, 65)]                                 # one frame past two tiles: 22 + 22 + 21
                + [(32, 128, 97)]                                # four tiles, one short: 25 + 25 + 25 + 22
                + [(8, 32, 40), (8, 32, 50)])                    # the protocol lengths: KTH's 40 future frames, 10 past + 40 future


def long_block_file(conv_first):
    """fixture of the long block case, tests/golden/<name>.npz: one file per order"""
    return "ae3d_long_block_" + ("conv" if conv_first else "attn")


def long_block_tag(conv_first):
    return AC.block_tag(*LONG_BLOCK, conv_first)


def long_block_input():
    """(x, cotangent) of the long block case, taken as AC.block_input takes them"""
    return AC.block_input(*LONG_BLOCK)
