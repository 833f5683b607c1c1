// The (attn dim, value dim) pairs the autoencoder's attention kernels are instantiated for - the non-local 2-D ones (ae_train.hip) and
// the temporal ones (ae_temporal.hip) alike: C = 64, 128, 256, 512 of the AE configs, A = C / 8, V = 4 A.  ops._NL_GRID is the Python
// side of this table (tests/test_ae_attn_ops_host.py holds the two against each other).  No dependencies: plain C++.
#pragma once

// X(A, V, extra...) once per pair, in dispatch order; whatever follows X in the call is handed to every X as its extra arguments
#define NPVP_AE_ATTN_DIMS(X, ...) X(8, 32, __VA_ARGS__) X(16, 64, __VA_ARGS__) X(32, 128, __VA_ARGS__) X(64, 256, __VA_ARGS__)

static inline bool npvp_ae_attn_dims(int A, int V) {
#define NPVP_AE_ATTN_IS(a, v, ...) || (A == a && V == v)
  return false NPVP_AE_ATTN_DIMS(NPVP_AE_ATTN_IS, );
#undef NPVP_AE_ATTN_IS
}
