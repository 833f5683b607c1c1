/* libnpvp_hip.so - C ABI of the MI355X (gfx950) kernels behind NPVP's Stage-2 predictor
 * hot path.  The reference has NO native boundary for this path: it is pure Python that
 * reaches ATen through torch.nn modules ("zero CUDA kernels, zero C++").  The
 * entry points below are what a reference-side binding replaces those torch calls with;
 * each one names the reference call sites whose arithmetic it takes over.  INTEGRATION.md
 * shows the ctypes stub a maintainer adds to ref/models/VidHRFormer.py.
 *
 * Conventions (all entry points)
 *   - plain pointers + sizes, fp32, row-major, no torch types; every pointer is DEVICE memory
 *     owned and allocated by the caller (including workspaces and saved-for-backward tensors);
 *   - the library never allocates, frees, synchronises or keeps global mutable state (but a launch counter and the
 *     thread-local error string); all work
 *     is enqueued on `stream` (a hipStream_t), so calls are graph-capturable and re-entrant;
 *   - return 0 on success, <0 on error (-1 bad argument, -2 launch failure, -3 workspace);
 *     npvp_last_error() gives the thread-local message; nothing throws;
 *   - canonical activation layout: x[F][P][C], F = N*T frames (f = n*T + t), P = H*W, C contiguous;
 *   - dropout / drop-path masks are a counter hash of (*seed, salt, element key): `seed` is a
 *     device uint64 (so a captured graph sees a new value per replay), `salt` identifies the call
 *     site; backward entry points replay the forward mask from the same (seed, salt).
 *
 * Where this header differs from SURVEY 8(b)'s sketch it is authoritative:
 *   - the data-parallel exchange (`npvp_dp_*`, at the end of this header) is the one part of the library WITH process state (one
 *     RCCL communicator per process); RCCL is looked up at the first npvp_dp_* call, not linked.  npvp_amd/dp.py drives either
 *     these entry points (NPVP_DP_COMM=c) or torch.distributed's ProcessGroupNCCL (default - the same RCCL; a PyTorch host
 *     already owns a communicator set, SyncBatchNorm's statistics travel on it either way).
 *   - `npvp_<op>_workspace_bytes` exists for the entry points that NEED a workspace (GEMM split-K, LayerNorm / frame-LN /
 *     fused-middle parameter-gradient partials, colsum, metrics); the others take none.
 */
#ifndef NPVP_HIP_H
#define NPVP_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* npvp_stream_t; /* == hipStream_t */

int npvp_version(void);
const char* npvp_last_error(void);
/* Diagnostics: kernels this library has launched in this process so far (one relaxed atomic add per launch).  bench.py reads it
 * around a step so that its record says how many launches a step is. */
long long npvp_launch_count(void);
/* A stream of the lowest priority the device offers, for work nothing on the critical path waits for (the in-place
 * weight-gradient writes); least / greatest receive the device's priority range (nullable). */
void* npvp_stream_create_low_priority(int* least, int* greatest);
int npvp_stream_destroy(void* stream);
/* Timing events that survive a HIP-graph capture (the benchmark's live per-kernel probe; the reference has no counterpart - its
 * timings are time.time() around a forward, ref/Inference.ipynb:463-467).  npvp_event_record on a CAPTURING stream becomes an
 * external event-record node (hipEventRecordWithFlags / hipEventRecordExternal): every replay stamps the event, and after a
 * synchronisation npvp_event_elapsed_ms(e0, e1) is the time between the two stamps of the LAST replay; on an ordinary stream it is a
 * plain hipEventRecord.  elapsed < 0: an event was never recorded or has not completed. */
void* npvp_event_create(void);
int npvp_event_record(void* event, void* stream);
float npvp_event_elapsed_ms(void* event0, void* event1);
int npvp_event_destroy(void* event);

/* Node census of a captured step (a hipGraph_t, e.g. torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()): counts[16] indexed by
 * hipGraphNodeType (0 kernel, 1 memcpy, 2 memset, ...), memset_bytes[0 .. max_memsets) the sizes of the first memset nodes; returns
 * the number of nodes or a negative error.  The training step of this library contains no memset node, and the host layer checks
 * it: on ROCm 7.2 a graph replayed from prepared packets (the runtime's default) does not execute its memset nodes reliably - stale fill
 * patterns once the process has issued other memsets (tools/graph_memset_node_repro.py, profiles/r06_graph_alloc_hazard.txt). */
long long npvp_graph_node_counts(void* graph, long long* counts, long long* memset_bytes, int max_memsets);

/* ---- GEMM (every nn.Linear / 1x1 Conv2d / MHA in- and out-projection and their backward:
 * ref/models/VidHRFormer.py:71-72,111,184-185,225 (token FFN), :345,364,380,387 (MlpDWBN fc1/fc2),
 * torch.nn.MultiheadAttention in_proj/out_proj at :70,180,192,270; NRMLP linears
 * ref/models/submodules.py:275,288,295).
 *   C[M,N] = epilogue(alpha * op(A)[M,K] op(B)[K,N])
 *   a_kc=1: A is [M][K]; a_kc=0: A is [K][M].   b_kc=1: B is [N][K]; b_kc=0: B is [K][N].
 *   epilogue order: +bias[N] -> aux_out (pre-activation copy) -> act -> dropout -> +residual
 *   act: 0 none, 1 GELU(erf), 2 ReLU, 3 multiply by GELU'(aux_in), 4 multiply by [aux_in > 0]
 *   drop_mode 0: per element; 1: per row group key=(row/drop_g1)%drop_g2 (DropPath)
 * K % 32 == 0, M % 4 == 0, N % 4 == 0, lda/ldb % 4 == 0, A/B 16-byte aligned.
 * precision 0: exact fp32-input MFMA (v_mfma_f32_32x32x2_f32; parity triage).  precision 4: every fp32 operand is
 * split into three bf16 terms and the six leading cross products are accumulated in fp32 on v_mfma_f32_32x32x16_bf16
 * (relative product error ~2^-23: fp32-grade).  precision 5: two terms, three products (~2^-16; opt-in for weight gradients).
 * precision 6 (the path's default): TWO fp16 terms per operand, three products on v_mfma_f32_32x32x16_f16 (~2^-22 per
 * product: fp32-grade at half the matrix instructions of precision 4).  fp16 has no exponent range to spare, so each operand
 * comes with an AMAX SLOT (2 KB of device memory holding 32 words whose maximum bounds |operand|; see npvp_amax) and is scaled by the power
 * of two that puts the bound into [2^14, 2^15) - exact, undone in the epilogue.  It is taken by (a) a_kc = 1 launches with
 * fp16 planes in `b_pre` (npvp_split_weight_f16) and both a_amax / b_amax, (b) weight gradients (a_kc = b_kc = 0, plain
 * epilogue, K >= 1024) with both slots; every other launch with precision 6 runs as precision 4 without planes.
 * precision 7 ("f16x1", inference): precision 6 in every respect - planes, slots, routes, fallbacks, weight gradients - except that
 * the launches of (a), kernel ids 5 / 7, multiply the HIGH fp16 terms only: C = epilogue(alpha hi(A sa) hi(B sb) / (sa sb)), hi(x s) =
 * rne_f16(x s), ONE matrix instruction per product, 11 significant bits per operand (2.9e-4 rel-L2 of a product sum against the exact
 * one; accumulation stays fp32).  It reads plane 0 of the same fp16 planes (half the weight bytes) in K-steps of 32; tiles, epilogue,
 * c_amax and the per-row rescue of rows far below the tensor's bound are precision 6's.  Forward-only: adrop_p > 0 or skip_p > 0 with
 * precision 7 is an argument error.  npvp_amd.ops.eval_arithmetic("f16x1") is what passes it, for launches autograd does not record.
 * c_amax (nullable, any precision, unsplit launches): the kernel adds the bound of the values it stores to C to that slot -
 * the next GEMM's a_amax, at no extra pass.
 * Kernels: gemm_wide_kernel (128 x 256 tiles, 4 waves, A split on the fly, B = pre-split planes `b_pre` copied by LDS-DMA:
 * the large forward / dgrad shapes), gemm_wgrad_wide_kernel (weight gradients over >= 32 K token rows: row-major staging,
 * transposing LDS reads, split-K), gemm_split_db_kernel (128 x 128 tiles: everything else).
 * colsum_a (a_kc = 0 only, nullable): receives colsum_a[m] = sum_k A[k][m] - the bias gradient falls out of the
 * weight-gradient GEMM's own operand staging (dW = dy^T x, db = column sums of dy), no extra pass over dy.
 * accumulate = 1: C += result and colsum_a += sums - a weight / bias gradient is accumulated straight into the live
 * .grad slice of the flat gradient buffer (no temporary, no separate add kernel); the same flag exists on the other
 * entry points that produce parameter gradients (npvp_layernorm_bwd, npvp_frameln_act_bwd, npvp_colsum).
 * When the tile count is small and K large (weight gradients) the reduction is split over
 * workgroups through `workspace` (npvp_gemm_workspace_bytes; 0 = never split). */
long long npvp_gemm_workspace_bytes(int M, int N, int K);
/* which kernel npvp_gemm_f32 picks for a shape: 0 gemm_f32_kernel, 1 gemm_split_db_kernel (128 x 128 tiles), 2
 * gemm_wide_kernel<2,4,2,2> (128 x 256 tiles, weight planes by LDS-DMA), 3 gemm_wgrad_wide_kernel, 4 gemm_wide_kernel<2,2,2,2>
 * (the same kernel on 128 x 128 tiles: outputs too small to fill the chip with wide tiles), 5 gemm_f16_kernel<2,4,2,2> (precision 6,
 * 128 x 256 tiles; precision 7: its one-term instantiation), 6 gemm_wgrad_f16_kernel, 7 gemm_f16_kernel on smaller tiles.  The first word of npvp_gemm_route with a plain
 * epilogue.  Pure function (measurement aid; ops.gemm also decides from it which amax slots to fill). */
int npvp_gemm_kernel_id(int a_kc, int b_kc, int M, int N, int K, int precision, int has_planes);
/* The whole route of a launch, for tests that must prove which leaf of the dispatcher they hit (tests/gemm_route_cases.py).  It is the
 * dispatcher's own plan: npvp_gemm_f32 launches what the same planner returns for the facts of its arguments, this query reports what it
 * returns for a caller that hands over a workspace of npvp_gemm_workspace_bytes and (precision 6 / 7) both amax slots, and asks for no frame
 * statistics.  A caller that leaves the workspace or a slot out gets the same answer with that kernel's condition failing: precision 6
 * without slots runs as precision 4 without planes, a split plan without its workspace runs unsplit on the 128 x 128 kernel.
 * out4 = {kernel id as above, tile variant (precision 6, ids 5 / 7: 1 = 128 x 256, 2 = 128 x 128, 3 = 128 x 64, 4 = 64 x 128 tiles;
 * precision 4, ids 2 / 4: 1 = 128 x 256, 2 = 128 x 128; 0 elsewhere), split-K count of the launch, K-steps per split of that kernel (steps
 * of 16, of 32 for id 0)}.  plain_epilogue = no bias / activation / aux_out / residual / dropout (only such launches split K or take a
 * weight-gradient kernel).  With plain_epilogue = 1, out4[0] == npvp_gemm_kernel_id.  Precision 7 answers as precision 6 (the same for
 * npvp_gemm_kernel_id), except that on ids 5 / 7 the steps are the one-term kernel's own, of 32: out4[3] = K / 32.  Pure function. */
int npvp_gemm_route(int a_kc, int b_kc, int M, int N, int K, int precision, int has_planes, int plain_epilogue, int* out4);
int npvp_gemm_f32(int a_kc, int b_kc, int M, int N, int K, const float* A, long long lda, const float* B, long long ldb,
                  float* C, long long ldc, const float* bias, int act, const float* aux_in, float* aux_out,
                  const float* residual, long long ldr, float drop_p, int drop_mode, int drop_g1, int drop_g2,
                  const unsigned long long* seed, unsigned int salt, float alpha, int precision, float* colsum_a,
                  const void* b_pre, int accumulate, float* rowstats, const float* a_amax, const float* b_amax,
                  float* c_amax, unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                  void* workspace, long long ws_bytes, npvp_stream_t stream);
/* npvp_gemm_f32 with a ROW-SKIP spec (a_kc = 1; a weight gradient, a_kc = b_kc = 0, on the precision-6 kernel id 6 takes the spec
 * over its K rows as npvp_wgrad_f16_chained_skip does and under its conditions): (skip_p, skip_g1, skip_g2, skip_salt) name, like adrop, the row groups
 * (row / g1) % g2 that a DropPath site drops - rows whose result the caller multiplies by an exact 0 (forward) or whose rows of A
 * are exact zeros (dgrad).  On the precision-6 forward / dgrad kernels (ids 5 / 7) a tile all of whose rows lie in dropped groups
 * is not computed - no operand loads, no K loop, no row-guard pass - and runs its usual epilogue on zero accumulators, so C, the
 * rowstats partials and c_amax are written as always and a dropped row of a forward launch holds the bias.  Tiles that touch a kept
 * group, and every other kernel, compute as npvp_gemm_f32 does.  The decision is taken on the device from `seed`; skip_p = 0 is
 * npvp_gemm_f32. */
int npvp_gemm_f32_skip(int a_kc, int b_kc, int M, int N, int K, const float* A, long long lda, const float* B, long long ldb,
                       float* C, long long ldc, const float* bias, int act, const float* aux_in, float* aux_out,
                       const float* residual, long long ldr, float drop_p, int drop_mode, int drop_g1, int drop_g2,
                       const unsigned long long* seed, unsigned int salt, float alpha, int precision, float* colsum_a,
                       const void* b_pre, int accumulate, float* rowstats, const float* a_amax, const float* b_amax,
                       float* c_amax, unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                       float skip_p, int skip_g1, int skip_g2, unsigned int skip_salt, void* workspace, long long ws_bytes,
                       npvp_stream_t stream);
/* Range of the precision-6 (two-term fp16) arithmetic, per ROW.  Operands are scaled by ONE power of two per tensor (their amax
 * slot), so a row that lies 2^18 or more below its tensor's bound would keep only subnormal low terms.  Forward / dgrad launches
 * (kernel ids 5 / 7) repair this themselves: every thread keeps the running |max| of the rows of A it stages, and a tile in which
 * some row lies that far below the bound is computed a second time with every row scaled by the power of two of its OWN maximum
 * (exact; results bit-identical to the one-pass form when no row qualifies; cost: that tile twice).  A weight-gradient launch
 * (kernel id 6; the rows of dW are the COLUMNS of its operand A = dy) only detects the condition per workgroup K-chunk and, if
 * `range_flag` (nullable, a device counter the caller zeroed) is given, adds to it; the caller then re-runs that weight gradient
 * with precision 4, whose bf16 terms have fp32's exponent range (npvp_amd.ops.linear_wgrad: at once in strict mode, from the next
 * step on otherwise).  tests/test_hip_ops.py::test_heavy_tailed_rows_keep_their_precision. */
/* adrop_p > 0 (precision 6, launches that npvp_gemm_kernel_id maps to the fp16 kernels 5 / 6 / 7 only; anything else is an
 * argument error): a ROW-GROUP mask on the rows of operand A - row r is multiplied by the DropPath decision of group
 * (r / adrop_g1) % adrop_g2 (0 or 1 / (1 - p); same (seed, salt) stream as the forward site).  This is the backward of a DropPath
 * site (ref/models/VidHRFormer.py:513-525) without a masked copy of dy: for a dgrad (A = dy [M][K]) the mask is folded into
 * the scale of the rows a thread stages, for a weight gradient (A = dy [K][M], adrop_g1 % 16 == 0) into the scale of the K-step,
 * and the bias gradient colsum_a sums the masked rows. */
/* rowstats (nullable; default precision, a_kc = b_kc = 1, bias-only epilogue, M % 64 == 0, N % 128 == 0): receives
 * [M/64][N/64][2] partial (mean, M2) statistics of the output per frame of 64 rows and block of 64 columns;
 * npvp_frame_stats_finalize turns them into the frame LayerNorm's (mean, rstd): no statistics pass over C. */
int npvp_frame_stats_finalize(const float* part, int parts_per_frame, float values_per_part, float* mean, float* rstd,
                              int frames, float eps, npvp_stream_t stream);
/* Weights change once per optimiser step but are staged by every tile of three GEMMs: split them ONCE into the bf16
 * term planes the split-precision kernel consumes (3 terms x N*K bf16 each, blocked like the LDS image).
 * F feeds y = x w^T (pass as b_pre with b_kc = 1), D feeds dx = dy w (b_pre with b_kc = 0).  b_pre is optional
 * (NULL = split B on the fly, 128 x 128 kernel) and only honoured by precision 4 with a_kc = 1. */
int npvp_split_weight(const float* w, long long ld, int N, int K, void* F, void* D, npvp_stream_t stream);
/* The same for MANY weight views in one launch (after the optimiser step, ref/models/Predictor.py:136 opt.step()): desc is a
 * DEVICE array of `count` records of six 64-bit words {w, ld, N, K, F, D} (pointers as integers). */
int npvp_split_weights_batched(const void* desc, int count, npvp_stream_t stream);
/* ---- amax slots (precision 6).  A slot is 2 KB of device memory, zero before its tensor is produced: 32 words, 64 bytes
 * apart (word i at float offset 16 i; the rest is padding that keeps every word in its own memory sector).  Producers raise
 * single words with integer atomic max (the bit pattern of a non-negative float orders like the float: order independent, so
 * deterministic) and the tensor's bound is the maximum of the 32 words.  npvp_amax is the stand-alone producer for a
 * [rows][cols] matrix (row stride ld) that no kernel of this library wrote: slot = max(slot, |x|). */
int npvp_amax(const float* x, long long rows, long long cols, long long ld, float* slot, npvp_stream_t stream);

/* ---- weight gradients whose split-K reduction rides in the NEXT weight-gradient launch.  dW = dy^T x over 10^3..10^5 token rows
 * has only a handful of output tiles, so the precision-6 kernel (id 6) splits the reduction over ~512 workgroups and leaves
 * `splits` partial slabs to sum.  npvp_gemm_f32 sums them with a launch of its own (170 launches per training step of an 8-clip
 * shard, each an idle tail behind an MFMA-bound kernel).  The chained form defers that sum: it fills `my_job` and returns; the job
 * is handed as `prev_job` to the next chained launch ON THE SAME STREAM, where extra workgroups of that launch do it (HBM-bound work
 * beside MFMA-bound work, no launch, same summation order as the stand-alone reduction: bit-identical), or to
 * npvp_splitk_reduce_job when no launch follows (the end of a backward pass).  The caller keeps `workspace` alive until the job
 * has been handed on.  dw / db: accumulated into when `accumulate` (GradSink), else overwritten - by the job, not by this launch.
 * range_flag, adrop_*: as in npvp_gemm_f32. */
typedef struct npvp_reduce_job {
  const float* ws; float* out; long long ldc; int M, N, splits, accum; float alpha; int blocks; const float* cs_part; float* cs_out;
} npvp_reduce_job_t;                                                                 /* 64 bytes, plain data */
int npvp_wgrad_f16_chainable(int M, int N, int K);                                    /* dW [M][N] over K rows: 1 if the kernel takes it with splits > 1 */
long long npvp_wgrad_f16_chain_workspace_bytes(int M, int N, int K);
int npvp_wgrad_f16_chained(int M, int N, int K, const float* dy, long long lda, const float* x, long long ldb, float* dw,
                           long long ldc, float* db, int accumulate, const float* a_amax, const float* b_amax,
                           unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                           const unsigned long long* seed, const void* prev_job, void* my_job, void* workspace,
                           long long ws_bytes, npvp_stream_t stream);
/* the same with a ROW SKIP: skip_* is the row-group spec of a DropPath site (probability, rows per group, groups, salt; the decision
 * for group g is the site's own, taken on the device from `seed`).  Contract: the rows of dy in dropped groups ARE ZERO; the launch
 * then leaves their K-steps out - x is not read there (it may hold anything) - and deals the kept K-steps evenly over the splits, so
 * dw / db are what the launch without the skip gives up to the order of the split-K sum.  Taken when K == skip_g1 * skip_g2 (each
 * group once), skip_g1 % 16 == 0, skip_g1 >= 256 and skip_g2 <= 64; any other spec runs every K-step, exactly as skip_p = 0 does. */
int npvp_wgrad_f16_chained_skip(int M, int N, int K, const float* dy, long long lda, const float* x, long long ldb, float* dw,
                                long long ldc, float* db, int accumulate, const float* a_amax, const float* b_amax,
                                unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                                float skip_p, int skip_g1, int skip_g2, unsigned int skip_salt,
                                const unsigned long long* seed, const void* prev_job, void* my_job, void* workspace,
                                long long ws_bytes, npvp_stream_t stream);
int npvp_splitk_reduce_job(const void* job, npvp_stream_t stream);
/* n job records (64 bytes each, back to back in HOST memory at `jobs`) in ceil(n / 32) launches; two records of one launch must not
 * name the same `out`. */
int npvp_splitk_reduce_multi(const void* jobs, int n, npvp_stream_t stream);
/* The backward of ONE linear layer y = x w^T (+ b) as ONE launch (precision 6): dx[R,K] = epilogue((adrop mask) dy[R,N] w[N,K]) and
 * dw[N,K] += dy^T x, db[N] += column sums of dy.  Both GEMMs read dy and nothing of each other; on the 8-clip shards of the
 * data-parallel configurations each of them alone leaves half the chip idle (256 workgroups), together they fill it - and a step
 * captured single-stream into a HIP graph (no gradient stream to overlap them) keeps the overlap inside the launch.  Arguments:
 * the dgrad half as npvp_gemm_f32(a_kc = 1, b_kc = 0, M = R, N = K, K = N) takes them - w_planes_d / w_amax = the weight's D planes
 * and slot (npvp_split_weight_f16), act 0 / 3 / 4 with aux_in [R][ldx], the dropout REPLAY of a forward site, residual, dx_amax
 * (nullable) - and the weight-gradient half as npvp_wgrad_f16_chained takes them (always accumulating; its split-K reduction is
 * handed on in my_job, the previous launch's comes in prev_job; npvp_splitk_reduce_job runs the last one).
 * npvp_linear_bwd_f16_takes(R, N, K): 1 when the pair is taken - a small-tile dgrad (fewer than 512 tiles of 128 x 256) and a
 * chainable weight gradient (R >= 1024); everything else stays two launches. */
int npvp_linear_bwd_f16_takes(int R, int N, int K);
int npvp_linear_bwd_f16(int R, int N, int K, const float* dy, long long ldy, const float* dy_amax, const void* w_planes_d,
                        const float* w_amax, float* dx, long long ldx, int act, const float* aux_in, const float* residual,
                        long long ldr, float drop_p, int drop_mode, int drop_g1, int drop_g2, unsigned int drop_salt, float* dx_amax,
                        const float* x, long long ldxx, const float* x_amax, float* dw, long long ldw, float* db,
                        unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                        const unsigned long long* seed, const void* prev_job, void* my_job, void* workspace, long long ws_bytes,
                        npvp_stream_t stream);
/* the same with the row-skip spec of npvp_gemm_f32_skip on the dgrad's tiles and, where npvp_wgrad_f16_chained_skip takes the spec
 * (K there = R here), on the weight gradient's K-steps: the rows of dy in dropped groups are zero, x is not read there */
int npvp_linear_bwd_f16_skip(int R, int N, int K, const float* dy, long long ldy, const float* dy_amax, const void* w_planes_d,
                             const float* w_amax, float* dx, long long ldx, int act, const float* aux_in, const float* residual,
                             long long ldr, float drop_p, int drop_mode, int drop_g1, int drop_g2, unsigned int drop_salt,
                             float* dx_amax, const float* x, long long ldxx, const float* x_amax, float* dw, long long ldw, float* db,
                             unsigned int* range_flag, float adrop_p, int adrop_g1, int adrop_g2, unsigned int adrop_salt,
                             float skip_p, int skip_g1, int skip_g2, unsigned int skip_salt, const unsigned long long* seed,
                             const void* prev_job, void* my_job, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* w [N][K] -> the fp16 planes of precision 6: F[2 terms][K/8][N][8 over k], D[2 terms][N/8][K][8 over n] (2*N*K fp16 each,
 * either may be null), scaled by the power of two of w's amax, which is (re)computed into amax_slot (zeroed here first).
 * npvp_split_weights_f16: the same for `count` views in three stream operations; desc is a DEVICE array of records of eight
 * 64-bit words {w, ld, N, K, F, D, amax_slot, 0}; amax_table / amax_bytes (nullable) name the contiguous memory that holds
 * all the records' slots and is zeroed first (otherwise the caller zeroes the slots). */
int npvp_split_weight_f16(const float* w, long long ld, int N, int K, void* F, void* D, float* amax_slot, npvp_stream_t stream);
int npvp_split_weights_f16(const void* desc, int count, void* amax_table, long long amax_bytes, npvp_stream_t stream);
/* Producer-side slots: every entry point below whose output can be the A operand of a GEMM takes a nullable `amax` slot
 * (after its last data argument) and adds the bound of the values it stores to it - no pass over the tensor is spent on it. */

/* ---- token LayerNorm(C) (ref/models/VidHRFormer.py:65-66,69,77,175-176,179,189,194-195; shared final
 * norm :47-48,150-151; relu=1 fuses the decoder's F.relu_ :159).  C in {256,512,768,1024}.
 * mean/rstd [rows] are saved for backward (nullable in fwd). */
int npvp_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd, long long rows,
                       int C, float eps, int relu, float* y_amax, npvp_stream_t stream);
long long npvp_layernorm_bwd_workspace_bytes(long long rows, int C);
int npvp_layernorm_bwd(const float* dy, const float* x, const float* w, const float* b, const float* mean,
                       const float* rstd, float* dx, float* dw, float* db, long long rows, int C, int relu,
                       const float* dres /* nullable: dx += dres, the residual branch's gradient */,
                       int accumulate /* 1: dw, db +=; 2: leave the partial sums in workspace */, float* dx_amax,
                       void* workspace, long long ws_bytes, npvp_stream_t stream);
/* second stage of npvp_layernorm_bwd(accumulate = 2), on a stream of the caller's choice (the gradient stream) */
int npvp_layernorm_bwd_reduce(const void* workspace, float* dw, float* db, long long rows, int C, int accumulate,
                              npvp_stream_t stream);

/* Deferred parameter-gradient reductions.  The second stages above (npvp_layernorm_bwd_reduce, npvp_frameln_act_bwd_reduce,
 * npvp_mlpdw_mid_bwd_reduce_into) each sum a set of partial rows into a gradient slice nobody reads before the optimiser: ~150
 * small launches per backward pass.  The *_reduce_job forms take the same arguments and, instead of launching, write a 48-byte job
 * record to HOST memory at `job`; npvp_sum_rows_multi runs n such records (back to back at `jobs`) with ceil(n / 40) launches, the
 * records travelling in the kernels' argument blocks (nothing to upload or keep alive; graph-capturable).  Each form sums in a
 * fixed order of its own.  One plan (csrc/norm.hip plan_sum_rows) picks the column blocks of both, so a queued job is bit-identical
 * to the single launch wherever the two split the partial rows over the same lanes: the float4 walk (fewer than 64 partial rows
 * over >= 4096 columns: the frame LayerNorm) and every set of 64 or more partial rows (LayerNorm from 253 token rows on).  It is
 * equal to rounding where they do not: fewer than 64 partial rows off the float4 walk (LayerNorm below 253 rows, a frame LayerNorm
 * below 4096 columns: 4 row lanes in the single launch, 16 in the queued one) and npvp_mlpdw_mid_bwd_reduce_into, whose kernel
 * walks the chunks serially per thread.  The workspaces must stay alive until npvp_sum_rows_multi has been enqueued behind their
 * producers (same stream, or a stream ordered after it). */
int npvp_layernorm_bwd_reduce_job(const void* workspace, float* dw, float* db, long long rows, int C, int accumulate, void* job);
int npvp_frameln_act_bwd_reduce_job(const void* workspace, float* dw, float* db, int frames, int per_frame, int accumulate, void* job);
int npvp_mlpdw_mid_bwd_reduce_job(const void* workspace, float* gw, float* gb, int frames, int Ch, void* job);
int npvp_sum_rows_multi(const void* jobs, int n, npvp_stream_t stream);

/* The decoder's final LayerNorm + ReLU writing the reference's (N,T,C,H,W) tensor directly (ref/models/VidHRFormer.py:150-159:
 * norm, relu_, permute(0,1,4,2,3)).  P must be 64, C 256 or 512; mean / rstd per token row as npvp_layernorm_fwd writes them, so
 * the backward is npvp_transpose of dy followed by npvp_layernorm_bwd. */
int npvp_layernorm_nchw_fwd(const float* x, const float* w, const float* b, float* out_nchw, float* mean, float* rstd, int frames,
                            int P, int C, float eps, int relu, npvp_stream_t stream);

/* ---- PosFeatFuser 'layer' (ref/models/submodules.py:432-454: GroupNorm(1,C,affine=False) over one
 * frame's C*H*W elements, then xhat*(1+gamma)+beta).  x [N*T][per_frame], add [N][per_frame] or NULL
 * (the `+ query_evt` of ref/models/VidHRFormer.py:211,236), beta/gamma [T][per_frame] (gamma NULL for
 * fuse_method 'Add').  mean/rstd [N*T] are outputs. */
int npvp_frame_stats(const float* x, const float* add, float* mean, float* rstd, int frames, int T, int per_frame,
                     float eps, npvp_stream_t stream);
int npvp_posfuse_fwd(const float* x, const float* add, const float* beta, const float* gamma, float* y, float* mean,
                     float* rstd, int N, int T, int per_frame, float eps, float* y_amax, npvp_stream_t stream);
/* bwd: du = d(x+add) [N*T][per_frame]; dbeta / dgamma [T][per_frame] (nullable) = the sums over the batch of dy and dy*uhat (the
 * reference's autograd sums them where beta / gamma broadcast over N).  npvp_posfuse_bwd_fused(N, T, per_frame) == 1: they come out
 * of the apply pass itself (the batch loop runs inside the thread; dyxh is not touched and may be NULL); == 0 (few (t, e) columns,
 * many samples): dyxh [N*T][per_frame] is scratch for dy*uhat and two reductions follow.  accumulate = 1: dbeta / dgamma += (a
 * positional table feeds ~30 sub-layers per step: its gradient is summed in place instead of by autograd's add kernels). */
/* The pre-norm LayerNorm of an attention sub-layer and the positional fuse of its output in ONE kernel (frames of P = 64 token rows,
 * C = 512): y1 = LayerNorm(x) [N*T*P][C] with its row statistics ln_mean / ln_rstd [N*T*P], fused = posfuse(y1 (+ add)) with
 * its frame statistics pf_mean / pf_rstd [N*T]; the same results as npvp_layernorm_fwd followed by npvp_posfuse_fwd. */
int npvp_ln_posfuse_fwd(const float* x, const float* lw, const float* lb, float ln_eps, float* y1, float* ln_mean, float* ln_rstd,
                        const float* add, const float* beta, const float* gamma, float* fused, float* pf_mean, float* pf_rstd,
                        int N, int T, int P, int C, float pf_eps, float* y1_amax, float* fused_amax, npvp_stream_t stream);
int npvp_posfuse_bwd_fused(int N, int T, int per_frame);
int npvp_posfuse_bwd(const float* dy, const float* x, const float* add, const float* gamma, const float* mean,
                     const float* rstd, float* du, float* dyxh, float* dbeta, float* dgamma, int N, int T, int per_frame,
                     int accumulate, void* workspace, long long ws_bytes /* >= 8*N*T */, npvp_stream_t stream);

/* param_free_norm_type = 'instance' of the same module (ref/models/submodules.py:427-431: InstanceNorm2d(affine=False), statistics
 * per (frame, channel) over the P = H*W <= 64 pixels): x [N*T][P][C] channels-last, add [N][P][C] or NULL, beta / gamma [T][P][C],
 * mean / rstd [N*T][C].  No shipped configuration uses it; it is here so that the module's whole constructor surface runs. */
int npvp_posfuse_instance_fwd(const float* x, const float* add, const float* beta, const float* gamma, float* y, float* mean,
                              float* rstd, int N, int T, int P, int C, float eps, float* y_amax, npvp_stream_t stream);
int npvp_posfuse_instance_bwd(const float* dy, const float* x, const float* add, const float* gamma, const float* mean,
                              const float* rstd, float* du, float* dyxh, int N, int T, int P, int C, npvp_stream_t stream);

/* ---- MlpDWBN inner stages (ref/models/VidHRFormer.py:374-392) on the channels-last hidden tensor
 * h [frames][per_frame = H*W*Ch]:  out = res + droppath_n( drop( GELU( LayerNorm((Ch,H,W))(h) ) ) )
 * with the per-element affine w,b given channels-last [H*W][Ch]; mean/rstd from npvp_frame_stats. */
int npvp_frameln_act_fwd(const float* h, const float* mean, const float* rstd, const float* w, const float* b,
                         const float* res, float* out, int frames, int per_frame, float drop_p, unsigned int salt,
                         float dp_p, unsigned int dp_salt, int frames_per_sample, const unsigned long long* seed,
                         float* out_amax, npvp_stream_t stream);
long long npvp_frameln_act_bwd_workspace_bytes(int frames, int per_frame);
int npvp_frameln_act_bwd(const float* dout, const float* h, const float* mean, const float* rstd, const float* w,
                         const float* b, float* dh, float* dw, float* db, int frames, int per_frame, float drop_p,
                         unsigned int salt, float dp_p, unsigned int dp_salt, int frames_per_sample,
                         const unsigned long long* seed, int accumulate /* 1: dw, db +=; 2: leave partials */,
                         float* dh_amax, void* workspace, long long ws_bytes, npvp_stream_t stream);
int npvp_frameln_act_bwd_reduce(const void* workspace, float* dw, float* db, int frames, int per_frame, int accumulate,
                                npvp_stream_t stream);
/* depthwise 3x3, zero pad 1 (ref/models/VidHRFormer.py:351-358); wt is tap-major [9][Ch]; flip=1 gives the
 * input gradient.  wgrad writes one contiguous [10][Ch] buffer: 9 taps then the bias gradient. */
int npvp_dwconv3x3(const float* a, const float* wt, const float* bias, float* out, int frames, int H, int W, int Ch,
                   int flip, npvp_stream_t stream);
/* the same forward convolution, also returning the frame-LayerNorm statistics (mean, rstd over H*W*Ch per frame) of its
 * output, so that MlpDWBN's norm2 needs no statistics pass (8x8 grid, Ch % 1024 == 0; workspace >= frames*Ch/1024*8 B) */
int npvp_dwconv3x3_stats(const float* a, const float* wt, const float* bias, float* out, float* mean, float* rstd, int frames,
                         int H, int W, int Ch, float eps, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* ---- fused middle of MlpDWBN (ref/models/VidHRFormer.py:381-385: norm1 -> GELU -> depthwise 3x3 [-> norm2's statistics]),
 * 8x8 grid, Ch % 512 == 0.  Forward: h2 = dwconv3x3(gelu(LayerNorm((Ch,H,W))(h1))) + bias in ONE pass over the hidden tensor
 * (a1 is never materialised) plus mean2 / rstd2 of h2 per frame.  wt [9][Ch] tap-major, bias [Ch], w1n / b1n [H*W][Ch].
 * workspace >= frames * (Ch/512) * 8 bytes. */
int npvp_mlpdw_mid_fwd(const float* h1, const float* mean1, const float* rstd1, const float* w1n, const float* b1n,
                       const float* wt, const float* bias, float* h2, float* mean2, float* rstd2, int frames, int H, int W,
                       int Ch, float eps, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* The forward of MlpDWBN's middle and of its frame LayerNorms WITHOUT statistics launches: the consumer merges the partial
 * (mean_j, M2_j) pairs its producer left (part [frames][J][2], nb values per partial) and writes mean / rstd (outputs, for backward).
 * npvp_mlpdw_mid_fwd_parts: part1 = the rowstats of the fc1 GEMM (J1 = Ch / 64, nb1 = 4096); part2 [frames][Ch / 512][2] (32 768
 * values each) receives h2's partials.  npvp_frameln_act_fwd_parts: npvp_frameln_act_fwd with (part, J, nb, eps) in, mean / rstd
 * out; per_frame % 4096 == 0. */
int npvp_mlpdw_mid_fwd_parts(const float* h1, const float* part1, int J1, float nb1, float* mean1, float* rstd1, const float* w1n,
                             const float* b1n, const float* wt, const float* bias, float* h2, float* part2, int frames, int H,
                             int W, int Ch, float eps, npvp_stream_t stream);
int npvp_frameln_act_fwd_parts(const float* h, const float* part, int J, float nb, float eps, float* mean, float* rstd,
                               const float* w, const float* b, const float* res, float* out, int frames, int per_frame,
                               float drop_p, unsigned int salt, float dp_p, unsigned int dp_salt, int frames_per_sample,
                               const unsigned long long* seed, float* out_amax, npvp_stream_t stream);
/* Backward: da1 = conv^T(dh2); dwt_db [10][Ch] (9 tap rows + bias row; accumulate 1: +=, 2: leave the partials in workspace
 * for npvp_mlpdw_mid_bwd_reduce) with a1 recomputed from h1; psum [frames][Ch/256][2] = partial (sum g, sum g*hhat),
 * g = da1 * gelu'(y1) * w1n: the statistics of norm1's backward (npvp_frameln_act_bwd_apply, nparts = Ch/256). */
long long npvp_mlpdw_mid_bwd_workspace_bytes(int frames, int Ch);
int npvp_mlpdw_mid_bwd(const float* dh2, const float* h1, const float* mean1, const float* rstd1, const float* w1n,
                       const float* b1n, const float* wt, float* da1, float* dwt_db, float* psum, int frames, int H, int W,
                       int Ch, int accumulate, void* workspace, long long ws_bytes, npvp_stream_t stream);
int npvp_mlpdw_mid_bwd_reduce(const void* workspace, float* dwt_db, int frames, int Ch, int accumulate, npvp_stream_t stream);
/* the partials of an accumulate = 2 call straight into the Conv2d parameter gradients (weight [Ch][1][3][3], bias [Ch]), in place:
 * reduction over the chunks, transposition and accumulation in one launch */
int npvp_mlpdw_mid_bwd_reduce_into(const void* workspace, float* gw, float* gb, int frames, int Ch, npvp_stream_t stream);
/* The same with norm2's backward inside (ref VidHRFormer.py:385-387: act2(norm2(.)) + Dropout): da2 = gradient w.r.t.
 * a2 = drop(gelu(norm2(h2))); the kernel evaluates dh2 = rstd2 (g - s1 - hhat2 s2), g = da2 * mask * gelu'(y2) * w2n, element by
 * element while it fills its window, so dh2 is never written or read (two passes over the [R, Ch] tensor less).  psum2
 * [frames][nparts2 <= 256][2] = partial (sum g, sum g*hhat2) from npvp_frameln_act_bwd_pgrad, which also produces norm2's
 * parameter gradients.  drop_p / salt / seed: the forward's elementwise dropout (0 = none). */
int npvp_mlpdw_mid_bwd_n2(const float* da2, const float* h2, const float* mean2, const float* rstd2, const float* w2n,
                          const float* b2n, const float* psum2, int nparts2, float drop_p, unsigned int salt,
                          const unsigned long long* seed, const float* h1, const float* mean1, const float* rstd1,
                          const float* w1n, const float* b1n, const float* wt, float* da1, float* dwt_db, float* psum, int frames,
                          int H, int W, int Ch, int accumulate, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* frame-LN backward WITHOUT the input gradient: psum [frames][per_frame / 1024][2] = partial (sum g, sum g*hhat) for a consumer
 * that evaluates dh itself (npvp_mlpdw_mid_bwd_n2); dw / db, accumulate and workspace exactly as npvp_frameln_act_bwd
 * (npvp_frameln_act_bwd_reduce applies).  per_frame % 1024 == 0. */
int npvp_frameln_act_bwd_pgrad(const float* dout, const float* h, const float* mean, const float* rstd, const float* w,
                               const float* b, float* psum, float* dw, float* db, int frames, int per_frame, float drop_p,
                               unsigned int salt, float dp_p, unsigned int dp_salt, int frames_per_sample,
                               const unsigned long long* seed, int accumulate, void* workspace, long long ws_bytes,
                               npvp_stream_t stream);
/* frame-LN backward with the statistics supplied by the producer of dout (one pass instead of two; no dropout):
 * psum [frames][nparts][2]; workspace as npvp_frameln_act_bwd. */
int npvp_frameln_act_bwd_apply(const float* dout, const float* h, const float* mean, const float* rstd, const float* w,
                               const float* b, const float* psum, int nparts, float* dh, float* dw, float* db, int frames,
                               int per_frame, int accumulate, float* dh_amax, void* workspace, long long ws_bytes,
                               npvp_stream_t stream);
/* ---- three of these launches with the node's DropPath as a FRAME-SKIP spec: (skip_p, skip_salt, skip_fps = frames per sample, seed)
 * are the (dp_p, dp_salt, frames_per_sample, seed) that the node's last npvp_frameln_act_fwd_parts call multiplies its output by.
 * The frames of a sample which that call drops are not worked on: no read of the hidden tensor, no GELU, mask hash or tap
 * arithmetic.  Every output is still written in full - a skipped frame gets what the kernel would produce from a zero input
 * (forward: h2 = 0 with the partial (0, 0); out = res, or 0 without res) or a zero gradient (backward: dh = 0, no contribution to
 * dw / db) - so a consumer that skips nothing stays correct on them.  The decision is taken on the device from the device seed
 * (nothing on the host, no extra launch); skip_p = 0 skips nothing, and the entry points above are exactly that.  In
 * _fwd_parts_skip the call's `seed` serves the skip as well.  (The fused middle's backward and npvp_frameln_act_bwd_pgrad have no
 * such form: profiles/droppath_skip.txt.) */
int npvp_mlpdw_mid_fwd_parts_skip(const float* h1, const float* part1, int J1, float nb1, float* mean1, float* rstd1,
                                  const float* w1n, const float* b1n, const float* wt, const float* bias, float* h2, float* part2,
                                  int frames, int H, int W, int Ch, float eps, float skip_p, unsigned int skip_salt, int skip_fps,
                                  const unsigned long long* seed, npvp_stream_t stream);
int npvp_frameln_act_fwd_parts_skip(const float* h, const float* part, int J, float nb, float eps, float* mean, float* rstd,
                                    const float* w, const float* b, const float* res, float* out, int frames, int per_frame,
                                    float drop_p, unsigned int salt, float dp_p, unsigned int dp_salt, int frames_per_sample,
                                    const unsigned long long* seed, float* out_amax, float skip_p, unsigned int skip_salt,
                                    int skip_fps, npvp_stream_t stream);
int npvp_frameln_act_bwd_apply_skip(const float* dout, const float* h, const float* mean, const float* rstd, const float* w,
                                    const float* b, const float* psum, int nparts, float* dh, float* dw, float* db, int frames,
                                    int per_frame, int accumulate, float* dh_amax, void* workspace, long long ws_bytes,
                                    float skip_p, unsigned int skip_salt, int skip_fps, const unsigned long long* seed,
                                    npvp_stream_t stream);

/* im2col / col2im of the EventEncoder's dense 3x3 conv (ref/models/submodules.py:376), channels-last:
 * col2im=0: in [F][H*W][C] -> out [F*H*W][9*C] (tap-major columns); col2im=1: the adjoint. */
int npvp_im2col3x3(const float* in, float* out, int frames, int H, int W, int C, int col2im, npvp_stream_t stream);
long long npvp_dwconv3x3_wgrad_workspace_bytes(int frames, int Ch);
int npvp_dwconv3x3_wgrad(const float* a, const float* dout, float* dwt_db, int frames, int H, int W, int Ch,
                         void* workspace, long long ws_bytes, npvp_stream_t stream);

/* ---- attention cores (the bmm/softmax/dropout/bmm inside torch.nn.MultiheadAttention as called at
 * ref/models/VidHRFormer.py:104-107 (encoder temporal, masked), :221 (decoder temporal), :239 (enc-dec),
 * :298-300 (spatial window; window gather = ref :447-475 as index math)).
 *   mode 0 spatial: dim0 = N*T frames, groups = frames x windows, L = S = ws*ws
 *   mode 1 temporal: dim0 = N, groups = N x P pixels, L = Tq, S = Tk (rows (n*T + t)*P + p)
 *   mask_mode 1 = encoder quirk ref :100-102.  q NOT pre-scaled; head_dim must be 64.
 *   Sequence lengths: npvp_attn_fwd / npvp_attn_bwd take L, S <= 128 (up to 32: the MFMA kernels every shipped configuration runs
 *   on; 33 .. 128: generic kernels - one workgroup per (group, head), operands in LDS, scalar fp32 arithmetic); the
 *   npvp_attn_long_* pair below takes EVERY L, S >= 1 (streaming MFMA kernels, LDS and registers independent of the length;
 *   npvp_amd.ops uses them above 128), so the only bounds left are that token rows and (group, head, tile) indices fit 32 bits and,
 *   in spatial mode, ws <= 1024 (a window of 2^20 tokens: the window-local row arithmetic) - the reference's
 *   nn.MultiheadAttention has no length limit, ref VidHRFormer.py:94-107. */
int npvp_attn_fwd(const float* q, long long ld_q, const float* k, long long ld_k, const float* v, long long ld_v, float* o,
                  long long ld_o, int mode, int dim0, int P, int W, int ws, int Tq, int Tk, int heads, int head_dim,
                  int mask_mode, float drop_p, const unsigned long long* seed, unsigned int salt, float* o_amax,
                  npvp_stream_t stream);
int npvp_attn_bwd(const float* q, long long ld_q, const float* k, long long ld_k, const float* v, long long ld_v,
                  const float* go, long long ld_o, float* dq, long long ld_dq, float* dk, long long ld_dk, float* dv,
                  long long ld_dv, int mode, int dim0, int P, int W, int ws, int Tq, int Tk, int heads, int head_dim,
                  int mask_mode, float drop_p, const unsigned long long* seed, unsigned int salt, float* dq_amax,
                  float* dk_amax /* may equal dq_amax: one slot for a packed q|k gradient */, float* dv_amax,
                  npvp_stream_t stream);
/* The same function, arguments and conventions (dropout keys, mask, amax slots) for any sequence length: one workgroup per
 * (group, head, tile of 64 query rows) streams K / V through LDS in tiles of 64 keys with an online softmax; backward recomputes
 * the softmax statistics (m, 1 / sum, delta per query row) into `workspace` ([3][groups * heads * L] floats: nothing is saved by
 * forward), then dQ per query tile and dK / dV per key tile.  Deterministic: no floating-point atomics, every output element
 * written once. */
int npvp_attn_long_fwd(const float* q, long long ld_q, const float* k, long long ld_k, const float* v, long long ld_v, float* o,
                       long long ld_o, int mode, int dim0, int P, int W, int ws, int Tq, int Tk, int heads, int head_dim,
                       int mask_mode, float drop_p, const unsigned long long* seed, unsigned int salt, float* o_amax,
                       npvp_stream_t stream);
long long npvp_attn_long_bwd_workspace_bytes(int mode, int dim0, int P, int W, int ws, int Tq, int Tk, int heads);
int npvp_attn_long_bwd(const float* q, long long ld_q, const float* k, long long ld_k, const float* v, long long ld_v,
                       const float* go, long long ld_o, float* dq, long long ld_dq, float* dk, long long ld_dk, float* dv,
                       long long ld_dv, int mode, int dim0, int P, int W, int ws, int Tq, int Tk, int heads, int head_dim,
                       int mask_mode, float drop_p, const unsigned long long* seed, unsigned int salt, float* dq_amax,
                       float* dk_amax /* may equal dq_amax */, float* dv_amax, void* workspace, long long ws_bytes,
                       npvp_stream_t stream);

/* ---- the stochastic predictor as a sampler: S futures per clip, the context encoded once (forward only).
 * The reference draws ONE latent per forward (ref/models/Predictor.py:320-322: zo = evt_prior(...), reparameterize at
 * ref/models/submodules.py:408-410) and its encoder-decoder attention (ref/models/VidHRFormer.py:229-239) sees one query set
 * per clip; S samples there are S whole forwards.  Here the decoder runs on S * N clips, sample-major (clip s * N + n), while
 * the memory and its K / V projections stay at N clips.
 *
 * npvp_reparam_samples: z[s][i] = mu[i] + expf(0.5f * logvar[i]) * g(ctr), ctr = (sample_base + s) * numel + i in 64 bits,
 *   g = sqrtf(-2 logf(u1)) * cosf(2 pi u2), u1 = ((r1 >> 8) + 1) * 2^-24, u2 = (r2 >> 8) * 2^-24, r1 / r2 = the library's
 *   counter hash (the dropout masks' rng_u32) of (seed, salt, 2 ctr) / (seed, salt, 2 ctr + 1).  mu, logvar [numel]; z and the
 *   nullable eps_out [S][numel] (eps_out receives g).  Sample sample_base + s is the same bits for every S and every split of
 *   S into calls.  `seed` points to a 64-bit value in DEVICE memory (as for dropout: a captured graph reads a fresh seed on
 *   replay).  Pointers 16-byte aligned; no amax slot (z is the fuser's `add` operand, which takes none). */
int npvp_reparam_samples(const float* mu, const float* logvar, float* z, float* eps_out, long long numel, int S,
                         long long sample_base, const unsigned long long* seed, unsigned int salt, npvp_stream_t stream);
/* npvp_attn_samples_fwd: the temporal (mode 1) attention core of npvp_attn_fwd, no mask, no dropout, for S query sets per
 *   clip: q / o rows ((s * N + n) * Tq + t) * P + p, k / v rows (n * Tk + t) * P + p, own row strides as in npvp_attn_fwd,
 *   head_dim 64, ONE o_amax slot for the whole output.  Tq, Tk <= 32 (the MFMA form; longer sequences are an argument error:
 *   call npvp_attn_fwd / npvp_attn_long_fwd once per sample slab, the slab being a pointer offset).  One wave loads a (clip,
 *   pixel, head) group's K / V tiles once and serves `sample_chunk` samples with them (0: the library chooses; any value gives
 *   the same bits): sample s of o is bit for bit what npvp_attn_fwd writes for that sample's slab of q on the same k / v. */
int npvp_attn_samples_fwd(const float* q, long long ld_q, const float* k, long long ld_k, const float* v, long long ld_v, float* o,
                          long long ld_o, int S, int N, int P, int Tq, int Tk, int heads, int head_dim, int sample_chunk,
                          float* o_amax, npvp_stream_t stream);

/* ---- layout / reductions / masks */
int npvp_drop_apply(const float* x, float* out, long long rows, int ncols, float p, int mode, int g1, int g2,
                    const unsigned long long* seed, unsigned int salt, float* out_amax, npvp_stream_t stream);
int npvp_transpose(const float* in, float* out, int batch, int R, int C, npvp_stream_t stream); /* [B][R][C]->[B][C][R] */
/* Gradient slots of nn.Conv2d(C, C, 3, groups=C) (ref VidHRFormer.py:351-358: weight [C][1][3][3], bias [C]) from the tap-major
 * table [10][C] (9 weight rows + the bias row) that npvp_mlpdw_mid_bwd / npvp_dwconv3x3_wgrad produce: gw[c][tap] += dwtb[tap][c],
 * gb[c] += dwtb[9][c].  Accumulates in place (the flat gradient buffer of the optimiser). */
int npvp_dwtb_accumulate(const float* dwtb, float* gw, float* gb, int C, npvp_stream_t stream);
/* forward direction: weight [C][1][3][3] + bias [C] (NULL = zeros) -> the tap-major table wtb [10][C] (9 tap rows + the bias row) */
int npvp_dwtb_build(const float* w, const float* b, float* wtb, int C, npvp_stream_t stream);
int npvp_reduce_mid(const float* in, float* out, int A, int B, long long Cc, float scale, int accumulate, npvp_stream_t stream);    /* accumulate = 1: out += */
int npvp_broadcast_mid(const float* in, float* out, int A, int B, long long Cc, float scale, npvp_stream_t stream);
/* Centre padding of a feature grid to the next multiple of the attention window and its adjoint (ref/models/VidHRFormer.py:488-511,
 * PadBlock.pad_if_needed / depad_if_needed), on token rows [frames][H*W][C] with row strides ld_* (floats).  The caller supplies the
 * geometry: Hp >= H, Wp >= W, 0 <= top <= Hp - H, 0 <= left <= Wp - W (the reference: top = (Hp - H) / 2, left = (Wp - W) / 2).
 * C % 4 == 0, strides % 4 == 0, buffers 16-byte aligned, row counts below 2^31.
 *   pad: src [F*H*W, C] -> dst [rows_out >= F*Hp*Wp, C].  Every element of dst is written exactly once: the centre rows are copies, the
 *        border rows and the trailing rows [F*Hp*Wp, rows_out) zeros (a caller rounds rows_out up for a GEMM; no zero-filled buffer is
 *        assumed and nothing is memset).  F = 0 writes rows_out zero rows.
 *   cut: src [>= F*Hp*Wp, C] -> dst [F*H*W, C] = the centre rows, + addend [F*H*W, C] (row stride ld_add) when it is not NULL.
 * Each is the other's adjoint.  dst_amax (nullable): the amax slot of dst.  Plain copies: bit-reproducible. */
int npvp_grid_center_pad(const float* src, long long ld_src, float* dst, long long ld_dst, int F, int H, int W, int Hp, int Wp, int top,
                         int left, int C, long long rows_out, float* dst_amax, npvp_stream_t stream);
int npvp_grid_center_cut(const float* src, long long ld_src, const float* addend, long long ld_add, float* dst, long long ld_dst, int F,
                         int H, int W, int Hp, int Wp, int top, int left, int C, float* dst_amax, npvp_stream_t stream);
/* The learned event token of the encoder, on token rows [N][T][P][C] with row strides ld_* (floats).  C % 4 == 0, strides % 4 == 0 and
 * >= C, buffers 16-byte aligned, N*(T+1)*P below 2^31.  Plain copies: bit-reproducible; every output element is written exactly once.
 *   join (ref/models/VidHRFormer.py:36 the token appended as frame T+1 of every clip, :40-41 the positional tables given a zero frame):
 *        y [N, T+1, P, C]: y[n, t < T] = x[n, t], y[n, T] = token.  token_clip_stride (floats) = 0: ONE [P, C] block for all clips (the
 *        parameter EVT); > 0: one block per clip, clip n at token + n * token_clip_stride; token = NULL: zeros (a table's zero frame
 *        with N = 1).  x = NULL: zeros too (the backward of a split whose first output had no gradient).
 *   split (ref/models/Predictor.py:344  x[:, 0:-1], x[:, -1]): y [N, T+1, P, C] -> x [N, T, P, C] and / or last [N, P, C]; either output
 *        may be NULL (not both), and only the rows of a wanted output are read.
 * Each is the other's adjoint; the gradient of a token shared by the clips is npvp_reduce_mid(A = 1, B = N) of the split's `last`.
 * *_amax (nullable): the amax slot of that output. */
int npvp_evt_token_join(const float* x, long long ld_x, const float* token, long long ld_token, long long token_clip_stride, float* y,
                        long long ld_y, int N, int T, int P, int C, float* y_amax, npvp_stream_t stream);
int npvp_evt_token_split(const float* y, long long ld_y, float* x, long long ld_x, float* last, long long ld_last, int N, int T, int P,
                         int C, float* x_amax, float* last_amax, npvp_stream_t stream);

/* out[n] = sum_r x[r][n]: bias gradients of every Linear / Conv2d on the path */
long long npvp_colsum_workspace_bytes(long long rows, int N);
int npvp_colsum(const float* x, long long rows, int N, long long ld, float* out, int accumulate /* out += */,
                void* workspace, long long ws_bytes, npvp_stream_t stream);

/* ---- scalar losses of shared_step (ref/models/Predictor.py:172-194): L1Loss = lam * mean|a - b| (ref/models/criterion.py:99-121)
 * and the sum under Div_KL (ref/models/criterion.py:341-354).  Two-stage sums in a fixed order: deterministic, and - unlike a
 * multi-block torch reduction - without a semaphore that a memset node of a captured graph has to clear.  out / gout are device
 * scalars; l1_mean_bwd writes da = sgn(a - b) * ((gout * lam) / n).  workspace >= 1024 floats. */
int npvp_l1_mean(const float* a, const float* b, long long n, float lam, float* out, void* workspace, long long ws_bytes,
                 npvp_stream_t stream);
int npvp_l1_mean_bwd(const float* a, const float* b, long long n, const float* gout, float lam, float* da, npvp_stream_t stream);
int npvp_sum_all(const float* x, long long n, float* out, void* workspace, long long ws_bytes, npvp_stream_t stream);

/* ---- optimiser step of training_step_no_gan (ref/models/Predictor.py:135-136,197): clip_grad_norm_
 * over a flat gradient range, then torch.optim.AdamW semantics on flat buffers.  hyper = {lr, step}
 * and clip = {norm, coef} live in device memory.  clip may be NULL (nothing is scaled); with a clip,
 * 0 <= clip_begin <= clip_end <= n.  The flat buffers are 16-byte aligned; the workspace holds 1024 floats. */
int npvp_grad_norm_clip(const float* g, long long n, float max_norm, float* out2, void* workspace, long long ws_bytes,
                        npvp_stream_t stream);
int npvp_adamw_step(float* p, float* g, float* m, float* v, long long n, const float* hyper, float beta1, float beta2,
                    float eps, float weight_decay, const float* clip, long long clip_begin, long long clip_end,
                    int write_back_grad, npvp_stream_t stream);

/* ---- evaluation metrics on device (ref/utils/metrics.py:12-43 PSNR / MSEScore, :46-108 SSIM, called per
 * predicted time-step by pred_ave_metrics :110-140).  Images are [N][C][H][W] fp32 (per_image = C*H*W); out is N floats.
 *   sqdiff: out[n] = scale * sum_i ((x[n][i] - y[n][i]) / data_range)^2   (PSNR: scale = 1/per_image, then -10 log10(. + 1e-8)
 *           on the N results; MSEScore: scale = 1, data_range = 1)
 *   ssim:   out[n] = mean over (C,H,W) of the SSIM map, zero-padded Gaussian window; `taps` is a HOST array of window_size
 *           floats (the normalised 1-D Gaussian; the reference's 2-D window is its outer product, :78-83); window_size in
 *           {3,5,7,11}; N*C < 65536. */
long long npvp_sqdiff_workspace_bytes(int N, long long per_image);
int npvp_sqdiff_per_image(const float* x, const float* y, int N, long long per_image, float data_range, float scale, float* out,
                          void* workspace, long long ws_bytes, npvp_stream_t stream);
long long npvp_ssim_workspace_bytes(int N, int C, int H, int W);
int npvp_ssim_per_image(const float* img1, const float* img2, int N, int C, int H, int W, const float* taps /* host */,
                        int window_size, float* out, void* workspace, long long ws_bytes, npvp_stream_t stream);

/* ---- input frames (ref/utils/dataset.py:835-858 VidToTensor + VidNormalize): uint8 HWC frames as decoded ->
 * normalised fp32 (frames, C, H, W): dst = (src / 255 - mean[c]) / std[c].  mean / std are HOST arrays of C floats; C in {1,3,4};
 * frames < 65536. */
int npvp_u8hwc_to_f32chw(const void* src_u8, float* dst, long long frames, int H, int W, int C, const float* mean,
                         const float* std, npvp_stream_t stream);

/* ---- frozen Stage-1 autoencoder epilogues (SURVEY 8f #1 stage 2; ref/models/ResNetAutoEncoder.py:51-261, submodules.py:9-95):
 * with BatchNorm folded into the frozen convolution weights, conv -> BN -> ReLU (-> + skip) is MIOpen's convolution plus ONE pass
 *   out = act(x + bias[c]) + residual      act: 0 none, 1 ReLU, 2 tanh, 3 sigmoid; residual nullable
 *   layout 0: x [outer][inner = C], channel = column (channels_last memory); layout 1: x [outer = N*C][inner = H*W] (NCHW).
 * act_bwd: dx = g * act'(.) from the forward output y (no residual), the decoder's input-gradient path. */
int npvp_bias_act(const float* x, const float* bias, const float* residual, float* out, long long outer, long long inner, int C,
                  int layout, int act, npvp_stream_t stream);
int npvp_act_bwd(const float* g, const float* y, float* dx, long long n, int act, npvp_stream_t stream);
/* The tail of NonLocalAttenion2D.forward (ref/models/submodules.py:150-176: bias of out_proj, folded BatchNorm, activation, gamma *,
 * + x) as ONE pass over out_proj's product, 12 B per element with a residual:
 *   out = fmaf(s, act(x + bias[c]), residual)      residual NULL: out = s * act(x + bias[c])
 * s = *scale, ONE float in DEVICE memory read by the kernel (no host synchronisation: the call can be captured in a graph);
 * scale NULL: s = 1, and the result is npvp_bias_act's bit for bit.  Layouts, acts and the vector rule are npvp_bias_act's; every
 * output element is written exactly once (no atomics, no workspace). */
int npvp_bias_act_scaled(const float* x, const float* bias, const float* scale, const float* residual, float* out, long long outer,
                         long long inner, int C, int layout, int act, npvp_stream_t stream);

/* ---- 3 x 3 convolutions of the frozen encoder on the matrix cores (csrc/conv3x3.hip; opt-in, to_device_layout(..., conv3x3="hip")):
 * the stride-1 "same" convolutions with C_in, C_out multiples of 64 - the spatial_conv of every Factorized3DConvAttn
 * (ref/models/submodules.py:23-27, zero padding) and the two convolutions of every ResnetBlock (ref/models/ResNetAutoEncoder.py:
 * 206-261, ReflectionPad2d(1)) - as ONE forward-only implicit-GEMM launch on channels-last frames, BatchNorm folded into w and bias:
 *   y[f,h,w,co] = act( sum_{kh,kw,ci} x[f, src(h,kh), src(w,kw), ci] * w[co,ci,kh,kw] + bias[co] ) (+ residual[f,h,w,co])
 * x [F][H][W][C_in], y and residual (nullable) [F][H][W][C_out], fp32; act as npvp_bias_act (0 none, 1 ReLU, 2 tanh, 3 sigmoid).
 * pad_mode 0: zero padding (an out-of-range tap contributes 0; H, W >= 1).  pad_mode 1: ReflectionPad2d(1) (-1 -> 1, H -> H - 2;
 * H, W >= 2).  The padding is index math (npvp_conv3x3_src): no padded copy, no im2col tensor, no separate epilogue pass.  Any
 * H x W; output tiles may straddle frame borders, taps never do.  F * H * W < 2^31.
 * Arithmetic: precision 6 of npvp_gemm_f32 ("f16x3": both operands scaled by the power of two of their amax slot and split into two
 * fp16 terms, three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation) on the GEMM M = F H W, N = C_out, K = 9 C_in with K
 * ordered (kh, kw, ci).  No split-K and no atomics on y: every output element is written exactly once and two runs give the same
 * bits.  Unlike the GEMM there is no per-row rescue: one scale per tensor (a pixel 2^18 below the tensor's bound keeps subnormal low
 * terms, i.e. an absolute error of 2^-40 of the bound).  Nothing here synchronises; every call can be captured in a graph. */
/* bytes of the weight planes: two fp16 terms of [C_out][9 C_in] */
long long npvp_conv3x3_planes_bytes(int C_in, int C_out);
/* w [C_out][C_in][3][3] (contiguous) -> planes[2 terms][9 C_in / 8][C_out][8 over k], k = (kh * 3 + kw) * C_in + ci - the F layout of
 * npvp_split_weight_f16 for the matrix [C_out][9 C_in], so a K-step of the kernel stays inside one tap -, scaled by the power of two
 * of w's amax, which is (re)computed into the slot w_amax (zeroed here first).  Once per frozen weight. */
int npvp_conv3x3_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, npvp_stream_t stream);
/* The convolution.  planes / w_amax: from npvp_conv3x3_planes; x_amax: the slot that bounds |x| (its producer's, or npvp_amax over
 * [F H W][C_in]); y_amax (nullable): receives the bound of the values stored to y, as the GEMM epilogues' c_amax does - the x_amax
 * of a following convolution at no extra pass.  workspace / ws_bytes: reserved, the kernel needs none (pass NULL, 0).  x, y, residual
 * and planes 16-byte aligned; y must not overlap x or residual. */
int npvp_conv3x3_f16(const float* x, const void* planes, const float* bias, const float* residual, float* y, int F, int H, int W,
                     int C_in, int C_out, int pad_mode, int act, const float* x_amax, const float* w_amax, float* y_amax,
                     void* workspace, long long ws_bytes, npvp_stream_t stream);
/* The plan npvp_conv3x3_f16 launches for a shape (it launches what the same planner returns): out6 = {tile variant (1: 128 x 128
 * output tiles, C_out % 128 == 0; 2: 128 x 64), rows per tile, columns per tile, row tiles, column tiles, workgroups (256 threads
 * each, one per tile)}.  Returns 0, or -1 for a shape the convolution refuses.  Pure function. */
int npvp_conv3x3_route(int F, int H, int W, int C_in, int C_out, int* out6);
/* out4 = {m0, m1, n0, n1}: the rows [m0, m1) of [F H W] and columns [n0, n1) of C_out that workgroup `block` of that plan stores -
 * the function the kernel itself calls.  Pure function. */
int npvp_conv3x3_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4);
/* Source coordinate of tap `tap` (0, 1, 2 = offsets -1, 0, +1) at output coordinate `c` of an axis of `extent` pixels, or -1 for a tap
 * that contributes 0 (zero padding) - the __host__ __device__ function the kernel calls (csrc/conv3x3_index.h).  -2: bad argument. */
int npvp_conv3x3_src(int c, int tap, int extent, int pad_mode);

/* ---- The stride-2 3 x 3 convolutions of the frozen encoder (opt-in, to_device_layout(..., down3x3="hip")): block1 and every
 * block{i}_conv (ref/models/ResNetAutoEncoder.py:75-106: Conv2d(kernel 3, stride 2, padding 1), BatchNorm folded, ReLU), the same
 * kernel, arithmetic, tiles and epilogue as npvp_conv3x3_f16 on the GEMM M = F Ho Wo, N = C_out, K = 9 C_in:
 *   y[f,oh,ow,co] = act( sum_{kh,kw,ci} x[f, 2 oh + kh - 1, 2 ow + kw - 1, ci] * w[co,ci,kh,kw] + bias[co] ) (+ residual[f,oh,ow,co])
 * x [F][H][W][C_in]; y and residual (nullable) [F][Ho][Wo][C_out] with Ho = (H + 1) / 2, Wo = (W + 1) / 2; a tap outside the H x W
 * grid contributes 0 (zero padding only: no pad_mode) - on an odd extent that is tap 2 of the last output as well as tap 0 of the
 * first.  C_in % 32 == 0 (block1 of the ngf = 32 encoders: one K-step per tap) and C_out % 64 == 0; F, H, W >= 1; H * W and
 * F * Ho * Wo < 2^31.  Every output element is written exactly once (no split-K, no atomics on y); two runs give the same bits. */
/* bytes of the weight planes, or -1 for channel counts outside the rule above */
long long npvp_conv3x3s2_planes_bytes(int C_in, int C_out);
/* npvp_conv3x3_planes under the stride-2 channel rule: the same layout planes[2 terms][9 C_in / 8][C_out][8 over k],
 * k = (kh * 3 + kw) * C_in + ci, the same kernel, w_amax zeroed and recomputed here.  Once per frozen weight. */
int npvp_conv3x3s2_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, npvp_stream_t stream);
/* The convolution.  H, W: the INPUT grid.  planes / w_amax: from npvp_conv3x3s2_planes; x_amax: the slot that bounds |x|; y_amax
 * (nullable): receives the bound of the values stored to y.  act as npvp_bias_act.  workspace / ws_bytes: reserved (NULL, 0).
 * x, y, residual and planes 16-byte aligned; y must not overlap x or residual. */
int npvp_conv3x3s2_f16(const float* x, const void* planes, const float* bias, const float* residual, float* y, int F, int H, int W,
                       int C_in, int C_out, int act, const float* x_amax, const float* w_amax, float* y_amax, void* workspace,
                       long long ws_bytes, npvp_stream_t stream);
/* The plan npvp_conv3x3s2_f16 launches: out8 = the six fields of npvp_conv3x3_route for M = F Ho Wo, then Ho, Wo.  Returns 0, or -1
 * for a shape the convolution refuses.  Pure function. */
int npvp_conv3x3s2_route(int F, int H, int W, int C_in, int C_out, int* out8);
/* out4 = {m0, m1, n0, n1}: the rows [m0, m1) of [F Ho Wo] and columns [n0, n1) of C_out that workgroup `block` stores.  Pure function. */
int npvp_conv3x3s2_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4);
/* Source coordinate 2 o + tap - 1 of tap `tap` (0, 1, 2) at OUTPUT coordinate `o` (0 <= o < (extent + 1) / 2) of an axis of `extent`
 * input pixels, or -1 for a tap that contributes 0 - the __host__ __device__ function the kernel calls.  -2: bad argument. */
int npvp_conv3x3s2_src(int o, int tap, int extent);

/* ---- The transposed 3 x 3 convolutions of the frozen decoder (opt-in, to_device_layout(..., up3x3="hip")): every
 * ConvTranspose2d(kernel 3, stride 2, padding 1, output_padding 1), BatchNorm folded, ReLU (ref/models/ResNetAutoEncoder.py:148-204),
 * a third form of the same kernel (arithmetic, tiles, LDS stages and epilogue of npvp_conv3x3_f16), forward:
 *   y[f,oh,ow,co] = act( sum_{ci, (s, k): oh = 2 sh - 1 + kh, ow = 2 sw - 1 + kw} x[f,sh,sw,ci] * w[ci,co,kh,kw] + bias[co] )
 * x [F][H][W][C_in] -> y [F][2H][2W][C_out], fp32, channels-last; no residual.  The output splits by parity: pixel (2 i + a, 2 j + b)
 * belongs to class (a, b) and input-grid position (i, j); per axis parity 0 has one tap (kernel index 1, source i), parity 1 two
 * (kernel index 2 at source i; kernel index 0 at source i + 1, nothing at the far edge) - 1, 2, 2 and 4 taps per class, 9 per 4 outputs,
 * no multiplication by an inserted zero.  ONE launch: a workgroup owns a 128-row x 128- or 64-column tile of M = F H W input-grid rows
 * of ONE class, K = taps * C_in; the 4-tap class's workgroups come first in launch order.  C_in % 32 == 0, C_out % 64 == 0;
 * F, H, W >= 1; F * 2H * 2W < 2^31.  Every output element is written exactly once (no split-K, no atomics on y, no memset); two runs
 * give the same bits.  The input gradient of this convolution is npvp_conv3x3s2_f16 on the same weight memory read as a Conv2d
 * weight [out = C_in][in = C_out][3][3] (planes from npvp_conv3x3s2_planes(w, C_out, C_in, ...)). */
/* taps of an axis at output parity 0 / 1 (1 / 2); -2: bad argument */
int npvp_convt3x3s2_ntaps(int parity);
/* kernel index (0, 1, 2) of tap t (0 <= t < ntaps) at that parity; -2: bad argument */
int npvp_convt3x3s2_tap(int parity, int t);
/* source coordinate of tap t at input-grid position i (0 <= i < extent) and that parity, or -1 for a tap that contributes 0 - the
 * __host__ __device__ functions the kernel calls (csrc/conv3x3_index.h).  -2: bad argument. */
int npvp_convt3x3s2_src(int i, int parity, int t, int extent);
/* bytes of the weight planes, or -1 for channel counts outside the rule above */
long long npvp_convt3x3s2_planes_bytes(int C_in, int C_out);
/* w [C_in][C_out][3][3] (the ConvTranspose2d layout, contiguous) -> planes[2 terms][9 C_in / 8][C_out][8 over k],
 * k = (kh * 3 + kw) * C_in + ci (kernel index unflipped): npvp_conv3x3_planes' layout and arithmetic; a class reads the K-steps of its
 * taps.  w_amax is zeroed and recomputed here.  Once per frozen weight. */
int npvp_convt3x3s2_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, npvp_stream_t stream);
/* The convolution.  H, W: the INPUT grid.  planes / w_amax: from npvp_convt3x3s2_planes; x_amax: the slot that bounds |x|; y_amax
 * (nullable): receives the bound of the values stored to y.  act as npvp_bias_act.  workspace / ws_bytes: reserved (NULL, 0).
 * x, y and planes 16-byte aligned; y must not overlap x. */
int npvp_convt3x3s2_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in, int C_out,
                        int act, const float* x_amax, const float* w_amax, float* y_amax, void* workspace, long long ws_bytes,
                        npvp_stream_t stream);
/* The plan npvp_convt3x3s2_f16 launches: out8 = {tile variant, rows per tile, columns per tile, row tiles per class, column tiles,
 * workgroups of the launch (4 classes x row tiles x column tiles), 2H, 2W}.  Returns 0, or -1 for a refused shape.  Pure function. */
int npvp_convt3x3s2_route(int F, int H, int W, int C_in, int C_out, int* out8);
/* out6 = {a, b, m0, m1, n0, n1}: the class (row parity a, column parity b), the rows [m0, m1) of [F H W] input-grid positions and
 * the columns [n0, n1) of C_out that workgroup `block` stores - the function the kernel itself calls.  Pure function. */
int npvp_convt3x3s2_tile(int F, int H, int W, int C_in, int C_out, int block, int* out6);

/* ---- The 7 x 7 tail of the frozen decoder (opt-in, to_device_layout(..., tail7x7="hip"); csrc/conv7x7.hip): ReflectionPad2d(3) ->
 * Conv2d(C_in, C_out, 7) -> Tanh / Sigmoid (ref/models/ResNetAutoEncoder.py:148-204), forward and input gradient:
 *   y[f,co,h,w] = act( bias[co] + sum_{ci,kh,kw} x[f, refl_H(h + kh - 3), refl_W(w + kw - 3), ci] * w[co,ci,kh,kw] )
 * x [F][H][W][C_in] fp32 channels-last -> y [F][C_out][H][W] fp32 NCHW (the layout the decoder returns); no padded copy of x.
 * The kernel's column index is folded into N: Z[(f,h,w')][(kw,co)] = sum_{kh,ci} x[f, refl_H(h+kh-3), w', ci] w[co,ci,kh,kw] is a
 * GEMM with M = F H W, N = 7 * 4 = 32 (co padded to 4), K = 7 C_in ordered (kh, ci), and y = act(bias + sum_kw Z[(f,h,refl_W(w+kw-3))][(kw,co)])
 * is summed inside the workgroup, which owns whole image rows (W <= 128: 128 / W rows of the F * H rows) or one row's segment of 122
 * columns with a halo of 3 Z columns per side (W > 128).  f16x3 arithmetic as npvp_conv3x3_f16.  C_in % 32 == 0 (up to 4096),
 * 1 <= C_out <= 4, H, W >= 4, F * H * W < 2^31.  Every element of y is written exactly once (no atomics, no memset); two runs give
 * the same bits.  The 7 x 7 stem of the ENCODER is not routed. */
/* source coordinate of tap (0..6) at output coordinate c (0 <= c < extent, extent >= 4) of an axis behind ReflectionPad2d(3) - the
 * __host__ __device__ function the kernel calls (csrc/conv7x7_index.h).  -2: bad argument. */
int npvp_tail7x7_src(int c, int tap, int extent);
/* the adjoint: the output coordinate o with npvp_tail7x7_src(o, tap, extent) == s; which 0: the straight one (o = s + 3 - tap),
 * which 1: the one mirror image (low edge for tap <= 2, high edge for tap >= 4).  The coordinate, -1 when there is none, -2: bad
 * argument. */
int npvp_tail7x7_adj_src(int s, int tap, int extent, int which);
/* bytes of the weight planes (the forward's and the input gradient's have the same size), or -1 for channel counts outside the rule */
long long npvp_tail7x7_planes_bytes(int C_in, int C_out);
/* w [C_out][C_in][7][7] (contiguous) -> forward planes [2 terms][7 C_in / 8][32][8 over k], k = kh * C_in + ci, column kw * 4 + co
 * (zero columns for co >= C_out and kw = 7).  w_amax is zeroed and recomputed here.  Once per frozen weight. */
int npvp_tail7x7_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, npvp_stream_t stream);
/* the same weight -> the input gradient's planes [2 terms][28][C_in][8 over k], k = kh * 32 + kw * 4 + co, column ci, at the scale
 * of the SAME slot w_amax (read, not written: call npvp_tail7x7_planes first). */
int npvp_tail7x7_dgrad_planes(const float* w, int C_in, int C_out, void* planes, const float* w_amax, npvp_stream_t stream);
/* The forward.  act: 0 none, 2 tanh, 3 sigmoid.  workspace / ws_bytes: reserved (NULL, 0).  x, y and planes 16-byte aligned. */
int npvp_tail7x7_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in, int C_out, int act,
                     const float* x_amax, const float* w_amax, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* The plan npvp_tail7x7_f16 launches: out8 = {image rows per tile, column segments per row, output columns per segment, row tiles,
 * workgroups, Z rows per tile (128), Z columns (32), K-steps}.  Returns 0, or -1 for a refused shape.  Pure function. */
int npvp_tail7x7_route(int F, int H, int W, int C_in, int C_out, int* out8);
/* out6 = {r0, r1, w0, w1, z0, z1}: the image rows [r0, r1) of the F * H rows, the output columns [w0, w1) and the Z window [z0, z1)
 * of workgroup `block` - the function the kernel itself calls.  Pure function. */
int npvp_tail7x7_tile(int F, int H, int W, int C_in, int C_out, int block, int* out6);
/* The input gradient: dz [F][C_out][H][W] (g * act'(y), npvp_act_bwd on the planar tensors) -> dx [F][H][W][C_in] channels-last,
 *   dx[(f,s,t)][ci] = sum_kh sum_{(kw,co)} A[(f,s,t)][kh][(kw,co)] w[co,ci,kh,kw],  A = the sum of dz over npvp_tail7x7_adj_src's
 * at most 2 x 2 output pixels, taken in fp32 before the fp16 split.  M = F H W rows in tiles of 128, C_in in tiles of 64 (32 when
 * C_in % 64 != 0), K = 7 steps of 32.  dz_amax: the slot that bounds |dz|.  Written exactly once, no atomics. */
int npvp_tail7x7_dgrad_f16(const float* dz, const void* planes, float* dx, int F, int H, int W, int C_in, int C_out, const float* dz_amax,
                           const float* w_amax, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* out6 = {tile variant (1: 64 columns, 2: 32), rows per tile, columns per tile, row tiles, column tiles, workgroups} */
int npvp_tail7x7_dgrad_route(int F, int H, int W, int C_in, int C_out, int* out6);
/* out4 = {m0, m1, n0, n1}: the rows of [F H W] and the columns of C_in that workgroup `block` of the input gradient stores */
int npvp_tail7x7_dgrad_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4);

/* ---- The 7 x 7 stem of the frozen encoder (opt-in, to_device_layout(..., stem7x7="hip"); csrc/conv7x7.hip): ReflectionPad2d(3) ->
 * Conv2d(C_in, C_out, 7) -> BatchNorm (folded) -> ReLU (ref/models/ResNetAutoEncoder.py:51-146), forward only (the encoder runs under
 * no_grad in Stage 2):
 *   y[f,h,w,co] = act( bias[co] + sum_{kh,kw,ci} x[f, ci, refl_H(h + kh - 3), refl_W(w + kw - 3)] * w[co,ci,kh,kw] )
 * x [F][C_in][H][W] fp32 PLANAR (NCHW, the layout the data path hands the encoder; for C_in = 1 also the channels-last memory) ->
 * y [F][H][W][C_out] fp32 channels-last; refl is npvp_tail7x7_src; no padded copy of x.  An implicit GEMM with M = F H W in tiles of
 * 128, N = C_out in tiles of 64 (32 when C_out % 64 != 0) and the dense K order k = (kh * 7 + kw) * C_in + ci, zero-padded from
 * 49 C_in to a multiple of 32 (2 / 4 / 5 / 7 K-steps for C_in = 1 / 2 / 3 / 4).  f16x3 arithmetic as npvp_conv3x3_f16.
 * 1 <= C_in <= 4, C_out a positive multiple of 32 up to 4096, F >= 1, H, W >= 4, F * H * W < 2^31; y and planes 16-byte aligned.
 * Every element of y is written exactly once (no atomics on y, no memset); two runs give the same bits. */
/* out3 = {kh, kw, ci} of K index k - the __host__ __device__ function the gather and the planes kernel call (csrc/conv7x7_index.h).
 * Returns 0; 1 for an index of the zero padding (49 C_in <= k < K_pad; out3 = {-1, -1, -1}); -2: bad argument (out3 untouched). */
int npvp_stem7x7_k(int C_in, int k, int* out3);
/* bytes of the weight planes, or -1 for channel counts outside the rule */
long long npvp_stem7x7_planes_bytes(int C_in, int C_out);
/* w [C_out][C_in][7][7] (contiguous) -> planes [2 terms][K_pad / 8][C_out][8 over k] (zero for the padding of K).  w_amax is zeroed
 * (by a kernel, not a memset node) and recomputed here.  Once per frozen weight. */
int npvp_stem7x7_planes(const float* w, int C_in, int C_out, void* planes, float* w_amax, npvp_stream_t stream);
/* The forward.  act: 0 none, 1 ReLU.  y_amax: the slot that receives the bound of the stored values, or NULL.  workspace / ws_bytes:
 * reserved (NULL, 0). */
int npvp_stem7x7_f16(const float* x, const void* planes, const float* bias, float* y, int F, int H, int W, int C_in, int C_out, int act,
                     const float* x_amax, const float* w_amax, float* y_amax, void* workspace, long long ws_bytes, npvp_stream_t stream);
/* The plan npvp_stem7x7_f16 launches: out7 = {tile variant (1: 64 columns, 2: 32), rows per tile, columns per tile, row tiles, column
 * tiles, workgroups, K-steps}.  Returns 0, or -1 for a refused shape (out7 untouched).  Pure function. */
int npvp_stem7x7_route(int F, int H, int W, int C_in, int C_out, int* out7);
/* out4 = {m0, m1, n0, n1}: the rows of [F H W] and the columns of C_out that workgroup `block` stores - the function the kernel itself
 * calls.  Pure function. */
int npvp_stem7x7_tile(int F, int H, int W, int C_in, int C_out, int block, int* out4);

/* ---- Stage-1 autoencoder training (csrc/ae_train.hip): LitAE.training_step / shared_step (ref/models/ResNetAutoEncoder.py:13-49)
 * through ResnetEncoder / ResnetDecoder (ref :51-204) and NonLocalAttenion2D (ref/models/submodules.py:98-176); the convolutions
 * stay MIOpen's.  Every entry point is deterministic (fixed-order sums, no atomics) and needs no zero-filled buffer.
 * BatchNorm2d in training mode + ReLU (+ skip-add), replacing `norm_layer(c), nn.ReLU(True)` of ref :76-130 / :168-175 / :239-249
 * and the `+ x` of ref/models/submodules.py:80-93 / ResNetAutoEncoder.py:259-261:
 *   layout 0: x [outer = N*H*W][inner = C] (channels-last), C a power of two in [4, 1024]; layout 1: x [outer = N*C][inner = H*W],
 *   H*W % 4 == 0.  Buffers 16-byte aligned.  workspace >= npvp_bn_workspace_bytes(C).
 * bn_stats: sums[2][C] (double) = per-channel [sum x, sum x^2]  (a data-parallel caller all-reduces these and n, then applies);
 * bn_act_apply: mean / rstd from sums over `count` elements per channel (sums == NULL: from running_mean / running_var, eval mode),
 *   running statistics updated in place as torch does (momentum, unbiased variance; NULL = not tracked), then
 *   y = act((x - mean) rstd w + b) + residual  (act 0 none, 1 ReLU; residual nullable); mean / rstd [C] are saved for the backward;
 * bn_act_bwd: g' = g * act'(.) (the ReLU mask recomputed from x with the forward's arithmetic), dw = sum g' xhat, db = sum g',
 *   dx = w rstd (g' - db/n - xhat dw/n) (train = 1) or w rstd g' (train = 0: running statistics).  The skip-add's gradient is g itself. */
int npvp_bn_workspace_bytes(int C);
int npvp_bn_stats(const float* x, long long outer, long long inner, int C, int layout, double* sums, void* workspace, long long ws_bytes,
                  npvp_stream_t stream);
int npvp_bn_act_apply(const float* x, const float* w, const float* b, const float* residual, const double* sums, long long count,
                      float eps, float momentum, float* running_mean, float* running_var, long long outer, long long inner, int C,
                      int layout, int act, float* y, float* mean, float* rstd, npvp_stream_t stream);
int npvp_bn_act_bwd(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b, long long outer,
                    long long inner, int C, int layout, int act, int train, float* dx, float* dw, float* db, void* workspace,
                    long long ws_bytes, npvp_stream_t stream);
/* Synchronised BatchNorm for data-parallel Stage-1 training - what Lightning's `sync_batchnorm=True` beside the DDP strategy
 * (ref/train_AutoEncoder_lightning.py:40-42) makes of the BatchNorm2d layers of ref/models/ResNetAutoEncoder.py:76-130,168-175,239-249:
 * the two passes above, cut where the per-channel sums cross the ranks.  The caller all-reduces (sum) the double buffers in between.
 * bn_act_apply_sync: bn_act_apply in training mode from stat[2C+1] (device, double) = [sum x (C), sum x^2 (C), n]: bn_stats' sums
 *   followed by the element count per channel, all three summed over the ranks.  n is read on the device (shards may be uneven);
 *   mean, rstd, the running-statistic update (unbiased variance with the TOTAL n) and the apply pass follow from it.
 * bn_bwd_sums: the first half of bn_act_bwd over this rank's rows: sums[2C] (device, double) = [sum g' (C), sum g' xhat (C)], and
 *   dw / db (float) from these LOCAL sums - the gradient all-reduce (mean over ranks) completes them as it does every other parameter's.
 * bn_act_bwd_apply: the second half: dx = w rstd (g' - sum g'/n - xhat sum g' xhat / n) from the all-reduced sums[2C] and the device
 *   count n (one double: stat + 2C kept from the forward).
 * bn_act_apply / bn_act_bwd are these calls composed, on a host count and on sums in bn_act_bwd's own workspace; their dx pass reads
 * the float dw / db and a host 1/n where bn_act_bwd_apply rounds the double sums and 1 / n itself, to the same floats.  So given this
 * rank's own sums and count, the three calls produce the bits of bn_act_apply / bn_act_bwd (y, mean, rstd, running statistics, dx, dw,
 * db).  Same layouts, shape rules and alignment as above;
 * bn_bwd_sums needs the whole npvp_bn_workspace_bytes(C), bn_stats / bn_act_bwd accept what their problem's parts take; deterministic,
 * no zero-filled buffer. */
int npvp_bn_act_apply_sync(const float* x, const float* w, const float* b, const float* residual, const double* stat, float eps,
                           float momentum, float* running_mean, float* running_var, long long outer, long long inner, int C, int layout,
                           int act, float* y, float* mean, float* rstd, npvp_stream_t stream);
int npvp_bn_bwd_sums(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b, long long outer,
                     long long inner, int C, int layout, int act, double* sums, float* dw, float* db, void* workspace, long long ws_bytes,
                     npvp_stream_t stream);
int npvp_bn_act_bwd_apply(const float* g, const float* x, const float* mean, const float* rstd, const float* w, const float* b,
                          const double* sums, const double* count, long long outer, long long inner, int C, int layout, int act, float* dx,
                          npvp_stream_t stream);
/* ReflectionPad2d(P) (ref/models/ResNetAutoEncoder.py:72, :187, :234-236): layout 1 x [planes = N*C][H][W] -> y [planes][H+2P][W+2P];
 * layout 0 x [planes = N][H][W][C] -> y [N][H+2P][W+2P][C].  backward = 1: x is the padded gradient, y the input gradient, each
 * input pixel the fixed-order sum of the padded pixels that read it (no atomics).  1 <= P < H, W. */
int npvp_reflect_pad(const float* x, float* y, int planes, int H, int W, int C, int P, int layout, int backward, npvp_stream_t stream);
/* Non-local attention core of NonLocalAttenion2D.forward (ref/models/submodules.py:150-170): o = softmax(q k^T) v per frame, scores
 * NOT scaled, k / v = 2x2 max-pool (stride 2) of the projections over the H x W grid; F frames of H*W rows each.  q [F*H*W][ldq],
 * k [F*H*W][ldk] (first A columns), v [F*H*W][ldv] (first V columns) are the UNPOOLED projections; o [F*H*W][ldo]; lse [F*H*W] is
 * saved for the backward.  (A, V) in {(8,32), (16,64), (32,128), (64,256)} (C = 64..512, a = C/8, v = C/2), H even, W a power of
 * two, H*W in {4096, 1024, 256, 64} respectively (the grids of the five AE configs).  The score matrix stays on chip.
 * bwd: dq, and dk / dv of the unpooled projections: each window's gradient at its arg-max (first maximum in row-major order, as torch),
 * 0 at the other three positions.  D [2][F*H*W] is scratch (rowsum(go * o) and 1 / rowsum(P), summed in double).  dq / dk / dv may be column slices of one buffer. */
int npvp_nonlocal_attn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                           long long ldo, float* lse, int F, int H, int W, int A, int V, npvp_stream_t stream);
int npvp_nonlocal_attn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, const float* go,
                           long long ldgo, const float* lse, float* D, float* dq, long long lddq,
                           float* dk, long long lddk, float* dv, long long lddv, int F, int H, int W, int A, int V, npvp_stream_t stream);
/* The same core on ANY grid: F >= 1, H >= 2, W >= 2 (odd, rectangular, not a power of two), F*H*W < 2^31, (A, V) from the same
 * table; same argument lists, same tie rule, same lse, same D [2][F*H*W] scratch.  Pooled grid Hp = H/2, Wp = W/2 (floor, as
 * nn.MaxPool2d((2,2), stride=2)), Lk = Hp*Wp >= 1 keys; every query row attends.  Rows of an odd last line / column belong to no
 * window: their dk / dv are exactly 0, written by a kernel (no memset), so every element of dq / dk / dv is written exactly once.
 * A shape npvp_nonlocal_attn_fwd/bwd accept launches what they launch (the exact-tile form of the kernels, bit-identical results);
 * every other shape the general form of the same kernels - same tiles, thread maps and summation order, partial last query / key tiles masked
 * (masked key: score -inf, P = 0; masked query: no store, no contribution to dk / dv).  Deterministic, no atomics, no workspace.
 * NPVP_NL_GRID_GENERAL=1 in the environment (read once) sends the config shapes to the general form too: a measurement aid. */
int npvp_nonlocal_attn_grid_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                                long long ldo, float* lse, int F, int H, int W, int A, int V, npvp_stream_t stream);
int npvp_nonlocal_attn_grid_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                const float* go, long long ldgo, const float* lse, float* D, float* dq, long long lddq,
                                float* dk, long long lddk, float* dv, long long lddv, int F, int H, int W, int A, int V,
                                npvp_stream_t stream);
/* Temporal non-local attention: the core of NonLocalAttenion1D.forward (ref/models/submodules.py:221-243) as Factorized3DConvAttn
 * (learn_3d=True, :62-66, :86-91) applies it to the T frames of every pixel: o = softmax(q k^T) v over a pixel's T rows, scores NOT
 * scaled, one head.  Operands are read in place from channels-last token rows: row(n, t, p) = (n*T + t)*HW + p for clip n < N, frame
 * t < T, pixel p < HW; q [rows][ldq] and k [rows][ldk] (first A columns), v [rows][ldv] and o [rows][ldo] (first V columns),
 * lse [rows] saved for the backward.  (A, V) in {(8,32), (16,64), (32,128), (64,256)}; 1 <= T <= 32 (a pixel's T x T scores are
 * not tiled over the keys; every shipped clip length is <= 30); N, HW >= 1; N*T*HW < 2^31; leading dimensions multiples of 4
 * floats and pointers 16-byte aligned (float4 accesses).  Anything else returns -1 with the entry point's name and the offending
 * value in npvp_last_error.
 * bwd: P is recomputed from q, k and lse and its row normalised (Phat = P / sum P); D = rowsum(Phat * dP).  A pixel's dq, dk and dv
 * depend on that pixel's rows only, so one kernel writes all three: no workspace, no atomics, no memset, every element of
 * dq / dk / dv (first A / A / V columns of their rows) written exactly once, bit-identical on repeated runs.  dq / dk / dv may be
 * column slices of one buffer.  At T = 1: o = v, dq = dk = 0, dv = go exactly. */
int npvp_temporal_attn_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                           long long ldo, float* lse, int N, int T, int HW, int A, int V, npvp_stream_t stream);
int npvp_temporal_attn_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, const float* go,
                           long long ldgo, const float* lse, float* dq, long long lddq, float* dk, long long lddk, float* dv,
                           long long lddv, int N, int T, int HW, int A, int V, npvp_stream_t stream);
/* The same core for ANY clip length T >= 1 (N*T*HW < 2^31 is the only bound): same argument rules and refusals, plus the scratch
 * D [2][N*T*HW] of the backward (row sums of P, then D = rowsum(Phat * dP); non-null, 16-byte aligned, contents undefined on entry).
 * T <= 32 launches what npvp_temporal_attn_fwd/bwd launch (bit-identical results, D untouched).  Above that the keys are tiled: a
 * workgroup owns a tile of pixels x a tile of <= 32 frames (16 at (64,256); the clip cut into the fewest equal tiles) and walks the
 * other side of the T x T scores in tiles of the same size, so LDS per workgroup stays under 64 KB whatever T is.  fwd: one launch, two sweeps over the key tiles (running max
 * and sum, rescaled when the max rises; then exp(s - m) / l * v).  bwd: two launches - dq per (pixel tile, query tile), which also
 * writes D; dk and dv per (pixel tile, key tile) over the query tiles.  A key past T has P = 0, a query past T stores and contributes
 * nothing.  No atomics, no memset, no workspace but D; every element of o / lse / dq / dk / dv written exactly once; sums in tile
 * order, bit-identical on repeated runs; nothing read or written outside the first A / A / V columns of the operands' rows. */
int npvp_temporal_attn_long_fwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv, float* o,
                                long long ldo, float* lse, int N, int T, int HW, int A, int V, npvp_stream_t stream);
int npvp_temporal_attn_long_bwd(const float* q, long long ldq, const float* k, long long ldk, const float* v, long long ldv,
                                const float* go, long long ldgo, const float* lse, float* D, float* dq, long long lddq, float* dk,
                                long long lddk, float* dv, long long lddv, int N, int T, int HW, int A, int V, npvp_stream_t stream);

/* ---- the data-parallel exchange: all-reduce(mean) of the parameter gradients, RCCL over xGMI, one process per GPU.
 * Replaces what the reference gets from Lightning's DDP strategy (ref/train_Predictor_lightning.py:40-42: strategy = 'ddp' over
 * `devices` GPUs) for a host without torch.distributed.  Protocol: rank 0 calls npvp_dp_unique_id and carries the 128
 * bytes to every rank (file, socket, MPI, a torch.distributed store ...); every rank, with its device current, calls npvp_dp_init
 * (collective).  Per step: order `side` after the producers of a bucket of the flat gradient buffer, npvp_dp_allreduce_async(bucket,
 * n, side) - in place, mean over the ranks, same buckets in the same order on every rank, the host never blocks - and before the
 * optimiser npvp_dp_wait(compute): the compute stream waits on the device for every reduction enqueued so far.  npvp_dp_finalize
 * drains and releases the communicator.  RCCL is found at run time (the copy already loaded in the process, else $NPVP_RCCL_LIB, else
 * librccl.so.1 on the loader's path); a process that never calls these never loads it.  One communicator per process. */
int npvp_dp_unique_id(void* id_out_128_bytes);
int npvp_dp_init(int rank, int world, const void* unique_id_128_bytes);
int npvp_dp_world(void); /* 0 before npvp_dp_init */
int npvp_dp_rank(void);  /* -1 before npvp_dp_init */
int npvp_dp_allreduce_async(float* bucket, size_t n, npvp_stream_t side);
int npvp_dp_wait(npvp_stream_t compute);
int npvp_dp_finalize(void);

#ifdef __cplusplus
}
#endif
#endif
