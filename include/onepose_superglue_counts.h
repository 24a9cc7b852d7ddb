/* Variable-count SuperGlue batches of libonepose_hip -- included by onepose_hip.h.
 *
 * The declarations of this family live in a header of their own: onepose_hip.h's own
 * declarations are the 99 functions of ABI 9 (the table tests/test_binding.py pins), and neither
 * onepose_abi_version() (9) nor onepose_superglue_version() (1) is bumped: nothing that existed
 * changed.  The Python binding parses this file into _lib.FAMILIES["onepose_superglue_counts.h"]
 * and calls its functions by parameter name like every other.
 *
 * ------------------------------------------------------------------------------------ *
 * One matcher call for pairs of unequal keypoint counts and image sizes
 *   The SuperGlue entry points of onepose_hip.h batch only pairs with the same n0, n1 and image
 *   sizes.  Their callers feed them SuperPoint output, where that almost never holds: the 2D
 *   object detector's reference views and the pairs of sparse reconstruction.  Each entry point
 *   below is its sibling plus per-sample counts (and, for the forward, per-sample image sizes).
 * Versioned on its own: onepose_superglue_counts_version() returns 1.
 *
 * Layout: padded and uniform.  Every tensor keeps its sibling's shape and batch strides, with
 * n0 / n1 (n / m) the batch MAXIMA.  counts arrays are [batch] int32 DEVICE arrays: how many
 * leading tokens of each sample are real.  hw arrays are [batch, 2] int32 device arrays of
 * (h, w).  Any of them may be NULL: a NULL counts array means every sample has the full n, a
 * NULL hw array means the scalar sizes apply to every sample.
 *
 * Counts and sizes are read on the device: a count is clamped to [0, n], an h or w below 1 is read
 * as 1.  Grids are sized from the maxima, nothing is read back on the host, and every entry is a
 * fixed launch sequence for given (batch, n0, n1): capturable in a graph, and a replay after the
 * arrays changed in place computes with the new counts.  The token GEMMs and the score GEMM run
 * over the padded rows.
 *
 * Padding is harmless: no output bit depends on what lies in input slots past a count, on what
 * the workspace held before the call, or on the other samples of the batch (for given maxima;
 * the maxima choose the launch shapes).  The input stage writes zero rows for the padded tokens
 * and attention writes zeros for padded query rows; keys, Sinkhorn rows and columns and the
 * mutual check stop at each sample's own counts, and norm, log_mu and log_nu are those of the
 * sample's own m and n, computed in float64 on the device.
 *
 * With NULL arrays, or counts all equal to the maxima and hw equal to the scalars, an entry gives
 * the bits of its sibling.
 * ------------------------------------------------------------------------------------ */
#ifndef ONEPOSE_SUPERGLUE_COUNTS_H
#define ONEPOSE_SUPERGLUE_COUNTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int onepose_superglue_counts_version(void);

/* onepose_superglue_match over pairs of unequal counts and sizes.  Per image i: desc_i
 * [batch, 256, n_i], kpts_i [batch, n_i, 2] (x, y pixels), scores_i [batch, n_i], each with a
 * batch stride in elements (stride 0 = shared by the batch), n_i the batch maximum; counts_i
 * [batch] int32 or NULL; hw_i [batch, 2] int32 (h, w) or NULL, in which case h_i, w_i are the
 * sizes normalize_keypoints reads for every sample (they must be positive either way).
 * sinkhorn_iters >= 0, match_threshold and precision (ONEPOSE_PREC_FP32 only) as in the sibling;
 * the workspace is that of onepose_superglue_workspace_bytes(batch, n0, n1), 256-byte aligned.
 * Outputs keep their padded shapes: matches0 [batch, n0] / matches1 [batch, n1] int64 and
 * mscores0 / mscores1 fp32; entries past a sample's count are -1 and 0.  A sample with either
 * count 0 gives -1 and 0 everywhere (the reference's empty branch, :269-276, for that pair
 * alone) and does not disturb the others.  log_assignment [batch, n0+1, n1+1] fp32 or NULL:
 * sample b's (c0+1) x (c1+1) matrix is the top-left block of its slot, with the dustbin row at c0
 * and the dustbin column at c1; everything outside the block -- the whole slot of a sample with
 * an empty side -- is left as the caller gave it.
 * Host refusals in the sibling's order (precision: ONEPOSE_ERR_UNSUPPORTED; shape, iterations,
 * image sizes, null inputs / outputs, negative strides: ONEPOSE_ERR_INVALID), then one more: a
 * side with a batch stride of 0 together with a non-null counts array for that side is
 * ONEPOSE_ERR_INVALID (a shared side has one count, its n); then the workspace checks
 * (ONEPOSE_ERR_INVALID, ONEPOSE_ERR_WORKSPACE). */
int onepose_superglue_match_counts(const void* packed_weights,
                                   const float* desc0, int64_t desc0_bstride,
                                   const float* kpts0, int64_t kpts0_bstride,
                                   const float* scores0, int64_t scores0_bstride,
                                   const float* desc1, int64_t desc1_bstride,
                                   const float* kpts1, int64_t kpts1_bstride,
                                   const float* scores1, int64_t scores1_bstride,
                                   int batch, int n0, int n1, int h0, int w0, int h1, int w1,
                                   const int* counts0, const int* counts1, const int* hw0,
                                   const int* hw1, int sinkhorn_iters, float match_threshold,
                                   int precision, int64_t* matches0, int64_t* matches1,
                                   float* mscores0, float* mscores1, float* log_assignment,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* onepose_log_optimal_transport with per-sample sizes: scores [batch, m, n] (bstride elements),
 * counts_m / counts_n [batch] int32 or NULL -> out [batch, m+1, n+1]: sample b's
 * (m_b+1) x (n_b+1) result Z + u + v - norm (norm, log_mu, log_nu of m_b and n_b) is the top-left
 * block of its slot, the dustbin row at m_b and the dustbin column at n_b; everything outside the
 * block, and the whole slot of a sample with m_b = 0 or n_b = 0, is left as the caller gave it.
 * The workspace is that of onepose_log_optimal_transport_workspace_bytes(batch, m, n).
 * Deterministic: no atomics, every merge in a fixed order. */
int onepose_log_optimal_transport_counts(const float* scores, int64_t scores_bstride, int batch,
                                         int m, int n, const int* counts_m, const int* counts_n,
                                         float alpha, int iters, float* out, void* workspace,
                                         size_t workspace_bytes, void* stream);

/* onepose_mha_softmax with per-sample sizes: q [batch, n, 256], k, v [batch, m, 256], token-major
 * with head-major channels (4 heads x 64), counts_q / counts_k [batch] int32 or NULL -> out
 * [batch, n, 256]: rows below counts_q[b] are softmax(q k^T / 8) v per head over the sample's
 * first counts_k[b] keys; rows past counts_q[b], and every row of a sample with counts_k[b] = 0,
 * are written as zeros.  Batch strides in elements (multiples of 4; 0 = shared input); pointers
 * 16-byte aligned. */
int onepose_mha_softmax_counts(const float* q, int64_t q_bstride, const float* k, int64_t k_bstride,
                               const float* v, int64_t v_bstride, int batch, int n, int m,
                               const int* counts_q, const int* counts_k, float* out,
                               int64_t out_bstride, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* ONEPOSE_SUPERGLUE_COUNTS_H */
