/* Per-sample keypoint counts for the 2D-3D matcher of libonepose_hip -- included by onepose_hip.h.
 *
 * The declarations of this family live in a header of their own: onepose_hip.h's own
 * declarations are the 99 functions of ABI 9 (the table tests/test_binding.py pins), and
 * onepose_abi_version() (9) is not bumped: nothing that existed changed.  The Python binding
 * parses this file into _lib.FAMILIES["onepose_match_counts.h"] and calls its functions by
 * parameter name like every other.
 *
 * ------------------------------------------------------------------------------------ *
 * One cached matcher call for frames of unequal keypoint counts
 *   onepose_match_cached* takes n1 as a host integer and treats every one of the n1 query slots
 *   as a keypoint.  Its callers feed it SuperPoint output, which fills its top-k only on dense
 *   images.  Each entry point below is its sibling plus counts2d: how many leading tokens of each
 *   sample's 2D side are real.  Only the 3D side's length is a property of the object, so only the
 *   2D side gets counts.
 * Versioned on its own: onepose_match_counts_version() returns 1.
 *
 * Scope: ONEPOSE_PREC_FP32 only (the other precisions: ONEPOSE_ERR_UNSUPPORTED before anything is
 * launched); the cached path; both descriptor dtypes; ONEPOSE_OBJ_GAT_TABLES allowed; any batch
 * size (both KV fold paths); whole frames (the sharded matcher has no counts).
 *
 * Layout: padded and uniform.  Every tensor keeps the uniform call's shape and strides, with n1
 * the batch MAXIMUM.  counts2d is a [batch] int32 DEVICE array, or NULL: every sample is full.
 *
 * Read on the device: a count is clamped to [0, n1] by every kernel that reads it.  Nothing is
 * read back on the host.  Grids, the launch sequence and the workspace plan depend on (batch, n1,
 * n3, num_leaf, flags, stage range) only -- the one choice the pointer makes is between a
 * kernel and its counts instantiation, same grid -- so a call is capturable in a graph, and a
 * replay after counts2d changed in place computes with the new counts.
 *
 * No waiting on a device count: the number of arrivals that every ticket or arrival counter
 * expects (MLP conv 1's InstanceNorm finalize) is a function of the host arguments.  Workgroups
 * whose rows all lie past the count run, store their rows, write (0, 0) partials and arrive like
 * any other; nothing spins on, or sizes a loop of arrivals by, a value read from counts2d.
 *
 * What a count c means: sample b is matched as if its 2D side had c tokens.
 *   KV sums      In every attention whose source is the 2D side (the 2D self-attention of layers
 *                1, 4, 7, 10; the 3D half of the cross layers 2, 5, 8, 11) KV = sum phi(k) v^T and
 *                sum phi(k) stop at c: the QKV epilogue writes phi(k) = v = 0 for rows >= c into
 *                its chunk sums, so a chunk past c is exactly +0 and both fold paths (kv_fold256;
 *                kv_reduce + m_fold) add it in its usual place without changing a bit.
 *   Source length  In those attentions v / Ns and Z * Ns take Ns = c (max(c, 1) as the divisor:
 *                with c = 0 every v is masked).
 *   InstanceNorm The norm of the 2D side's MLP (every self and cross layer) takes mean and
 *                variance over c tokens.  Rows >= c are stored like any other and are 0 in the
 *                sums; a 64-row tile, or a first-level group, without a valid row is left out of
 *                the merges (a merge with a zero count never happens); tiles and groups are merged
 *                in their fixed order.  c = 0: mean = rstd = 0.
 *   Dual softmax softmax(S, dim=1) -- the column statistics -- and the column winners run over
 *                rows < c.  The row side is per row.
 *   Untouched    The 3D side's own norms, the GAT layers, every per-row operation (the q
 *                projection, MLP conv 2, the final projection and its L2 norm, the score GEMM).
 *
 * Padding is harmless: for given maxima, no output bit of sample b depends on what input slots
 * past c hold (NaN and 1e30 included: the input stage writes zero rows there by a select), on
 * what the workspace held, or on the other samples' counts or data.  Rows past c are carried
 * through the per-row kernels as finite, deterministic values that no reduction reads.
 *
 * Outputs keep their padded shapes.  Past c, matches0 = -1, mscores0 = 0 and conf rows (when conf
 * is given) are written as 0; matches1 never names a row >= c.  For c = 0 every match is -1, every
 * score 0 and conf 0: the reference's empty-input result (GATs_SuperGlue.py:223-231) as values.
 *
 * The uniform entries are untouched: they launch the kernels they launched and give the bits
 * they gave.  With counts2d = NULL an entry here launches exactly those kernels; with every count
 * equal to n1 the counts instantiations mask nothing and sum the same terms in the same order:
 * either way the uniform entry's bits.
 *
 * Deterministic: the same bits from run to run and on any stream; no floating-point atomics.
 * ------------------------------------------------------------------------------------ */
#ifndef ONEPOSE_MATCH_COUNTS_H
#define ONEPOSE_MATCH_COUNTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int onepose_match_counts_version(void);

/* Workspace of the entries below: at least what onepose_match_workspace_bytes_ex returns for the
 * same arguments (0 for arguments that query refuses). */
size_t onepose_match_counts_workspace_bytes(int batch, int n1, int n3, int num_leaf, int with_conf,
                                            int precision);

/* onepose_match_cached_stages with per-sample 2D counts: the sibling's parameters, by the same
 * names, plus counts2d ([batch] int32 device array or NULL).  Refusals in the sibling's order,
 * with one more after its precision check: a precision other than ONEPOSE_PREC_FP32 is
 * ONEPOSE_ERR_UNSUPPORTED.  Stage ranges compose as the sibling's do, on the same workspace and
 * with the same counts2d in every call of a frame: INPUTS writes the zero rows, the layers and
 * SCORE..WINNERS read the counts again. */
int onepose_match_cached_counts_stages(const void* packed_weights, const void* desc2d,
                                       int desc_dtype, int64_t desc2d_bstride,
                                       const float* object_cache, const float* leaves_prepared,
                                       int64_t prepared_bstride, int batch, int n1, int n3,
                                       int num_leaf, float scale_factor, float match_threshold,
                                       int precision, int object_flags, const int* counts2d,
                                       int64_t* matches0, int64_t* matches1, float* mscores0,
                                       float* mscores1, float* conf, void* workspace,
                                       size_t workspace_bytes, int first_stage, int last_stage,
                                       void* stream);

/* The whole range ONEPOSE_STAGE_INPUTS .. ONEPOSE_STAGE_WINNERS of the call above. */
int onepose_match_cached_counts(const void* packed_weights, const void* desc2d, int desc_dtype,
                                int64_t desc2d_bstride, const float* object_cache,
                                const float* leaves_prepared, int64_t prepared_bstride, int batch,
                                int n1, int n3, int num_leaf, float scale_factor,
                                float match_threshold, int precision, int object_flags,
                                const int* counts2d, int64_t* matches0, int64_t* matches1,
                                float* mscores0, float* mscores1, float* conf, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* ONEPOSE_MATCH_COUNTS_H */
