/* Two-view geometric verification of libonepose_hip -- included by onepose_hip.h.
 *
 * The declarations of this family live in a header of their own: onepose_hip.h's own
 * declarations are the 99 functions of ABI 9 (the table tests/test_binding.py pins), and
 * onepose_abi_version() is not bumped.  The Python binding parses this file into
 * _lib.FAMILY_SIGNATURES and calls its functions by parameter name like every other.
 *
 * ------------------------------------------------------------------------------------ *
 * Two-view verification  --  batched fundamental-matrix RANSAC
 *   The step between import_matches and point_triangulator that the reference leaves to
 *   COLMAP's matches_importer (src/sfm/triangulation.py:18-35): per image pair a two-view
 *   geometry is estimated from the pair's matches and only its inliers are kept.
 * Versioned on its own: onepose_twoview_version() returns 1.
 *
 * No COLMAP source or binary is at hand.  COLMAP's verifier runs LO-RANSAC over E, F and H
 * models; what is stated below is this project's own: parity with COLMAP's matches_importer
 * is NOT verified and is not claimed.  The defaults the Python layer passes (max_error 4 px,
 * confidence 0.999, max_num_trials 10000, min_num_inliers 15, min_inlier_ratio 0.25) carry the
 * names and values of COLMAP's documented options.  Not here: E and H models, LO-RANSAC,
 * cheirality tests, writing two-view geometries to a database.  tests/two_view_oracle.py
 * restates the entry point in plain loops.
 *
 * All pointers are device pointers.  The entry point allocates, frees and synchronises nothing,
 * makes one launch (one workgroup of 256 threads per pair, the pair's points in LDS) whatever
 * the data, and can be captured in a graph.  No floating-point atomics; every floating-point
 * step is the fp64 operation written here, a*b + c is never fused, every sum is taken in the
 * order stated: results are bit-identical from run to run.  Only + - * / sqrt and comparisons
 * touch the model, so a plain-loop restatement in IEEE double reproduces it.
 *
 * onepose_two_view_verify
 *   pts0, pts1 [batch, max_points, 2] fp32, pixels in COLMAP's convention (keypoint + 0.5); match i
 *   of pair b joins pts0[b, i] and pts1[b, i].  counts [batch] int32, clamped to [0, max_points].
 *   Outputs: F [batch, 9] fp64 row-major with x1^T F x0 = 0 (zeros without a model); inlier_mask
 *   [batch, max_points] uint8, zero past the count; n_inliers, iters, status [batch] int32.
 *   Host refusals (ONEPOSE_ERR_INVALID, nothing launched, no output written): a null pointer
 *   other than F_in, batch < 1, max_points < 1 or above onepose_two_view_max_points(),
 *   min_num_inliers < 8, max_trials < 1, refine_iters < 0, max_error negative or NaN, confidence
 *   not in (0, 1), min_inlier_ratio NaN.  A workspace smaller than
 *   onepose_two_view_workspace_bytes(): ONEPOSE_ERR_WORKSPACE (the kernel keeps its state in LDS;
 *   the workspace is reserved and not written).
 *
 *   With n = the pair's clamped count:
 *   status 1: n < min_num_inliers.  Nothing is run: mask and n_inliers zero, iters 0, F zeros
 *     (F_in's copy in the given-geometry mode).
 *   status 2: RANSAC found no model (no hypothesis with at least 8 inliers): zeros.
 *   status 3: a model, but n_inliers < min_num_inliers or (double)n_inliers < min_inlier_ratio *
 *     (double)n.  F, the mask and n_inliers are reported as for status 0; the caller drops the pair.
 *   status 0: verified.
 *
 *   Error of a match under F (squared Sampson distance), x0 = pts0, x1 = pts1 widened to double:
 *     a0 = (F0 x0 + F1 y0) + F2,  a1 = (F3 x0 + F4 y0) + F5,  a2 = (F6 x0 + F7 y0) + F8,
 *     b0 = (F0 x1 + F3 y1) + F6,  b1 = (F1 x1 + F4 y1) + F7,
 *     e = (x1 a0 + y1 a1) + a2,   err = (e e) / (((a0 a0 + a1 a1) + b0 b0) + b1 b1).
 *   A match is an inlier iff err <= max_error * max_error (a NaN err is not).  A model with a
 *   non-finite entry has no inliers.
 *
 *   Solver S(list): the normalised 8-point algorithm over an ordered list of m >= 8 matches.
 *     1 Per side: c = (sum x / m, sum y / m); d = sum sqrt(dx dx + dy dy) / m with dx = x - cx,
 *       dy = y - cy; s = 1.4142135623730951 / d; u = dx s, v = dy s.  Every sum starts at 0 and
 *       runs over the list in order as t = t + term; m is converted to double.
 *     2 a = (u1 u0, u1 v0, u1, v1 u0, v1 v0, v1, u0, v0, 1); M[i][j] = sum a_i a_j for i <= j, 45
 *       serial sums in list order, M symmetric.
 *     3 f = the eigenvector of M's smallest eigenvalue by the cyclic Jacobi J(9) below; N = f as
 *       3 x 3, row-major.
 *     4 Rank 2: G[i][j] = (N[0][i] N[0][j] + N[1][i] N[1][j]) + N[2][i] N[2][j]; v = J(3)'s
 *       eigenvector of G's smallest eigenvalue; w_i = (N[i][0] v0 + N[i][1] v1) + N[i][2] v2;
 *       N[i][j] = N[i][j] - w_i v_j.  (N loses its smallest singular value.)
 *     5 Denormalise, F = T1^T N T0: A[i][0] = N[i][0] s0, A[i][1] = N[i][1] s0, A[i][2] =
 *       (N[i][2] - A[i][0] cx0) - A[i][1] cy0; F[0][j] = s1 A[0][j], F[1][j] = s1 A[1][j],
 *       F[2][j] = (A[2][j] - cx1 F[0][j]) - cy1 F[1][j].
 *   J(k), on a symmetric k x k matrix A with V = I: at most 24 sweeps over (p, q), p < q, row by
 *     row.  A pair with |A_pq| <= 1e-20 sqrt(|A_pp A_qq|) or A_pq == 0 has A_pq set to 0 and is
 *     skipped.  Otherwise theta = (A_qq - A_pp) / (2 A_pq), t = (theta >= 0 ? 1 : -1) / (|theta| +
 *     sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c; for every r other than p, q:
 *     (A_rp, A_rq) = (c A_rp - s A_rq, s A_rp + c A_rq), mirrored; with bpp = c A_pp - s A_pq,
 *     bpq = s A_pp + c A_pq, bqp = c A_pq - s A_qq, bqq = s A_pq + c A_qq: A_pp = c bpp - s bqp,
 *     A_qq = s bpq + c bqq, A_pq = 0; for every r: (V_rp, V_rq) = (c V_rp - s V_rq, s V_rp + c
 *     V_rq).  A sweep without a rotation ends the iteration (non-finite input ends at 24 sweeps).
 *     The result is column j of V for the smallest A_jj, the first of equals.
 *
 *   F_in == NULL: estimate.  OpenCV 4.4's RANSACPointSetRegistrator loop on the scaffold of
 *     csrc/ransac.h, as the pose and affine kernels run it: cv::RNG((uint64)-1); per iteration a
 *     subset of 8 indices, each draw % n, a draw equal to an index already in the subset is drawn
 *     again; the hypothesis S(subset in draw order); its inlier count over all n matches;
 *     count > max(best, 7) makes it the best and niters = RANSACUpdateNumIters(confidence,
 *     (n - count) / n, 8, niters), starting from niters = max_trials.  64 iterations are evaluated
 *     per round and accepted in iteration order; those at or past niters are discarded, so model,
 *     mask and iters (the iterations run) are the sequential loop's.
 *     Then refine_iters refits: F' = S(the current inliers in ascending match order); its mask
 *     over all matches; F' and its mask replace the current ones iff F' is finite and its inlier
 *     count is not smaller.  The first refit that is not kept ends the refits.
 *   F_in != NULL, [batch, 9] fp64: given geometry.  No RANSAC: F is a copy of F_in, the mask is the
 *     same Sampson test against it, iters = 0, status 1, 3 or 0 by the rules above.
 *
 *   Mapping: lane h of wave 0 solves hypothesis h, its M and V in LDS at [entry][lane] (no
 *   per-thread array is indexed at run time); wave w counts the inliers of hypotheses w, w + 4,
 *   ...; in a refit 4, 2 and 45 lanes each take one of the serial sums.  17 bytes of LDS per match
 *   beside the fixed state: onepose_two_view_max_points() is what fits 160 KB (>= 4096).
 * ------------------------------------------------------------------------------------ */
#ifndef ONEPOSE_TWO_VIEW_H
#define ONEPOSE_TWO_VIEW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int onepose_twoview_version(void);
int onepose_two_view_max_points(void);
size_t onepose_two_view_workspace_bytes(int batch, int max_points);
int onepose_two_view_verify(const float* pts0, const float* pts1, const int* counts,
                            int max_points, int batch, const double* F_in, double max_error,
                            double confidence, int max_trials, int min_num_inliers,
                            double min_inlier_ratio, int refine_iters, double* F,
                            uint8_t* inlier_mask, int* n_inliers, int* iters, int* status,
                            void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
