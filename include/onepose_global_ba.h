/* Global bundle adjustment of libonepose_hip -- included by onepose_hip.h.
 *
 * The declarations of this family live in a header of their own, as those of
 * onepose_superglue_counts.h do: neither onepose_abi_version() (9) nor onepose_ba_version() (1)
 * is bumped, nothing that existed changed.  The Python binding parses this file into
 * _lib.FAMILIES["onepose_global_ba.h"] and calls its functions by parameter name.
 * Versioned on its own: onepose_gba_version() returns 1.
 *
 * ------------------------------------------------------------------------------------ *
 * Global bundle adjustment of an SfM model, fp64: Levenberg-Marquardt with preconditioned
 * conjugate gradients on the implicit Schur complement.
 *   The reference's last SfM stage (src/sfm/global_ba.py) shells out to COLMAP's bundle_adjuster
 *   with extrinsics refined and intrinsics fixed.  This family is the project's own solver for
 *   that problem; parity with COLMAP or Ceres is NOT claimed (COLMAP parametrises rotations by
 *   quaternions and picks its linear solver by model size).  No robust loss, no refinement of
 *   intrinsics.  The arithmetic below is restated in numpy float64 by tests/gba_oracle.py.
 *
 * Cost.  residual[n] = (fx x / z + cx - u, fy y / z + cy - v) with (x, y, z) = R(aa) X + t,
 * X = points[ptIdx[n]], (aa, t) = cam_pose[camIdx[n]], (fx, fy, cx, cy) = cam_K4[camIdx[n]],
 * (u, v) = obs_xy[n]; cost = 1/2 sum |residual|^2.  The rotation, its two branches (theta^2 > 0:
 * Rodrigues, else X + aa x X), the Jacobian and its series below theta^2 = 1e-4 are those of the
 * tracker family (onepose_hip.h, "Tracker back end"), operation by operation; the only change
 * is that row 0 of d r / d p carries fx and row 1 carries fy.
 *
 * Fixed parameters.  cam_fixed [n_cams] uint8 or NULL (nothing fixed): bit j set means pose
 * parameter j (aa0, aa1, aa2, t0, t1, t2) of that camera is constant.  At linearisation the
 * columns of Jc of fixed parameters are set to zero; after damping, the diagonal of U at those
 * parameters is set to 1.  Their rows and columns of the system are then those of the identity
 * with a zero right-hand side: their step is exactly 0, and the candidate keeps their bits.
 *
 * Index.  That of onepose_ba_build_index (onepose_hip.h), unchanged; the builder has no camera
 * limit.  onepose_gba_begin checks it on the device exactly as onepose_ba_solve does, before
 * anything is read through it: a malformed index gives status 2 and moves nothing.
 *
 * Levenberg-Marquardt, the tracker family's rules.  Per outer iteration, at the iterate:
 *   V_p = sum Jp^T Jp and g_p = sum Jp^T r over the point's observations in index order;
 *   U_c = sum Jc^T Jc and g_c = sum Jc^T r over the camera's observations;
 *   damping mu * clamp(diag, 1e-6, 1e32), mu = 1 / radius, is added to diag V and diag U;
 *   V_p = L L^T (3 x 3 Cholesky, column by column), z_p = L^-1 g_p; V^-1 is never formed;
 *   W_n = Jc^T Jp, Y_n = L^-1 W_n^T;
 *   M_c = U_c - sum_{n of c} Y_n^T Y_n (the 6 x 6 diagonal block of S), M_c = C C^T;
 *   rhs_c = -g_c + sum_{n of c} Y_n^T z_p.
 *   A 3 x 3 or 6 x 6 pivot that is not > 0 rejects the iteration (as a failed Cholesky of the
 *   tracker family does): radius /= factor, factor *= 2, the row's candidate cost, model
 *   decrease and rho are NaN.
 * Linear solve: S dc = rhs with S x = U x - sum_p W_p V_p^-1 W_p^T x never formed.  S x in two
 * passes: per point, y_p = L^-T L^-1 sum_n Jp_n^T (Jc_n x_cam(n)) over the point's observations
 * in index order; per camera, (S x)_c = U_c x_c - sum_n Jc_n^T (Jp_n y_pt(n)).  Preconditioned
 * CG with the preconditioner M = diag(M_c) applied through the factors C (Ceres' SCHUR_JACOBI):
 *   x = 0, res = rhs, z = M^-1 res, p = z, rz_0 = rz = res . z;
 *   rz_0 non-finite: stop, reason 4; rz_0 == 0: stop, reason 5 (x = 0);
 *   step k = 1, 2, ...: pSp = p . S p; if pSp is not finite: stop, reason 4; if pSp <= 0: stop,
 *   reason 3; alpha = rz / pSp, x += alpha p, res -= alpha S p, z = M^-1 res, rz' = res . z,
 *   beta = rz' / rz, p = z + beta p, rz = rz'; then stop if alpha, rz' or beta is not finite
 *   (reason 4), if sqrt(rz / rz_0) <= pcg_tol (reason 1), if k == pcg_max_iters (reason 2).
 *   Whatever the reason, dc = the current x and the LM test below decides on it.
 * dp = L^-T L^-1 (-g_p - sum_n Jp_n^T (Jc_n dc_cam(n))); candidate = iterate + (dc, dp);
 * md = -(J d) . (r + J d / 2); rho = (cost - cost') / md; accepted iff cost' is finite, md > 0
 * and rho > 1e-3.  Accepted: radius = min(radius / max(1/3, 1 - (2 rho - 1)^3), 1e16), factor =
 * 2.  Rejected: radius /= factor, factor *= 2; the next iteration reuses the linearisation.
 * Stop rules, tested after the radius update: an accepted step with function_tolerance > 0 and
 * |cost - cost'| / cost <= function_tolerance sets status 3 (Ceres' rule; the step stays
 * accepted); otherwise a radius below 1e-32 sets status 4 (Ceres' minimum radius; with both
 * tolerances 0 a converged solve runs on, rejecting, until this stops it).
 *
 * Order of every sum (no floating-point atomics anywhere; results are bit-identical from run to
 * run, on any stream, in a graph replay and under any split of the steps over calls):
 *   per point: one thread walks the point's CSR range in order;
 *   per camera: one wave; lane l adds the camera's CSR slots l, l + 64, ... in order, then a
 *   64-lane xor butterfly (offsets 32, 16, ..., 1);
 *   over observations (cost, md) and over cameras (the CG dot products, each camera's
 *   6-element dot product first, j = 0..5): thread t of one workgroup of 256 adds elements
 *   t, t + 256, ... in order, then a halving tree over the 256 partial sums.
 *
 * Entry points.  points [n_points, 3] and cam_pose [n_cams, 6] fp64, both in / out; cam_K4
 * [n_cams, 4] fp64; obs_xy [n_obs, 2] fp64; ptIdx, camIdx [n_obs] int64; cam_fixed [n_cams]
 * uint8 or NULL; index: the uploaded bytes of onepose_ba_build_index.  All device pointers.
 * Limits: 1 <= n_obs <= 2^20, 1 <= n_cams, n_points <= 2^20, active cameras <=
 * onepose_gba_max_cameras() (4096), n_steps in 1..1024, pcg_max_iters in 1..500, info_rows in
 * 0..65536.  onepose_gba_workspace_bytes returns 0 for a refused shape.
 *
 * onepose_gba_linearize: the first stage alone on the caller's arrays (no index): residuals
 * [n_obs, 2], Jc [n_obs, 2, 6] (fixed columns zeroed), Jp [n_obs, 2, 3], cost [1].  An
 * observation whose ids are out of range gets NaN rows (and the cost is NaN); nothing is read
 * through them.
 *
 * onepose_gba_begin validates the index, gathers the active variables, computes the initial
 * cost and writes the solver state (radius = initial_radius, factor = 2, cost, counters) into
 * the workspace; info is zeroed and its head written.  onepose_gba_step runs n_steps more outer
 * iterations from that state, with the same arrays, shapes, info and workspace as the begin
 * call (a workspace that holds no state of these shapes makes every launch a no-op).  The
 * launch sequence is fixed for given shapes, n_steps and pcg_max_iters; accept / reject, the CG
 * stop and termination are decided on the device, and after a stop the remaining launches do
 * nothing.  Neither call allocates, frees or synchronises: both can be captured in a graph.
 * On acceptance the caller's arrays receive the iterate: on return they hold the last accepted
 * one.  Cameras and points without observations are never written.
 *
 * info [8 + 8 * info_rows] fp64, device.  Head: [0] status (0 ran, 1 non-finite initial cost,
 * 2 bad index, 3 converged by function_tolerance, 4 radius below 1e-32), [1] iterations,
 * [2] accepted iterations, [3] initial cost, [4] final cost, [5] final radius, [6] total CG
 * iterations, [7] 0.  Then one row of 8 per outer iteration: cost, candidate cost, model
 * decrease, rho, the radius used, accepted, CG iterations, CG end reason (1 tolerance, 2 cap,
 * 3 p.Sp <= 0, 4 non-finite, 5 zero right-hand side; 0 when a factorisation failed).
 * Iterations past info_rows still run and are counted in the head.
 *
 * Checks, in this order, before anything is launched: null pointers (cam_fixed may be NULL);
 * shapes (sizes, active counts within 1..n and <= n_obs); active cameras over the limit;
 * info_rows; begin: initial_radius positive and finite; step: n_steps, pcg_max_iters, pcg_tol
 * and function_tolerance finite and >= 0 -- all ONEPOSE_ERR_INVALID -- then the workspace size
 * (ONEPOSE_ERR_WORKSPACE).
 * ------------------------------------------------------------------------------------ */
#ifndef ONEPOSE_GLOBAL_BA_H
#define ONEPOSE_GLOBAL_BA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int onepose_gba_version(void);
int onepose_gba_max_cameras(void);
size_t onepose_gba_workspace_bytes(int64_t n_obs, int n_active_cams, int n_active_points);
int onepose_gba_linearize(const double* points, const double* cam_pose, const double* cam_K4,
                          const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                          const uint8_t* cam_fixed, int64_t n_obs, int n_cams, int n_points,
                          double* residuals, double* Jc, double* Jp, double* cost, void* stream);
int onepose_gba_begin(double* points, double* cam_pose, const double* cam_K4,
                      const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                      const uint8_t* cam_fixed, const void* index, int64_t n_obs, int n_cams,
                      int n_points, int n_active_cams, int n_active_points,
                      double initial_radius, double* info, int info_rows, void* workspace,
                      size_t workspace_bytes, void* stream);
int onepose_gba_step(double* points, double* cam_pose, const double* cam_K4,
                     const double* obs_xy, const int64_t* ptIdx, const int64_t* camIdx,
                     const uint8_t* cam_fixed, const void* index, int64_t n_obs, int n_cams,
                     int n_points, int n_active_cams, int n_active_points, int n_steps,
                     int pcg_max_iters, double pcg_tol, double function_tolerance, double* info,
                     int info_rows, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif  /* ONEPOSE_GLOBAL_BA_H */
