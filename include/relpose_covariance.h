/*
 * relpose_covariance.h -- C ABI of librelpose_covariance.so (gfx950 / MI355X): the covariance of a two-view pose implied by the matches
 * it was fitted to -- how well the matches determine the pose, and which direction of it they determine worst.
 *
 * rp_refine_pose (relpose_refine.h) minimises the Cauchy-robust Sampson cost over the five degrees of freedom of (R, t) and returns a
 * cost; nothing says how far the minimiser moves when the noise is drawn again.  This fourteenth, small library evaluates, at a given
 * pose, the covariance of that M-estimator in its own five parameters: the SANDWICH A^-1 B A^-1 of the derivative of the estimating
 * equations (A) and the scatter of their terms (B).  It needs no noise scale: the residuals supply it.  The naive sigma^2 H^-1 (H the
 * Gauss-Newton matrix of the refinement) claims a standard deviation several times too small as soon as wrong matches are in the data
 * (DESIGN.md, 5.13).  The reference has no counterpart.
 *
 * The conventions of relpose_refine.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace, no randomness): results are bit-identical from call to call.
 */
#ifndef RELPOSE_COVARIANCE_H
#define RELPOSE_COVARIANCE_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_covariance_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_COVARIANCE_ABI_VERSION 1
#define RP_COVARIANCE_MAX_P 1728          /* 3 heads x 576 tokens */
int rp_covariance_abi_version(void);

/* Batched covariance of n poses against P correspondences each: one workgroup of 256 threads per problem, one pass over the rows, one
 * reduction.
 *   pose [n][7]       (t, q xyzw) as rp_refine_pose writes it -- normally its output
 *   x1, x2 [n][P][2]  normalised image coordinates in the convention of rp_refine_pose
 *   w [n][P]          base weights; NULL = all ones; a negative weight (or a NaN) counts as 0
 *   tau [n]           scale of the robust cost, > 0; required -- the tau the pose was refined with
 * The pose: t and q are normalised, each as v / |v| with the entry of largest magnitude m taken out first: u = v / m,
 * v / |v| = u / sqrt(sum u_i^2), |v| = m sqrt(sum u_i^2); every sum of this header is taken left to right unless parentheses say
 * otherwise.  The tangent basis (b1, b2) at t is the one of relpose_refine.h: e_k the unit vector of the smallest |t_k| (the lowest index
 * on ties), c = e_k x t, b1 = c / sqrt((c_0^2 + c_1^2) + c_2^2), b2 = t x b1.  The normalisation and the basis are evaluated WITHOUT
 * fused multiply-adds, so that `frame` can be restated bit for bit.
 * Residual s_p and its exact derivative J_p [5] with respect to (omega_0, omega_1, omega_2, beta_1, beta_2) -- all five are angles
 * in radians -- are those of relpose_refine.h, statement for statement (E = [t]x R, D_k, den, h_pk as there).
 * With w_p the clamped base weight, u_p = s_p^2 / tau^2 (s_p * s_p / (tau * tau)) and q_p = 1 + u_p:
 *      psi_p  = w_p s_p / q_p                  the influence of row p (w_p / q_p is the Cauchy weight of rp_refine_pose)
 *      psi'_p = w_p (1 - u_p) / (q_p q_p)      its derivative: NEGATIVE for a row beyond tau
 *      A = sum_p psi'_p J_p J_p^T              entry (i, j), j >= i: sum_p (psi'_p J_pi) J_pj
 *      B = sum_p psi_p^2 J_p J_p^T             entry (i, j), j >= i: sum_p ((psi_p psi_p) J_pi) J_pj
 *      C = A^-1 B A^-1                         the covariance of (omega, beta) -- in radians squared
 * Thread t sums its rows t, t + 256, .. in that order, the 64 lanes of a wave are summed by xor shuffles, the four waves as
 * ((w0 + w1) + w2) + w3 (csrc/block_sum.h); beside the 15 + 15 upper entries go four scalars: sum w_p, K = the number of rows with
 * w_p > 0, the number of rows with psi'_p < 0, and sum_p w_p tau^2 log1p(s_p^2 / tau^2).
 * C is formed in the diagonally scaled form, in thread 0, from the reduced sums:
 *   1. d_i = 1 / sqrt(A_ii).  An A_ii that is not positive (or not finite): status -1 with rho = 0.
 *   2. Ah_ij = A_ij d_i d_j off the diagonal, 1 on it; Bh_ij = B_ij d_i d_j (diagonal included).
 *   3. Cholesky Ah = L L^T, column by column: the PIVOT p_j = 1 - sum_{m<j} L_jm^2 (subtracted one by one), L_jj = sqrt(p_j),
 *      L_ij = (Ah_ij - sum_{m<j} L_im L_jm) / L_jj.  The first pivot that is not above 1e-6: status -1 with rho = that pivot.
 *      Otherwise rho = the smallest pivot, in (0, 1]: near 1 a well-determined pose, near 0 a direction the matches do not fix.
 *   4. The columns of M = Ah^-1: for c = 0..4, L y = e_c forward, L^T z = y backward (as lm_cholesky_solve of csrc/two_view.h), M_rc = z_r.
 *   5. T = M Bh (T_il = sum_k M_ik Bh_kl), Ch_ij = sum_l T_il M_jl for j >= i, C_ij = (d_i Ch_ij) d_j; C_ji = C_ij, copied.
 *      A C entry that is not finite: status -1 (rho as found).
 * The eigenvalues of C by cyclic Jacobi: RP_COVARIANCE_SWEEPS sweeps over the pairs (0,1), (0,2), .., (0,4), (1,2), .., (3,4), each
 * rotation: skipped if C_pq = 0; else theta = (C_qq - C_pp) / (2 C_pq), t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = 1),
 * c = 1 / sqrt(t^2 + 1), s = t c; C_pp -= t C_pq, C_qq += t C_pq, C_pq = 0, and for every other r (C_rp, C_rq) <- (c C_rp - s C_rq,
 * s C_rp + c C_rq), likewise the columns p, q of V (V = I at the start).
 * Outputs:
 *   cov [n][25]       C, row-major, exactly symmetric
 *   frame [n][6]      b1, b2: the 3 x 3 covariance of the unit t is [b1 b2] C_bb [b1 b2]^T with C_bb the lower right 2 x 2 block of C
 *   eig [n][5]        the eigenvalues of C, descending
 *   weak [n][5]       the unit eigenvector of eig[0] (the column of V under the largest diagonal entry, the lowest index on ties): the
 *                     direction of (omega, beta) in which the pose is LEAST determined; its component of largest magnitude is
 *                     positive (the lowest index on ties)
 *   stat [n][8]       (status, K, sd_rot = sqrt((C_00 + C_11) + C_22), sd_dir = sqrt(C_33 + C_44) -- the standard deviations of the
 *                     rotation and of the direction of t, in radians --, rho, the number of rows with psi' < 0, the robust cost
 *                     c = sum_p w_p tau^2 log1p(s_p^2 / tau^2) / sum_p w_p of rp_refine_pose's stat[1], 0)
 *   normal [n][30]    (NULL = off) the 15 upper entries of A row by row, then the 15 of B, as reduced
 * Status:
 *    1  ok.
 *    0  DEGENERATE: K < 6, |t| or |q| below 1e-30, a pose entry that is not finite, a tau that is not > 0 -- or a reduced sum that is
 *       not finite (a tau whose square leaves the range of fp32).  Every output element is 0, those of `normal` included.
 *   -1  NOT DETERMINED: the matches do not fix the pose at this tau -- so many rows lie beyond tau that A is not positive definite, or
 *       it is numerically singular (steps 1, 3, 5).  cov, eig, weak, sd_rot, sd_dir are 0; K, rho, the count of negative rows, c,
 *       frame and normal are written as above.
 * Nothing non-finite is written for finite inputs.
 * 6 <= P <= RP_COVARIANCE_MAX_P: a thread reads its (at most 7) rows once.
 * Argument checks before any launch: n <= 0, P < 6, pose / x1 / x2 / tau / cov / frame / eig / weak / stat NULL -> RP_EBADSHAPE;
 * P > RP_COVARIANCE_MAX_P -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not 4-byte aligned -> RP_EALIGN. */
#define RP_COVARIANCE_SWEEPS 6
int rp_pose_covariance(const float* pose, const float* x1, const float* x2, const float* w, const float* tau,
                       float* cov, float* frame, float* eig, float* weak, float* stat, float* normal,
                       int P, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_COVARIANCE_H */
