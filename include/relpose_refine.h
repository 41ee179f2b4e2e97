/*
 * relpose_refine.h -- C ABI of librelpose_refine.so (gfx950 / MI355X): non-linear refinement of a two-view pose on the essential
 * manifold, and the robust score of a pose against matches.
 *
 * rp_eight_point (relpose_eightpoint.h) minimises an algebraic error in nine unconstrained numbers and then projects onto the
 * essential manifold; rp_pose_from_essential (relpose_hip.h) decodes that projection.  This fourth, small library is the step every
 * classical two-view pipeline puts behind them: Levenberg-Marquardt on the geometric (Sampson) error over the five degrees of freedom
 * of (R, t), with the Cauchy weight the eight-point solver already uses.  With zero iterations the same entry point SCORES any pose --
 * the regressed one or the classical one -- against the matches on one scale.  The reference has no counterpart.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace, no randomness): results are bit-identical from call to call.
 */
#ifndef RELPOSE_REFINE_H
#define RELPOSE_REFINE_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_refine_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_REFINE_ABI_VERSION 1
#define RP_REFINE_MAX_P 1728              /* 3 heads x 576 tokens */
#define RP_REFINE_MAX_ITERS 32
int rp_refine_abi_version(void);

/* Batched refinement of n poses against P correspondences each: one workgroup per problem, the whole iteration in one launch.
 *   pose0 [n][7]      the start, (t, q xyzw) as rp_pose_from_essential writes it; t and q are normalised internally
 *   x1, x2 [n][P][2]  normalised image coordinates in the convention of rp_eight_point: X2 = R X1 + t, E = [t]x R, x2^T E x1 = 0
 *                     (homogeneous x = (x, y, 1))
 *   w [n][P]          base weights; NULL = all ones; a negative weight (or a NaN) counts as 0
 *   tau [n]           scale of the robust cost, in units of the square root of the Sampson distance, > 0; required
 * Residual of row p at the pose (R, t), with E = [t]x R, l2 = E x1, l1 = E^T x2, den = l2_x^2 + l2_y^2 + l1_x^2 + l1_y^2:
 *      s_p = x2^T E x1 / sqrt(den)      (the signed root of the Sampson distance; s_p = 0 where den is 0, and so is its derivative)
 * Cost:
 *      c = sum_p w_p tau^2 log1p(s_p^2 / tau^2) / sum_p w_p
 * -- the cost whose IRLS weight is the Cauchy weight w_p / (1 + s_p^2 / tau^2) of rp_eight_point.
 * Parameters, five: delta = (omega_0, omega_1, omega_2, beta_1, beta_2) moves the pose to
 *      R <- R exp([omega]x),  carried as q <- normalise(q (x) (omega sin(theta / 2) / theta, cos(theta / 2))), theta = |omega| (Hamilton
 *                             product, xyzw; sin(theta / 2) / theta = 1/2 - theta^2 / 48 for theta < 1e-4)
 *      t <- normalise(t + b1 beta_1 + b2 beta_2),  (b1, b2) the orthonormal basis of the tangent plane at t given by: e_k the unit
 *                             vector of the smallest |t_k| (the lowest index on ties), b1 = normalise(e_k x t), b2 = t x b1.
 * One ITERATION at the pose (R, t) with cost c and damping lambda:
 *   1. J_p [5] = d s_p / d delta at delta = 0, exact: with D_k = dE / d delta_k (D_k = E [e_k]x for k < 3, [b_1]x R, [b_2]x R),
 *      J_pk = (x2^T D_k x1 - s_p h_pk / sqrt(den)) / sqrt(den),  h_pk = l2_x (D_k x1)_x + l2_y (D_k x1)_y + l1_x (D_k^T x2)_x + l1_y (D_k^T x2)_y.
 *   2. H = sum_p o_p J_p J_p^T, g = sum_p o_p J_p s_p with o_p = w_p / (1 + s_p^2 / tau^2), the Cauchy weight at the pose.
 *   3. (H + lambda diag H) delta = -g, solved in the diagonally scaled form: with d_i = 1 / sqrt(H_ii), the matrix of the entries
 *      d_i H_ij d_j off the diagonal and 1 + lambda on it is factored by Cholesky, delta_i = -d_i z_i with z its solution for the
 *      right-hand side d_i g_i.  A diagonal entry of H or a pivot that is not positive, or a delta that is not finite, is a BREAKDOWN.
 *   4. The trial pose (above) and its cost c'.  The step is ACCEPTED only if c' < c, strictly: then the pose and c are replaced and
 *      lambda <- max(lambda / 10, 1e-7).  Otherwise, and after a breakdown, the pose is kept and lambda <- min(10 lambda, 1e7).
 * lambda starts at 1e-3.  Exactly `iters` iterations run, there is no early exit: a converged problem rejects its steps or takes null ones.
 * Outputs:
 *   pose [n][7]       (t unit, q xyzw unit with w >= 0); may alias pose0
 *   E [n][9]          [t]x R of the output pose, row-major, NOT sign-normalised (Frobenius norm sqrt 2)
 *   stat [n][4]       (c0 the cost at the start, c the cost at the output pose, the number of accepted steps, the 2-norm of the last
 *                     accepted delta or 0); c <= c0 always
 *   w_out [n][P]      (NULL = off) the Cauchy weights o_p at the output pose
 * iters = 0 is the scorer: pose = the normalised pose0, c = c0, w_out = the weights at pose0.
 * A DEGENERATE problem -- fewer than 5 rows of positive weight, |t0| or |q0| below 1e-30, or a tau that is not > 0 -- is not touched:
 * pose = pose0 copied bit for bit, E = 0, stat = 0, w_out = the clamped base weights.  E = 0 is the flag.  Nothing non-finite is
 * written for finite inputs.
 * P <= RP_REFINE_MAX_P: a thread keeps its (at most 7) rows in registers for the whole launch.
 * Argument checks before any launch: n <= 0, P < 5, iters < 0, pose0 / x1 / x2 / tau / pose / E / stat NULL -> RP_EBADSHAPE;
 * P > RP_REFINE_MAX_P, iters > RP_REFINE_MAX_ITERS -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not 4-byte
 * aligned -> RP_EALIGN. */
int rp_refine_pose(const float* pose0, const float* x1, const float* x2, const float* w, const float* tau,
                   float* pose, float* E, float* stat, float* w_out, int P, int iters, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_REFINE_H */
