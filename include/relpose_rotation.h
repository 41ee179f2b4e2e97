/*
 * relpose_rotation.h -- C ABI of librelpose_rotation.so (gfx950 / MI355X): the pure-rotation model behind the matches -- two-point
 * consensus and a three-parameter non-linear polish.
 *
 * With t = 0 every E = [t]x R fits the matches, for ANY t: the essential-matrix chains (relpose_consensus.h,
 * relpose_fivepoint.h) return a translation direction that means nothing, and the planar chain (relpose_homography.h) spends four rows
 * and eight degrees of freedom where two rows and three would do.  This twelfth, small library fits the model x2h ~ R x1h itself: two
 * rows make a minimal sample, all inliers then determine R well, and the inlier share of the best rotation says whether the pair
 * translates at all.
 *
 * CONVENTION.  Calibrated coordinates, x2h ~ R x1h (homogeneous x = (x, y, 1)); R is row-major [9]; quaternions are xyzw with w >= 0.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.  Nothing non-finite is written for finite inputs.
 */
#ifndef RELPOSE_ROTATION_H
#define RELPOSE_ROTATION_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_rotation_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_ROTATION_ABI_VERSION 1
#define RP_ROTATION_MAX_P 1728            /* 3 heads x 576 tokens */
#define RP_ROTATION_MAX_M 4096
#define RP_ROTATION_MAX_ITERS 64
int rp_rotation_abi_version(void);

/* DISTANCE of a row under R, used by both entry points: with m = R x1h (m_i = (R_i0 x + R_i1 y) + R_i2),
 * e = (m_x - u m_z, m_y - v m_z), x2 = (u, v),
 *      d = min((e_x^2 + e_y^2) / max(m_z^2, 1e-30), 1e30)   if m_z > 0,       d = 1e30   otherwise
 * -- the transfer distance of relpose_homography.h at H = R, expression for expression, with one difference: a rotation has a sign, so
 * a row that R sends behind the second camera (or onto its horizon) costs the maximum.  ROBUST COST of R:
 * c = sum_p w_p tau^2 log1p(d_p / tau^2) / sum_p w_p, weights clamped at 0 (a NaN counts as 0); INLIER SHARE:
 * sum w_p [d_p <= tau^2] / sum w_p -- both exactly those of relpose_homography.h. */

/* Rotation consensus: n independent problems of P correspondences, M hypotheses each; two launches on `stream`.
 *   x1, x2 [n][P][2], w [n][P] (NULL = ones; negative or NaN counts as 0), tau [n] (> 0, required), seed: exactly as for
 *   rp_homography_consensus.
 * ROWS.  pos is the ascending list of the rows of positive weight, K its length.
 * SAMPLER.  That of relpose_consensus.h with two draws: the same mix, the same s = mix(mix(seed + 0x9E3779B9 (i + 1)) ^ m) for problem i
 *   and hypothesis m; for k = 0, 1: r = mix(s + 0x9E3779B9 (k + 1)), j = K - 2 + k, t = (r (j + 1)) >> 32, c_k = j if t is among
 *   c_0 .. c_{k-1}, else t.  The sample is the rows pos[c_0], pos[c_1], in that order.
 * HYPOTHESIS m, per lane, fp32, no trigonometry.  Bearings a_k = unit(x1_k, 1), b_k = unit(x2_k, 1) (unit: the largest magnitude is
 *   divided out first, then the Euclidean norm).  Per image an orthonormal frame: e_1 = unit(a_0 + a_1), c = a_0 x a_1,
 *   e_2 = unit(unit(c) x e_1), e_3 = e_1 x e_2 (cross products as a_1 b_2 - a_2 b_1, ...; unit(c) is orthogonal to e_1 only to
 *   eps32 / |c|, so e_3 is taken again from e_1 and e_2: the frame is orthonormal to rounding whatever |c|); f_1, f_2, f_3 from b_0, b_1
 *   likewise.
 *   R_rc = (f_1r e_1c + f_2r e_2c) + f_3r e_3c: the least-squares rotation of the two pairs, which splits the mismatch of their two
 *   angles evenly.  Nothing tests beforehand whether the two angles agree: the cost decides.
 *   INVALID (hyp_R = 0, hyp_cost = FLT_MAX) if |a_0 x a_1| or |b_0 x b_1| is below 1e-6 (or not a number), on a non-finite entry of R,
 *   or on a non-finite cost.
 * SCORE.  hyp_cost[i][m] = the robust cost of hyp_R[i][m], summed over pos in ascending order.
 * SELECTION.  best[i] = the lowest index of the minimum hyp_cost among the valid hypotheses.
 * Outputs:
 *   R [n][9]          hyp_R[best], bit for bit
 *   best [n]          see above
 *   stat [n][4]       (hyp_cost[best], the inlier weight share at R, the number of valid hypotheses, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights w_p / (1 + d_p / tau^2) at R
 *   hyp_R [n][M][9], hyp_cost [n][M]   REQUIRED outputs, fully written; the second launch reads what the first wrote there
 *   samples [n][M][2] (NULL = off) the sampled row indices
 * A DEGENERATE problem -- K < 2, tau not > 0, or no valid hypothesis -- gives R = 0, best = -1, stat = (0, 0, number of valid
 * hypotheses, K), w_out = the clamped base weights; with K < 2 or tau not > 0 every hypothesis is invalid, and samples = 0 where K < 2.
 * LAYOUT.  hypothesis kernel: grid n ceil(M / 256), 256 threads, one lane per hypothesis, 42 496 B of LDS (the compacted rows), no
 * scratch.  Selection kernel: grid n, 256 threads, 2 176 B of LDS.
 * Argument checks before any launch: n <= 0, P < 2, M < 1, a required pointer NULL -> RP_EBADSHAPE; P > RP_ROTATION_MAX_P,
 * M > RP_ROTATION_MAX_M (or more than 2^31 - 1 workgroups, n ceil(M / 256)) -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other
 * pointer not 4-byte aligned -> RP_EALIGN. */
int rp_rotation_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed,
                          float* R, int* best, float* stat, float* w_out,
                          float* hyp_R, float* hyp_cost, int* samples, int P, int M, int n, void* stream);

/* Levenberg-Marquardt on the robust cost over the three degrees of freedom of R: one launch, one workgroup of 256 per problem.
 *   R0 [n][9]         the start, a near-rotation of any scale
 * STATE.  The unit quaternion q = rot_to_quat(R0 sqrt 3 / |R0|_F) (Shepperd's branches, normalised, w >= 0; |.|_F the Frobenius norm,
 *   fp32, no rescaling); R = quat_to_rot(q) wherever a matrix is needed.
 * Parameters, three: delta moves q to q' = unit((delta / 2, 1) (x) q), the sign fixed so that w >= 0; the product p (x) q in xyzw is
 *      x = ((p_w q_x + p_x q_w) + p_y q_z) - p_z q_y,   y = ((p_w q_y - p_x q_z) + p_y q_w) + p_z q_x,
 *      z = ((p_w q_z + p_x q_y) - p_y q_x) + p_z q_w,   w = ((p_w q_w - p_x q_x) - p_y q_y) - p_z q_z.
 * Residual of row p: with m = R x1h, r = ((m_x - u m_z) / m_z, (m_y - v m_z) / m_z); its Jacobian at delta = 0, exact, from
 *   dm_k = e_k x m: with p_x = m_x / m_z, p_y = m_y / m_z,
 *      J_0 = (-(p_x p_y), -(1 + p_y p_y)),   J_1 = (1 + p_x p_x, p_x p_y),   J_2 = (-p_y, p_x).
 *   A row with m_z <= 0 or m_z^2 < 1e-30 has no derivative: it enters the normal equations with weight 0 (and the cost with the
 *   clamped d).
 * One ITERATION at q with cost c and damping lambda:
 *   1. N = sum_p o_p J_p^T J_p (3 x 3), g = sum_p o_p J_p^T r_p with o_p = w_p / (1 + d_p / tau^2), the Cauchy weight at R: ONE fused
 *      reduction of 9 values, the 6 of the upper triangle row by row and the 3 of g.
 *   2. (N + lambda diag N) delta = -g in the diagonally scaled form of rp_refine_pose: d_i = 1 / sqrt(N_ii), the matrix d_i N_ij d_j off
 *      the diagonal and 1 + lambda on it factored by Cholesky.  A diagonal entry or a pivot that is not positive, a delta that is not
 *      finite, or a trial q' that has no direction is a BREAKDOWN.
 *   3. The trial q' and its cost c'.  ACCEPTED only if c' < c, strictly: then q and c are replaced and lambda <- max(lambda / 10, 1e-7).
 *      Otherwise, and after a breakdown, q is kept and lambda <- min(10 lambda, 1e7).
 * lambda starts at 1e-3.  Exactly `iters` iterations run, two barriers each; there is no early exit.  Each thread's rows (at most 7) stay
 * in registers; LDS holds the reduction buffer (288 B) and nothing else.
 * Outputs:
 *   R [n][9]          quat_to_rot(q) at the output; may alias R0
 *   pose [n][7]       (0, 0, 0, q): the pose format of the chains; t = 0 is what rp_triangulate documents as "nothing to triangulate"
 *   stat [n][4]       (c at the output, the inlier weight share at the output, the number of accepted steps, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights at the output
 * iters = 0 is the scorer: R = the normalised R0 (quat_to_rot(q)), c its cost.
 * A DEGENERATE problem -- K < 2, tau not > 0, R0 with a non-finite entry or a Frobenius norm below 1e-30 (the zero matrix that
 * rp_rotation_consensus writes for a degenerate problem) -- is not touched: R = R0 copied bit for bit, pose = 0, stat = (0, 0, 0, K),
 * w_out = the clamped base weights.
 * Argument checks before any launch: n <= 0, P < 2, iters < 0, x1 / x2 / tau / R0 / R / pose / stat NULL -> RP_EBADSHAPE;
 * P > RP_ROTATION_MAX_P, iters > RP_ROTATION_MAX_ITERS -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not
 * 4-byte aligned -> RP_EALIGN. */
int rp_rotation_refine(const float* x1, const float* x2, const float* w, const float* tau, const float* R0, int iters,
                       float* R, float* pose, float* stat, float* w_out, int P, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_ROTATION_H */
