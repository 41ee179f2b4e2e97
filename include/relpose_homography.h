/*
 * relpose_homography.h -- C ABI of librelpose_homography.so (gfx950 / MI355X): the plane-induced homography behind the matches --
 * consensus, non-linear polish, and the closed-form decomposition into at most two physically possible (R, t, n).
 *
 * Two essential matrices fit the matches of ONE plane, and the Sampson score cannot tell them apart: every chain
 * built on rp_eight_point_consensus (relpose_consensus.h) or rp_five_point_consensus (relpose_fivepoint.h) fails on a wall, a floor or
 * a facade that fills both views.  This eighth, small library is the classical answer: four rows make a minimal sample of the
 * homography H, all inliers then determine H well, and H decomposes in closed form.
 *
 * CONVENTION.  Calibrated coordinates, X2 = R X1 + t as in rp_eight_point; the points of the plane satisfy n^T X1 = d (n unit, d > 0),
 * so x2h ~ H x1h with H ~ R + t n^T / d (homogeneous x = (x, y, 1)); H is row-major [9], rows h1, h2, h3.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.  Nothing non-finite is written for finite inputs.
 */
#ifndef RELPOSE_HOMOGRAPHY_H
#define RELPOSE_HOMOGRAPHY_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_homography_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_HOMOGRAPHY_ABI_VERSION 1
#define RP_HOMOGRAPHY_MAX_P 1728          /* 3 heads x 576 tokens */
#define RP_HOMOGRAPHY_MAX_M 4096
#define RP_HOMOGRAPHY_MAX_ITERS 64
int rp_homography_abi_version(void);

/* TRANSFER DISTANCE of a row under H, used by all three entry points: with m = H x1h, e = (m_x - u m_z, m_y - v m_z), x2 = (u, v),
 *      d = min((e_x^2 + e_y^2) / max(m_z^2, 1e-30), 1e30)
 * -- the squared one-sided distance |pi(H x1h) - x2|^2, independent of the sign of H.  A row mapped to infinity costs a finite maximum;
 * it is never scored 0.  ROBUST COST of H: c = sum_p w_p tau^2 log1p(d_p / tau^2) / sum_p w_p, weights clamped at 0 (a NaN counts as 0).
 * NORMALISATION of H: division by the Frobenius norm sqrt(sum h_i^2) (fp32, no rescaling: a norm below 1e-30 or not finite is a
 * breakdown); SIGN RULE of rp_eight_point: the entry of largest magnitude, the first of equal ones, is positive. */

/* Homography consensus: n independent problems of P correspondences, M hypotheses each; two launches on `stream`.
 *   x1, x2 [n][P][2], w [n][P] (NULL = ones; negative or NaN counts as 0), tau [n] (> 0, required), seed: exactly as for
 *   rp_eight_point_consensus.
 * ROWS.  pos is the ascending list of the rows of positive weight, K its length.
 * SAMPLER.  That of relpose_consensus.h with four draws: the same mix, the same s = mix(mix(seed + 0x9E3779B9 (i + 1)) ^ m) for problem i
 *   and hypothesis m; for k = 0 .. 3: r = mix(s + 0x9E3779B9 (k + 1)), j = K - 4 + k, t = (r (j + 1)) >> 32, c_k = j if t is among
 *   c_0 .. c_{k-1}, else t.  The sample is the rows pos[c_0] .. pos[c_3], in that order.
 * HYPOTHESIS m.  Hartley normalisation per image about the first sampled row (centroid c = p_0 + sum (p_k - p_0) / 4, scale
 *   s = sqrt 2 / mean |p_k - c|; a mean below 1e-30 is a breakdown); sampled row k gives the rows 2k, 2k + 1 of the 8 x 9 matrix,
 *   (x, y, 1, 0, 0, 0, -u x, -u y, -u) and (0, 0, 0, x, y, 1, -v x, -v y, -v) in normalised coordinates; its null vector by eight
 *   Householder reflections of the transpose applied to e_9, never the normal matrix (a zero column gets beta = 0);
 *   H = T2^-1 H^ T1; normalisation and sign rule as above.  INVALID (hyp_H = 0, hyp_cost = FLT_MAX) on a breakdown, a non-finite entry
 *   or a non-finite cost.  Three collinear rows do not break down: they give a rank-deficient H whose cost is high.
 * SCORE.  hyp_cost[i][m] = the robust cost of hyp_H[i][m], summed over pos in ascending order.
 * SELECTION.  best[i] = the lowest index of the minimum hyp_cost among the valid hypotheses.
 * Outputs:
 *   H [n][9]          hyp_H[best], bit for bit
 *   best [n]          see above
 *   stat [n][4]       (hyp_cost[best], the inlier weight share sum w_p [d_p <= tau^2] / sum w_p at H, the number of valid hypotheses, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights w_p / (1 + d_p / tau^2) at H
 *   hyp_H [n][M][9], hyp_cost [n][M]   REQUIRED outputs, fully written; the second launch reads what the first wrote there
 *   samples [n][M][4] (NULL = off) the sampled row indices
 * A DEGENERATE problem -- K < 4, tau not > 0, or no valid hypothesis -- gives H = 0, best = -1, stat = (0, 0, number of valid
 * hypotheses, K), w_out = the clamped base weights; with K < 4 or tau not > 0 every hypothesis is invalid, and samples = 0 where K < 4.
 * LAYOUT.  hypothesis kernel: grid n ceil(M / 256), 256 threads, one lane per hypothesis, 42 496 B of LDS (the compacted rows), no
 * scratch.  Selection kernel: grid n, 256 threads, 2 176 B of LDS.
 * Argument checks before any launch: n <= 0, P < 4, M < 1, a required pointer NULL -> RP_EBADSHAPE; P > RP_HOMOGRAPHY_MAX_P,
 * M > RP_HOMOGRAPHY_MAX_M (or more than 2^31 - 1 workgroups, n ceil(M / 256)) -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other
 * pointer not 4-byte aligned -> RP_EALIGN. */
int rp_homography_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed,
                            float* H, int* best, float* stat, float* w_out,
                            float* hyp_H, float* hyp_cost, int* samples, int P, int M, int n, void* stream);

/* Levenberg-Marquardt on the robust cost over the eight degrees of freedom of H: one launch, one workgroup of 256 per problem.
 *   H0 [n][9]         the start, any scale and sign; normalised internally
 * Parameters, eight: delta moves H to normalise(H (I + D)), D = sum_k delta_k G_k with the generators of sl(3) in the order
 *   E_01, E_02, E_10, E_12, E_20, E_21 (E_ij the unit matrix of row i, column j), diag(1, -1, 0), diag(0, 1, -1):
 *      D = [[delta_6, delta_0, delta_1], [delta_2, delta_7 - delta_6, delta_3], [delta_4, delta_5, -delta_7]].
 * Residual of row p: with m = H x1h, r = ((m_x - u m_z) / m_z, (m_y - v m_z) / m_z); its Jacobian at delta = 0, exact: for the generator
 *   E_ij, dm = x1h_j (column i of H), J_k = ((dm_x - (m_x / m_z) dm_z) / m_z, (dm_y - (m_y / m_z) dm_z) / m_z).  A row with
 *   m_z^2 < 1e-30 has no derivative: it enters the normal equations with weight 0 (and the cost with the clamped d).
 * One ITERATION at H with cost c and damping lambda:
 *   1. N = sum_p o_p J_p^T J_p (8 x 8), g = sum_p o_p J_p^T r_p with o_p = w_p / (1 + d_p / tau^2), the Cauchy weight at H: ONE fused
 *      reduction of 44 values, the 36 of the upper triangle row by row and the 8 of g.
 *   2. (N + lambda diag N) delta = -g in the diagonally scaled form of rp_refine_pose: d_i = 1 / sqrt(N_ii), the matrix d_i N_ij d_j off
 *      the diagonal and 1 + lambda on it factored by Cholesky.  A diagonal entry or a pivot that is not positive, a delta that is not
 *      finite, or a trial H whose normalisation breaks down is a BREAKDOWN.
 *   3. The trial H and its cost c'.  ACCEPTED only if c' < c, strictly: then H and c are replaced and lambda <- max(lambda / 10, 1e-7).
 *      Otherwise, and after a breakdown, H is kept and lambda <- min(10 lambda, 1e7).
 * lambda starts at 1e-3.  Exactly `iters` iterations run, two barriers each; there is no early exit.  Each thread's rows (at most 7) stay
 * in registers; LDS holds the reduction buffer (1 408 B) and nothing else.
 * Outputs:
 *   H [n][9]          Frobenius norm 1, sign rule; may alias H0
 *   stat [n][4]       (c at the output, the inlier weight share sum w_p [d_p <= tau^2] / sum w_p at the output, the number of accepted steps, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights at the output
 * iters = 0 is the scorer: H = the normalised H0, c its cost.
 * A DEGENERATE problem -- K < 4, tau not > 0, H0 with a non-finite entry or a norm below 1e-30 -- is not touched: H = H0 copied bit for
 * bit, stat = (0, 0, 0, K), w_out = the clamped base weights.
 * Argument checks before any launch: n <= 0, P < 4, iters < 0, x1 / x2 / tau / H0 / H / stat NULL -> RP_EBADSHAPE;
 * P > RP_HOMOGRAPHY_MAX_P, iters > RP_HOMOGRAPHY_MAX_ITERS -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not
 * 4-byte aligned -> RP_EALIGN. */
int rp_homography_refine(const float* x1, const float* x2, const float* w, const float* tau, const float* H0, int iters,
                         float* H, float* stat, float* w_out, int P, int n, void* stream);

/* Decomposition of H into poses and plane normals: one launch, one workgroup of 256 per problem, every thread decomposes redundantly.
 *   1. (s_1 >= s_2 >= s_3, V) = svd3x3_dev(H); H <- H / s_2; w_c = w_p / (1 + d_p / tau^2), the Cauchy weights at H; the sign of H is
 *      fixed so that sum_p w_c sign(x2h^T H x1h) >= 0 (sign(0) = 0).
 *   2. sigma_i = (s_i / s_2)^2.  If sigma_1 - sigma_3 < 1e-4 the case is PURE ROTATION (or a plane at infinity): one candidate, index 0,
 *      R = U diag(1, 1, det) V^T the rotation nearest to H, t = 0, n = 0, cstat = (1, 0, 0, 1): |t|/d = 0 with valid = 1 is the flag.
 *   3. Otherwise, with v_1, v_2, v_3 the columns of V:  u+- = sqrt((1 - sigma_3) / (sigma_1 - sigma_3)) v_1 +- sqrt((sigma_1 - 1) /
 *      (sigma_1 - sigma_3)) v_3 (numerators clamped at 0);  U = [v_2, u, v_2 x u], W = [H v_2, H u, H v_2 x H u], R = W U^T,
 *      n = v_2 x u, t / d = (H - R) n.  R is re-orthonormalised through its quaternion (Shepperd's branches, normalised, w >= 0).
 *      CANDIDATES, in this order: 0 = (u+, t, n), 1 = (u+, -t, -n), 2 = (u-, t, n), 3 = (u-, -t, -n).
 *   4. Per candidate, over all rows: the VISIBILITY share sum w_c [n^T x1h > 0] / sum w_c, and the Cauchy-robust SAMPSON cost
 *      sum w_p tau^2 log1p(s_p / tau^2) / sum w_p of E = [t^]x R (t^ = t / |t|) with the BASE weights -- expression for expression the
 *      cost of rp_eight_point_consensus and rp_refine_pose, so it sits on one scale with every other pose of the chain.
 * Outputs:
 *   pose [n][4][7]    (t unit, q xyzw unit with w >= 0)
 *   normal [n][4][3]  n, unit
 *   cstat [n][4][4]   (visibility share, Sampson cost, |t| / d, valid 1 / 0)
 *   pick [n][2]       the two best candidates: valid first, then visibility >= vis_min first, then ascending Sampson cost, then index;
 *                     -1 = none
 * An invalid candidate is all zero.  H with a non-finite entry, s_2 = 0 or s_2 < 1e-6 s_1, tau not > 0, or sum w_c not > 0 gives four
 * invalid candidates and pick = (-1, -1).
 * Argument checks before any launch: n <= 0, P < 1, H / x1 / x2 / tau / pose / normal / cstat / pick NULL -> RP_EBADSHAPE;
 * P > RP_HOMOGRAPHY_MAX_P -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not 4-byte aligned -> RP_EALIGN. */
int rp_pose_from_homography(const float* H, const float* x1, const float* x2, const float* w, const float* tau, float vis_min,
                            float* pose, float* normal, float* cstat, int* pick, int P, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_HOMOGRAPHY_H */
