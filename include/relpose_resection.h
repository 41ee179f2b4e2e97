/*
 * relpose_resection.h -- C ABI of librelpose_resection.so (gfx950 / MI355X): camera resection -- the pose of a camera from 3-D points
 * and their images: three-point (P3P) consensus and a six-parameter non-linear polish.
 *
 * Every other solver library relates the two images of ONE pair, and every translation it returns is a direction: rp_triangulate writes
 * points in units of the baseline.  Two pairs that share an image give two baselines of unknown ratio.  This fifteenth
 * library relates a third image to the structure of a pair: given the points X_p (rp_triangulate, in the frame of the shared image) and
 * their images x_p in the third camera it fits the pose (R, t) of that camera, and the LENGTH of t is the ratio of the two baselines.
 *
 * CONVENTION.  Calibrated image coordinates.  m = R X + t, x ~ (m_x / m_z, m_y / m_z); R = quat_to_rot(q), row-major.  A pose is
 * (t, q xyzw) with w >= 0 and |q| = 1; t is NOT normalised: its length is the result.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.  Nothing non-finite is written for finite inputs.
 */
#ifndef RELPOSE_RESECTION_H
#define RELPOSE_RESECTION_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_resection_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_RESECTION_ABI_VERSION 1
#define RP_RESECTION_MAX_P 1728           /* 3 heads x 576 tokens */
#define RP_RESECTION_MAX_M 4096
#define RP_RESECTION_MAX_ITERS 64
int rp_resection_abi_version(void);

/* DISTANCE of a row under a pose (t, q), used by both entry points, fp32: with R = quat_to_rot(q) (csrc/two_view.h),
 * m_i = ((R_i0 X_x + R_i1 X_y) + R_i2 X_z) + t_i, e = (m_x - u m_z, m_y - v m_z), x = (u, v),
 *      d = min((e_x^2 + e_y^2) / max(m_z^2, 1e-30), 1e30)   if m_z > 0 and m_z^2 >= 1e-30,       d = 1e30   otherwise
 * -- the form of relpose_rotation.h with m = R X + t: d = |m_xy / m_z - x|^2, and a point behind the camera or on its horizon costs the
 * maximum.  ROBUST COST of a pose: c = sum_p w_p tau^2 log1p(d_p / tau^2) / sum_p w_p, weights clamped at 0 (a NaN counts as 0);
 * INLIER SHARE: sum w_p [d_p <= tau^2] / sum w_p. */

/* P3P consensus: n independent problems of P point-image rows, M hypotheses each; two launches on `stream`.
 *   X [n][P][3]  the points, x [n][P][2] their images, w [n][P] (NULL = ones; negative or NaN counts as 0), tau [n] (> 0, required),
 *   seed: as for rp_rotation_consensus.
 * ROWS.  pos is the ascending list of the rows of positive weight, K its length.
 * SAMPLER.  That of relpose_consensus.h with three draws: the same mix, the same s = mix(mix(seed + 0x9E3779B9 (i + 1)) ^ m) for problem
 *   i and hypothesis m; for k = 0, 1, 2: r = mix(s + 0x9E3779B9 (k + 1)), j = K - 3 + k, t = (r (j + 1)) >> 32, c_k = j if t is among
 *   c_0 .. c_{k-1}, else t.  The sample is the rows pos[c_0], pos[c_1], pos[c_2], in that order.
 * HYPOTHESIS m, per lane: Grunert's three-point solution, in fp64 (the precedent is the five-point library), every loop of a fixed trip
 *   count and every index static.  The inputs are the fp32 rows, converted exactly.
 *   1. Bearings f_k = (u_k, v_k, 1) / sqrt((u_k^2 + v_k^2) + 1); ca = f_1 . f_2, cb = f_0 . f_2, cg = f_0 . f_1 (dot: (a_0 b_0 + a_1 b_1)
 *      + a_2 b_2); squared sides a2 = |X_1 - X_2|^2, b2 = |X_0 - X_2|^2, c2 = |X_0 - X_1|^2 (of the differences, the same sum).
 *   2. INVALID sample (thresholds): a side with a2, b2 or c2 < 1e-12 max(a2, b2, c2) (coincident points, or not a number);
 *      |(X_1 - X_0) x (X_2 - X_0)|^2 < 1e-12 c2 b2 (collinear points); |f_i x f_j|^2 < 1e-12 for a pair of bearings (they coincide).
 *   3. With the distances s_0, s_1 = y s_0, s_2 = v s_0 of the points along the bearings, k = (a2 - c2) / b2, l = c2 / b2, the law of
 *      cosines in the three sides gives y = N(v) / D(v), N = (1 + k) - 2 k cb v + (k - 1) v^2, D = 2 cg - 2 ca v, and the quartic
 *      A(v) = D^2 + N^2 - 2 cg N D - l (1 - 2 cb v + v^2) D^2 = 0, its five coefficients from the products of the coefficient lists.
 *      INVALID if |A_4| <= 1e-12 max_i |A_i| (a root at infinity), or a coefficient is not a number.
 *   4. Real roots, closed form (Ferrari).  Monic a_i = A_i / A_4; v = z - a_3 / 4 gives z^4 + p z^2 + q z + r.  The resolvent
 *      m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0: its LARGEST real root by Cardano (one real root: the sum of the two cube roots;
 *      three: 2 sqrt(-P / 3) cos(acos(clamp(.)) / 3)), then TWO Newton steps on the resolvent.  If m > 1e-14 max(1, |p|): s = sqrt(2 m),
 *      and the roots of z^2 - s z + (p / 2 + m + q / (2 s)) and z^2 + s z + (p / 2 + m - q / (2 s)); otherwise (a biquadratic)
 *      z^2 = (-p +- sqrt(p^2 - 4 r)) / 2.  A quadratic has real roots if its discriminant is >= -1e-9 times the magnitude of its terms; a
 *      negative discriminant within that band counts as 0 (a double root is kept, twice).
 *      SLOTS 0 .. 3: (first quadratic +, -), (second quadratic +, -); biquadratic: (+sqrt z2_+, -sqrt z2_+, +sqrt z2_-, -sqrt z2_-).
 *      Every root is polished by THREE Newton steps on the monic quartic (a step with a derivative of 0 is skipped).
 *   5. A slot is a SOLUTION if v > 0, |D(v)| >= 1e-9, den = (1 - 2 cb v) + v^2 > 0 and y > 0, where y is the root cg +- sqrt(w2),
 *      w2 = (cg^2 - 1) + l den, of the side X_0 X_1's own equation y^2 - 2 cg y + (1 - l den) = 0 that is nearer to N / D (of equally
 *      near ones the +; y = N / D itself if w2 < 0): N / D names the branch, but where N and D vanish together its value is lost.
 *      s_0 = sqrt(b2 / den), s_1 = y s_0, s_2 = v s_0: all three depths positive.
 *   6. The pose of a solution: Y_k = s_k f_k; the frames e_1 = unit(X_1 - X_0), e_3 = unit(e_1 x (X_2 - X_0)), e_2 = e_3 x e_1 and
 *      g_1, g_2, g_3 from Y likewise; R_rc = (g_1r e_1c + g_2r e_2c) + g_3r e_3c; t = Y_0 - R X_0; q = rot_to_quat(R) (Shepperd's
 *      branches, fp64).  (t, q) are rounded to fp32 and q is normalised again in fp32 (unit<4>, w >= 0).  A solution with a non-finite
 *      entry is dropped.
 *   A sample with no solution is INVALID, too.  INVALID: hyp_pose = 0, hyp_cost = FLT_MAX, hyp_count = 0.
 * SCORE.  Every solution is scored by the robust cost of its fp32 pose on all K rows in ONE walk over pos in ascending order (up to four
 *   running sums); a solution with a cost that is not below FLT_MAX is dropped.  The lane keeps its cheapest solution, of equal ones the
 *   first in slot order: hyp_pose[i][m], hyp_cost[i][m]; hyp_count[i][m] is the number of solutions that were kept to the end.
 * SELECTION.  best[i] = the lowest index of the minimum hyp_cost among the valid hypotheses.
 * Outputs:
 *   pose [n][7]       hyp_pose[best], bit for bit
 *   best [n]          see above
 *   stat [n][4]       (hyp_cost[best], the inlier weight share at pose, the number of valid hypotheses, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights w_p / (1 + d_p / tau^2) at pose
 *   hyp_pose [n][M][7], hyp_cost [n][M]   REQUIRED outputs, fully written; the second launch reads what the first wrote there
 *   hyp_count [n][M]  (NULL = off), int
 *   samples [n][M][3] (NULL = off) the sampled row indices
 * A DEGENERATE problem -- K < 3, tau not > 0, or no valid hypothesis -- gives pose = 0, best = -1, stat = (0, 0, number of valid
 * hypotheses, K), w_out = the clamped base weights; with K < 3 or tau not > 0 every hypothesis is invalid, and samples = 0 where K < 3.
 * LAYOUT.  hypothesis kernel: grid n ceil(M / 256), 256 threads, one lane per hypothesis, 63 232 B of LDS: the rows of the shared
 * consensus core as they are (42 496 B; its staging takes two float2 operands, the image is both) and the points of the same rows
 * (20 736 B) -- 36 B per row where 28 B would do: the price of ONE definition of the staging and the sampler; two workgroups per CU
 * either way, the registers allow no more.  No scratch.  Selection kernel: grid n, 256 threads, 2 176 B of LDS.
 * Argument checks before any launch: n <= 0, P < 3, M < 1, a required pointer NULL -> RP_EBADSHAPE; P > RP_RESECTION_MAX_P,
 * M > RP_RESECTION_MAX_M (or more than 2^31 - 1 workgroups, n ceil(M / 256)) -> RP_EUNSUPPORTED; x not 8-byte aligned, any other
 * pointer not 4-byte aligned -> RP_EALIGN. */
int rp_p3p_consensus(const float* X, const float* x, const float* w, const float* tau, int seed,
                     float* pose, int* best, float* stat, float* w_out,
                     float* hyp_pose, float* hyp_cost, int* hyp_count, int* samples, int P, int M, int n, void* stream);

/* Levenberg-Marquardt on the robust cost over the six degrees of freedom of the pose: one launch, one workgroup of 256 per problem.
 *   pose0 [n][7]      the start (t, q); q of any length >= 1e-30
 * STATE.  t = t0, q = unit(q0) with the sign fixed so that w >= 0; R = quat_to_rot(q) wherever a matrix is needed.
 * Parameters, six: (omega, upsilon) moves q to q' = unit((omega / 2, 1) (x) q), the sign fixed so that w >= 0 (the product of
 *   relpose_rotation.h), and t to t' = t + upsilon.
 * Residual of row p: r = (e_x / m_z, e_y / m_z); its Jacobian at 0, exact, from dm = omega x Y + upsilon, Y = R X = m - t (computed as the
 *   three sums without t): with i = 1 / m_z, p_x = m_x i, p_y = m_y i,
 *      Jx = i (-(p_x Y_y),          Y_z + p_x Y_x,  -Y_y,  1,  0,  -p_x),
 *      Jy = i (-(Y_z + p_y Y_y),    p_y Y_x,         Y_x,  0,  1,  -p_y).
 *   A row with m_z <= 0 or m_z^2 < 1e-30 has no derivative: it enters the normal equations with weight 0 (and the cost with the
 *   clamped d).
 * One ITERATION at (t, q) with cost c and damping lambda:
 *   1. N = sum_p o_p J_p^T J_p (6 x 6), g = sum_p o_p J_p^T r_p with o_p = w_p / (1 + d_p / tau^2): ONE fused reduction of 27 values, the
 *      21 of the upper triangle row by row and the 6 of g.
 *   2. (N + lambda diag N) delta = -g in the diagonally scaled form of rp_refine_pose (lm_cholesky_solve<6>).  A diagonal entry or a pivot
 *      that is not positive, a delta that is not finite, or a trial q' that has no direction is a BREAKDOWN.
 *   3. The trial (t', q') and its cost c'.  ACCEPTED only if c' < c, strictly: then the state and c are replaced and
 *      lambda <- max(lambda / 10, 1e-7).  Otherwise, and after a breakdown, the state is kept and lambda <- min(10 lambda, 1e7).
 * lambda starts at 1e-3.  Exactly `iters` iterations run, two barriers each; there is no early exit.  Each thread's rows (at most 7) stay
 * in registers; LDS holds the reduction buffer (864 B) and nothing else.
 * Outputs:
 *   pose [n][7]       (t, q) at the output; may alias pose0
 *   stat [n][4]       (c at the output, the inlier weight share at the output, the number of accepted steps, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights at the output
 * iters = 0 is the scorer: pose = (t0, unit(q0)), c its cost.
 * A DEGENERATE problem -- K < 3, tau not > 0, pose0 with a non-finite entry or |q0| below 1e-30 (the zero pose that rp_p3p_consensus
 * writes for a degenerate problem) -- is not touched: pose = pose0 copied bit for bit, stat = (0, 0, 0, K), w_out = the clamped base
 * weights.
 * Argument checks before any launch: n <= 0, P < 3, iters < 0, X / x / tau / pose0 / pose / stat NULL -> RP_EBADSHAPE;
 * P > RP_RESECTION_MAX_P, iters > RP_RESECTION_MAX_ITERS -> RP_EUNSUPPORTED; x not 8-byte aligned, any other pointer not 4-byte
 * aligned -> RP_EALIGN. */
int rp_pnp_refine(const float* X, const float* x, const float* w, const float* tau, const float* pose0, int iters,
                  float* pose, float* stat, float* w_out, int P, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_RESECTION_H */
