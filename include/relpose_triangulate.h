/*
 * relpose_triangulate.h -- C ABI of librelpose_triangulate.so (gfx950 / MI355X): two-view structure -- the optimal correction of every
 * match onto the epipolar constraint of a given pose, the point both corrected rays meet in, its depths, its parallax and the
 * reprojection error.
 *
 * Every other library of the chain answers "where is camera 2?" and reports the Sampson distance, a first-order stand-in for the
 * reprojection error.  This ninth, small library answers "where are the points?": per match the nearest pair (x1c, x2c) that satisfies
 * x2ch^T E x1ch = 0 exactly (Lindstrom's two-step scheme: a fixed trip count, no polynomial), the intersection of the two rays, and per
 * problem the robust reprojection cost, the share of the points in front of both cameras and the mean parallax.
 *
 * CONVENTION.  Calibrated coordinates, X2 = R X1 + t as in rp_eight_point, E = [t]x R, x2h^T E x1h = 0 (homogeneous x = (x, y, 1));
 * a pose is (t, q xyzw) as rp_pose_from_essential writes it.  t is normalised, so points and depths are in units of the baseline.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace, no randomness): results are bit-identical from call to call.  Nothing non-finite is written for
 * finite inputs.
 */
#ifndef RELPOSE_TRIANGULATE_H
#define RELPOSE_TRIANGULATE_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_triangulate_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_TRIANGULATE_ABI_VERSION 1
#define RP_TRIANGULATE_MAX_P 1728         /* 3 heads x 576 tokens */
int rp_triangulate_abi_version(void);

/* Batched triangulation of n problems of P correspondences each under one pose per problem: one launch, one workgroup of 256 per
 * problem, a thread owns the rows tid + 256 k (at most 7), ONE fused six-value reduction; every loop has a fixed trip count.
 *   pose [n][7]       (t, q xyzw); t and q are normalised internally
 *   x1, x2 [n][P][2]  the matches
 *   w [n][P]          base weights; NULL = all ones; a negative weight (or a NaN) counts as 0
 *   tau [n]           scale of the robust cost, > 0; required
 * The weights enter `stat` only: every row of a non-degenerate problem is triangulated whatever its weight.
 * OPTIMAL CORRECTION of a row.  With a_ = x2h, b_ = x1h, E~ the upper-left 2 x 2 of E, m = (E b_)_xy, m' = (E^T a_)_xy:
 *   1. a = m^T E~ m', b = ((|m|^2 + |m'|^2)) / 2, c = a_^T E b_, d = sqrt(max(b^2 - a c, 0)), lambda = c / (b + d)
 *   2. D2 = lambda m, D1 = lambda m'
 *   3. m <- m - E~ D1, m' <- m' - E~^T D2
 *   4. lambda <- lambda 2 d / (|m|^2 + |m'|^2), D2 = lambda m, D1 = lambda m'
 *   5. x2c = x2 - D2, x1c = x1 - D1
 * A denominator (b + d in step 1, |m|^2 + |m'|^2 in step 4) that is not above 1e-30 gives lambda = 0 there: both points sit at the
 * epipoles, the row stays uncorrected.  (x1c, x2c) is the minimiser of |x1 - x1c|^2 + |x2 - x2c|^2 on the constraint, the reprojection
 * error for a fixed E, to second order in the correction.
 * THE POINT of a row.  x1ch, x2ch the corrected points, homogeneous; r = R x1ch, g = x2ch x r:
 *   z1 = (t x x2ch) . g / |g|^2,  z2 = (t x r) . g / |g|^2     the depths in camera 1 and camera 2
 *   X = z1 x1ch                                                the point, in the frame of camera 1
 *   phi = atan2(|g|, x2ch . r)                                 the parallax, radians
 *   d2 = |D1|^2 + |D2|^2                                       the squared reprojection error, summed over both images
 * A row with |g|^2 < 1e-10 |x2ch|^2 |r|^2 (sin phi below 1e-5: fp32 cannot resolve the parallax) is AT INFINITY: X = 0, z1 = z2 = 0;
 * its d2 and phi are written all the same.  A negative depth is written as it is: it is information about the match, not an error.
 * Outputs:
 *   X [n][P][3]       the triangulated point
 *   aux [n][P][4]     (z1, z2, d2, phi)
 *   xc [n][P][4]      (NULL = off) (x1c, x2c)
 *   stat [n][4]       with o_p = w_p / (1 + d2_p / tau^2), the Cauchy weights:
 *                       the robust reprojection cost sum_p w_p tau^2 log1p(d2_p / tau^2) / sum_p w_p -- on the scale of the Sampson
 *                         costs of rp_refine_pose and rp_eight_point_consensus, of which d2 is the exact counterpart;
 *                       the share in front of both cameras, sum_p o_p [z1 > 0 and z2 > 0] / sum_p o_p (rows at infinity: not in front);
 *                       the Cauchy-weighted mean parallax sum_p o_p phi_p / sum_p o_p, radians;
 *                       K, the number of rows of positive weight.
 *                     With K = 0 (or sum_p o_p not > 0) the rows are written all the same and the three quotients are 0.
 * A DEGENERATE problem -- |t| or |q| below 1e-30 (t = 0 is a pure rotation: there is nothing to triangulate), a pose with a non-finite
 * entry, or a tau that is not > 0 -- gives X = 0, aux = 0, xc = 0 and stat = (0, 0, 0, K).
 * Argument checks before any launch: n <= 0, P < 1, pose / x1 / x2 / tau / X / aux / stat NULL -> RP_EBADSHAPE;
 * P > RP_TRIANGULATE_MAX_P -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not 4-byte aligned -> RP_EALIGN. */
int rp_triangulate(const float* pose, const float* x1, const float* x2, const float* w, const float* tau,
                   float* X, float* aux, float* xc, float* stat, int P, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_TRIANGULATE_H */
