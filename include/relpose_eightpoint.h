/*
 * relpose_eightpoint.h -- C ABI of librelpose_eightpoint.so (gfx950 / MI355X): the classical eight-point algorithm on the GPU.
 *
 * The network of this project learns the eight-point algorithm implicitly; this third, small library is the explicit one, so the two can
 * be compared on the device: correspondences (relpose_readout.h: rp_emm_matches, or any other matcher) -> essential matrix E -> pose
 * (relpose_hip.h: rp_pose_from_essential).  The reference has no counterpart: it regresses R, t and never estimates E from matches.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace, no randomness): results are bit-identical from call to call.
 */
#ifndef RELPOSE_EIGHTPOINT_H
#define RELPOSE_EIGHTPOINT_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_eightpoint_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_EIGHTPOINT_ABI_VERSION 1
#define RP_EIGHTPOINT_MAX_P 1728          /* 3 heads x 576 tokens */
#define RP_EIGHTPOINT_MAX_ITERS 16
int rp_eightpoint_abi_version(void);

/* Batched weighted, normalised eight-point solver with robust re-weighting: n independent problems of P correspondences each, one
 * workgroup per problem, the whole iteration in one launch.
 *   x1, x2 [n][P][2]  normalised image coordinates of the same 3-D points in camera 1 / camera 2, in the convention of
 *                     rp_pose_from_essential: X2 = R X1 + t, E = [t]x R, x2^T E x1 = 0 (homogeneous x = (x, y, 1))
 *   w [n][P]          base weights; NULL = all ones; a negative weight (or a NaN) counts as 0
 *   tau [n]           scale of the robust weight, in units of the square root of the Sampson distance (so: of normalised image
 *                     coordinates), > 0; may be NULL only when iters == 0
 * One SOLVE with weights w_p:
 *   1. Hartley normalisation per image: the weighted centroid c = x_0 + sum w (x - x_0) / sum w (taken about the first point, so that
 *      coincident points give exactly c = x_0) goes to the origin, the weighted mean distance m = sum w |x - c| / sum w to sqrt 2:
 *      x^ = (x - c) sqrt 2 / m, i.e. x^h = T xh with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], s = sqrt 2 / m.
 *   2. The rows sqrt(w_p) (x2^h (x) x1^h) = sqrt(w_p) [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of a [P][9] matrix A (for a
 *      row-major F^).  F^ is the right singular vector of A's smallest singular value, found by a one-sided (Hestenes) Jacobi iteration
 *      on A itself -- never on the 9 x 9 normal matrix A^T A, which would square the condition number: fp32 is adequate for the
 *      former only.  A fixed number of cyclic sweeps over the 36 column pairs in the order (0,1), (0,2), .. (7,8).
 *   3. F = T2^T F^ T1, then the projection onto the essential manifold: F = U diag(e1, e2, e3) V^T -> E = U diag(1, 1, 0) V^T.
 *   4. The sign: the entry of E of the largest magnitude is positive; among equal magnitudes the lowest index decides.
 * Re-weighting: `iters` rounds of iteratively re-weighted least squares with a Cauchy weight, iters + 1 solves in all.  Solve 0 uses
 * the base weights; after solve k, with E_k its result,
 *      w_{k+1,p} = w_p / (1 + d_p(E_k) / tau^2),
 *      d_p(E) = (x2^T E x1)^2 / ((E x1)_x^2 + (E x1)_y^2 + (E^T x2)_x^2 + (E^T x2)_y^2)   (the Sampson distance; d = 0 where the
 *      denominator is 0, and then w_{k+1,p} = w_p).
 * Outputs:
 *   E [n][9]          row-major, singular values (1, 1, 0)
 *   stat [n][4]       of the LAST solve: (sigma_9 / sigma_1, sigma_8 / sigma_1, e2 / e1, wsum) -- sigma_1 >= .. >= sigma_9 the singular
 *                     values of A (a small sigma_8 / sigma_1 flags a degenerate configuration: a planar scene, a pure rotation),
 *                     e2 / e1 the ratio of the two largest singular values of F before the projection (1 for a true essential
 *                     matrix), wsum the sum of the weights the solve used
 *   w_out [n][P]      (NULL = off) the weights the last solve used
 * A DEGENERATE solve -- fewer than 8 rows of positive weight, or a weighted mean distance of 0 (below 1e-30) in either image -- ends
 * its problem: E = 0, stat = (0, 0, 0, wsum), w_out = the weights as they stood.  Nothing non-finite is written for finite inputs.
 * P <= RP_EIGHTPOINT_MAX_P: the nine columns of A stay in LDS for the whole iteration.
 * Argument checks before any launch: n <= 0, P < 8, iters < 0, x1 / x2 / E / stat NULL, tau NULL with iters > 0 -> RP_EBADSHAPE;
 * P > RP_EIGHTPOINT_MAX_P, iters > RP_EIGHTPOINT_MAX_ITERS -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other pointer not
 * 4-byte aligned -> RP_EALIGN. */
int rp_eight_point(const float* x1, const float* x2, const float* w, const float* tau, float* E, float* stat, float* w_out,
                   int P, int iters, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_EIGHTPOINT_H */
