/*
 * relpose_fivepoint.h -- C ABI of librelpose_fivepoint.so (gfx950 / MI355X): the calibrated five-point consensus, a seeded
 * hypothesise-and-verify whose minimal solver uses the known intrinsics.
 *
 * rp_eight_point_consensus (relpose_consensus.h) draws eight rows per hypothesis: with 60 % of outliers a sample is clean with
 * probability 0.4^8 = 0.07 %, less than one in 1024.  The calibrated minimal problem needs five rows (0.4^5 = 1 %).  This seventh,
 * small library is that header's consensus with a five-point solve in place of the eight-point one: up to ten essential matrices per
 * sample, every one of them scored against ALL rows with the same robust cost, the best one returned with the Cauchy weights at it.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_FIVEPOINT_H
#define RELPOSE_FIVEPOINT_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_fivepoint_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_FIVEPOINT_ABI_VERSION 1
#define RP_FIVEPOINT_MAX_P 1728           /* 3 heads x 576 tokens */
#define RP_FIVEPOINT_MAX_M 4096
#define RP_FIVEPOINT_ROOTS 10             /* slots per sample: a five-point problem has at most ten real solutions */
int rp_fivepoint_abi_version(void);

/* Five-point consensus: n independent problems of P correspondences, M samples each, ten slots per sample; two launches on `stream`.
 *   x1, x2 [n][P][2], w [n][P] (NULL = ones; negative or NaN counts as 0), tau [n] (> 0, required), seed: exactly as for
 *   rp_eight_point_consensus.  x1, x2 are CALIBRATED coordinates: X2 = R X1 + t, x2^T E x1 = 0.
 * ROWS.  pos is the ascending list of the rows of positive weight, K its length.
 * SAMPLER.  That of relpose_consensus.h with five draws: the same mix, the same s = mix(mix(seed + 0x9E3779B9 (i + 1)) ^ m) for problem i
 *   and sample m; for k = 0 .. 4: r = mix(s + 0x9E3779B9 (k + 1)), j = K - 5 + k, t = (r (j + 1)) >> 32, c_k = j if t is among
 *   c_0 .. c_{k-1}, else t.  The sample is the rows pos[c_0] .. pos[c_4].
 * SOLVE of one sample, in fp64 up to the last step (the 10 x 10 block's condition number exceeds 1e4 in 5 % of exact samples; float32
 *   loses roots there):
 *   - the five rows x2h (x) x1h, NO Hartley normalisation (a similarity per image would break the essential constraints);
 *   - an orthonormal basis X, Y, Z, W of their null space: five Householder reflections of the 9 x 5 transpose applied to e_6 .. e_9,
 *     never the 9 x 9 normal matrix;
 *   - for E = x X + y Y + z Z + W the ten cubics det E = 0, 2 E E^T E - tr(E E^T) E = 0 in the 20 monomials of degree <= 3, ordered
 *     x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | x xz xz^2 y yz yz^2 1 z z^2 z^3;
 *   - Gauss-Jordan elimination of the first ten columns with partial (row) pivoting;
 *   - ROUTE: Nister's tenth-degree polynomial.  The rows of x^2z, x^2, y^2z, y^2, xyz, xy give (row - z next row) three equations
 *     B(z) (x, y, 1)^T = 0 with entries of degree 3, 3, 4; p(z) = det B(z).  Its real roots in [-R, R], R = 1 + max |p_i / p_10| (Cauchy),
 *     are bracketed by the real roots of p', those by the roots of p'', ... down to the linear derivative; a bracket with a sign
 *     change is halved 48 times and polished by 4 Newton steps that may not leave it.  Every loop has a fixed trip count.  (x, y, 1)
 *     is the largest of the three cross products of two rows of B(z);
 *   - each solution is rounded to float32 at Frobenius norm 1 and finished as rp_eight_point finishes F: U diag(1, 1, 0) V^T with
 *     svd3x3_dev, then that header's sign rule (the entry of largest magnitude, the first of equal ones, is positive).
 *   A sample BREAKS DOWN when a Householder column norm or an elimination pivot is below 1e-12, or p_10 = 0 / R is not finite: no roots.
 * SLOTS.  A sample's roots fill slots 0 .. c-1 in ASCENDING z, skipping a root with a non-finite entry or a non-finite cost; every
 *   further slot is invalid: hyp_E = 0, hyp_cost = FLT_MAX.
 * SCORE.  hyp_cost[i][m][k] = sum_p w_p tau^2 log1p(d_p / tau^2) / sum_p w_p over pos ascending, the cost of relpose_consensus.h (fp32).
 * SELECTION.  The minimum of hyp_cost over the valid slots; among equal minima the lowest (m, k).
 * Outputs:
 *   E [n][9]          the best root, bit for bit
 *   best [n][2]       (m, k)
 *   stat [n][4]       (its cost, the inlier weight share sum w_p [d_p <= tau^2] / sum w_p at E, the number of valid slots, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights w_p / (1 + d_p / tau^2) at E
 *   hyp_E [n][M][10][9], hyp_cost [n][M][10]   REQUIRED outputs, fully written; the second launch reads what the first wrote there
 *   samples [n][M][5] (NULL = off) the sampled row indices
 * A DEGENERATE problem -- K < 5, tau not > 0, or no valid slot -- gives E = 0, best = (-1, -1), stat = (0, 0, number of valid slots, K),
 * w_out = the clamped base weights; with K < 5 or tau not > 0 every slot is written as invalid, and samples = 0 where K < 5.  Nothing
 * non-finite is written for finite inputs.
 * LAYOUT.  hypothesis kernel: grid n ceil(M / 256), 256 threads, one lane per sample; 42 496 B of LDS hold the compacted rows; the
 * 10 x 20 system (1600 B) is the lane's private array and lives in scratch, as the root brackets do.  Selection kernel: grid n, 256
 * threads, 2 176 B of LDS.
 * Argument checks before any launch: n <= 0, P < 5, M < 1, a required pointer NULL -> RP_EBADSHAPE; P > RP_FIVEPOINT_MAX_P,
 * M > RP_FIVEPOINT_MAX_M (or more than 2^31 - 1 workgroups, n ceil(M / 256)) -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other
 * pointer not 4-byte aligned -> RP_EALIGN. */
int rp_five_point_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed,
                            float* E, int* best, float* stat, float* w_out,
                            float* hyp_E, float* hyp_cost, int* samples, int P, int M, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_FIVEPOINT_H */
