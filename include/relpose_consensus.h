/*
 * relpose_consensus.h -- C ABI of librelpose_consensus.so (gfx950 / MI355X): a seeded hypothesise-and-verify in front of the eight-point
 * solver.
 *
 * rp_eight_point (relpose_eightpoint.h) and rp_refine_pose (relpose_refine.h) are local methods started from the all-data least-squares
 * solution; beyond some 20 % of outliers that start lies in a wrong basin and neither leaves it.  This fifth, small
 * library supplies the start: M minimal eight-point solves on sampled rows, each scored against ALL rows with the robust cost that
 * rp_refine_pose reports, the best one returned together with the Cauchy weights at it -- which rp_eight_point takes as base weights.
 * The sampler is counter based: the same seed gives the same samples, so the memory contract below holds as everywhere else.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_CONSENSUS_H
#define RELPOSE_CONSENSUS_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_consensus_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_CONSENSUS_ABI_VERSION 1
#define RP_CONSENSUS_MAX_P 1728           /* 3 heads x 576 tokens */
#define RP_CONSENSUS_MAX_M 4096
int rp_consensus_abi_version(void);

/* Consensus eight-point: n independent problems of P correspondences, M hypotheses each; two launches on `stream`.
 *   x1, x2 [n][P][2]  normalised image coordinates, the convention of rp_eight_point: X2 = R X1 + t, x2^T E x1 = 0
 *   w [n][P]          base weights; NULL = all ones; a negative weight (or a NaN) counts as 0
 *   tau [n]           scale of the robust cost, in units of the square root of the Sampson distance, > 0; required
 *   seed              any int; used as its 32-bit pattern
 * ROWS.  pos is the ascending list of the rows of positive weight, K its length.
 * SAMPLER (all arithmetic modulo 2^32).  mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   For problem i and hypothesis m: s = mix(mix(seed + 0x9E3779B9 (i + 1)) ^ m); for k = 0 .. 7: r = mix(s + 0x9E3779B9 (k + 1)),
 *   j = K - 8 + k, t = (r (j + 1)) >> 32 (the 64-bit product), c_k = j if t is among c_0 .. c_{k-1}, else t  -- Floyd's sampling: eight
 *   draws, always distinct, uniform over the subsets.  The sample is the rows pos[c_0] .. pos[c_7], in that order.
 * HYPOTHESIS m is the solve of rp_eight_point with iters = 0 on those eight rows with unit weights: Hartley normalisation (about the
 *   first sampled row), the null vector of the 8 x 9 row matrix -- by Householder reflections of its transpose, never through the
 *   9 x 9 normal matrix --, F = T2^T F^ T1, the projection to singular values (1, 1, 0), that header's sign rule.  A solve that breaks
 *   down (a mean distance below 1e-30 in either image) or yields a non-finite entry or a non-finite cost is INVALID: hyp_E = 0,
 *   hyp_cost = FLT_MAX.
 * SCORE.  hyp_cost[i][m] = sum_p w_p tau^2 log1p(d_p / tau^2) / sum_p w_p over pos in ascending order, d_p the Sampson distance of
 *   rp_eight_point (0 where its denominator is 0): the cost rp_refine_pose reports.
 * SELECTION.  best[i] = the lowest index of the minimum hyp_cost among the valid hypotheses.
 * Outputs:
 *   E [n][9]          hyp_E[best], bit for bit
 *   best [n]          see above
 *   stat [n][4]       (hyp_cost[best], the inlier weight share sum w_p [d_p <= tau^2] / sum w_p at E, the number of valid hypotheses, K)
 *   w_out [n][P]      (NULL = off) the Cauchy weights w_p / (1 + d_p / tau^2) at E: base weights for rp_eight_point
 *   hyp_E [n][M][9], hyp_cost [n][M]   REQUIRED outputs, fully written: every hypothesis and its cost.  The second launch reads what
 *                     the first wrote there; they are results, not a workspace
 *   samples [n][M][8] (NULL = off) the sampled row indices
 * A DEGENERATE problem -- K < 8, tau not > 0, or no valid hypothesis -- gives E = 0, best = -1, stat = (0, 0, number of valid
 * hypotheses, K), w_out = the clamped base weights; with K < 8 or tau not > 0 every hypothesis is written as invalid, and samples = 0
 * where K < 8.  Nothing non-finite is written for finite inputs.
 * Argument checks before any launch: n <= 0, P < 8, M < 1, a required pointer NULL -> RP_EBADSHAPE; P > RP_CONSENSUS_MAX_P,
 * M > RP_CONSENSUS_MAX_M (or more than 2^31 - 1 workgroups, n ceil(M / 256)) -> RP_EUNSUPPORTED; x1 / x2 not 8-byte aligned, any other
 * pointer not 4-byte aligned -> RP_EALIGN. */
int rp_eight_point_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed,
                             float* E, int* best, float* stat, float* w_out,
                             float* hyp_E, float* hyp_cost, int* samples, int P, int M, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_CONSENSUS_H */
