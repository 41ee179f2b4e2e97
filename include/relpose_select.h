/*
 * relpose_select.h -- C ABI of librelpose_select.so (gfx950 / MI355X): which two-view model do the matches support -- the essential
 * matrix, the plane-induced homography or the pure rotation.
 *
 * Every essential-matrix chain fails on a plane, every chain returns a meaningless translation on a rotating pair, and the planar chain
 * spends eight parameters on a rotation.  This thirteenth, small library puts the candidates those chains
 * return on ONE scale, an information criterion: the residuals of a match under each candidate, a noise scale taken
 * from the residuals themselves, and per candidate the cost of coding every match either as an inlier of the model or as an outlier --
 * an outlier costs the same under every model, so the choice depends on the inliers alone.
 *
 * CONVENTION.  Calibrated coordinates, homogeneous x = (x, y, 1); a candidate is a row-major [9] matrix of kind
 *      0  essential     x2h^T E x1h = 0
 *      1  homography    x2h ~ H x1h
 *      2  rotation      x2h ~ R x1h, and R x1h in front of the second camera
 * of any scale (and, for kinds 0 and 1, any sign).
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, and the memory
 * contract -- every documented output element is written by every call, nothing else is, and no result depends on what an output held
 * before (no atomics, no workspace): results are bit-identical from call to call.  Nothing non-finite is written for finite inputs.
 */
#ifndef RELPOSE_SELECT_H
#define RELPOSE_SELECT_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_select_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_SELECT_ABI_VERSION 1
#define RP_SELECT_MAX_P 1728              /* 3 heads x 576 tokens */
#define RP_SELECT_MAX_C 8                 /* candidates per problem */
int rp_select_abi_version(void);

/* Model selection: n independent problems of P correspondences and C candidates each; one launch, one workgroup of 256 per problem.
 *   x1, x2 [n][P][2], w [n][P] (NULL = ones), tau [n] (> 0, required: the band of the scale estimate), sigma [n] or NULL (an entry > 0
 *   is the noise scale, used as given; any other entry, a NaN included: estimated), models [n][C][9],
 *   kinds [C] in {0, 1, 2}: a HOST array, read before the launch and the same for every problem,
 *   outlier_cost: the fixed cost of coding a row as an outlier, > 3 ln 4 and <= 1e6 (8 = twice the dimension r = 4 of a match).
 * ROWS.  pos is the list of the rows of positive weight (a negative one or a NaN counts as 0), K its length.  The criterion counts a
 *   row ONCE: the weights only say which rows exist, their size is not used.
 * MODEL TABLE (d the dimension of the model's manifold in the space of matches, k its parameters, 4 - d its codimension):
 *      essential (3, 5, 1)        homography (2, 8, 2)        rotation (2, 3, 2)
 * RESIDUAL e2 of row p = (x, y) <-> (u, v) under candidate c with matrix h, fp32; every sum is taken left to right unless
 *   parenthesised:
 *   kind 0: s = sampson(h, x1, x2) of csrc/two_view.h: l2 = (h0 x + h1 y + h2, h3 x + h4 y + h5, h6 x + h7 y + h8),
 *      l1 = (h0 u + h3 v + h6, h1 u + h4 v + h7), r = u l2_x + v l2_y + l2_z, den = l2_x^2 + l2_y^2 + l1_x^2 + l1_y^2,
 *      s = r r / den (0 where den is not > 0).
 *   kinds 1 and 2: the Sampson error of the two constraints eps = (m_x - u m_z, m_y - v m_z), m = h x1h:
 *      m_i = h_{3i} x + h_{3i+1} y + h_{3i+2};   eps0 = m_x - u m_z, eps1 = m_y - v m_z;
 *      a = (h0 - u h6, h1 - u h7), b = (h3 - v h6, h4 - v h7), mm = m_z m_z;
 *      A = (a0 a0 + a1 a1) + mm, B = a0 b0 + a1 b1, D = (b0 b0 + b1 b1) + mm, det = A D - B B;
 *      s = ((D (eps0 eps0) - (2 B) (eps0 eps1)) + A (eps1 eps1)) / det;   det <= 1e-30 or not a number: s = 1e30.
 *      Kind 2 additionally has s = 1e30 where m_z is not > 0, as the distance of relpose_rotation.h.
 *   For every kind e2 = min(max(s, 0), 1e30), and 1e30 where s is not a number.
 * A candidate is INVALID if its matrix has a non-finite entry or a Frobenius norm (the nine squares summed in order, fp32) below 1e-30
 *   -- the zero matrix the consensus kernels write for a degenerate problem: its stat = (FLT_MAX, 0, 0, 0), its resid row is 1e30, it
 *   is never picked and never supplies the scale.
 * SCALE.  B_c = the number of rows of pos with e2 <= tau^2; med_c = the element of 0-based rank B_c / 2 (integer division) of those
 *   residuals in ascending order -- EXACT: non-negative floats order as their bit patterns, and the element is found by bisection
 *   over the bits, one count per bit, for all candidates at once (32 steps, no sort, no data-dependent loop);
 *   s2_c = med_c / 0.454936423 for codimension 1, med_c / 1.386294361 for codimension 2 (the medians of chi^2_1 and chi^2_2).
 *   sigma2 = sigma^2 if sigma is given; otherwise the minimum of s2_c over the valid candidates with B_c >= 16 (the lowest index
 *   among equals).  In both cases sigma2 <- min(max(sigma2, (tau / 1024)^2), 1e30).
 * CRITERION.  With L = 1.386294361 (ln 4) and dL_c = L d_c:
 *      thr_c = (outlier_cost - dL_c) sigma2,      I_c = the number of rows of pos with e2 < thr_c,      S_c = the sum of those e2,
 *      G_c = ((S_c / sigma2 + I_c dL_c) + (K - I_c) outlier_cost) + k_c log(4 K);
 *   S_c is summed per thread over its rows p = thread, thread + 256, ... in ascending order and then over the workgroup as
 *   csrc/block_sum.h does.  pick = the lowest index of the minimum G_c among the valid candidates.  With outlier_cost = 8 the inlier
 *   gates are 3.841 sigma2 (essential) and 5.227 sigma2 (homography, rotation).
 * Outputs:
 *   pick [n]          see above
 *   stat [n][C][4]    (G_c, I_c, thr_c, B_c)
 *   scale [n][2]      (sigma = sqrt(sigma2), the index of the candidate that supplied it, or -1 if it was given)
 *   resid [n][C][P]   (NULL = off) e2 of EVERY row, those outside pos included
 *   label [n][P]      (NULL = off) bit c set iff the row is in pos and e2 < thr_c -- what tells the points off a plane from those on it
 * A DEGENERATE problem -- K < 8, tau not > 0, no valid candidate, or no scale (sigma not given and no valid candidate with
 * B_c >= 16) -- gives pick = -1, every stat row (FLT_MAX, 0, 0, 0), scale = (0, -1), label = 0; resid is written as for any other.
 * LAYOUT.  grid n, 256 threads; a thread's rows (at most 7) and their residuals stay in registers; LDS holds the reduction buffer
 * (512 B) and nothing else; no matrix instruction, no scratch.
 * Argument checks before any launch: n <= 0, P < 8, C < 1, x1 / x2 / tau / models / kinds / pick / stat / scale NULL, a kind outside
 * {0, 1, 2}, outlier_cost not in (3 ln 4, 1e6] -> RP_EBADSHAPE; P > RP_SELECT_MAX_P, C > RP_SELECT_MAX_C -> RP_EUNSUPPORTED; x1 / x2
 * not 8-byte aligned, any other pointer not 4-byte aligned -> RP_EALIGN. */
int rp_model_select(const float* x1, const float* x2, const float* w, const float* tau, const float* sigma,
                    const float* models, const int* kinds /* HOST, [C] */, float outlier_cost,
                    int* pick, float* stat, float* scale, float* resid, int* label,
                    int P, int C, int n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_SELECT_H */
