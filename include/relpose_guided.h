/*
 * relpose_guided.h -- C ABI of librelpose_guided.so (gfx950 / MI355X): the EMM's matches read again under a pose.
 *
 * rp_emm_matches (relpose_readout.h) takes the argmax of every row of the Essential Matrix Module's attention over all 576 tokens of the
 * other image.  rp_emm_guided_matches takes it over the tokens NEAR THE EPIPOLAR LINE that a given fundamental matrix assigns to the
 * owner -- classical guided matching on the dense score surface -- and reports how much of the attention's mass lies inside that band:
 * a score of the pose against the attention itself.  The reference has no counterpart.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, 576 tokens per
 * image, head dim 64, and the memory contract -- every documented output element is written by every call, nothing else is, and no
 * result depends on what an output held before (no atomics, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_GUIDED_H
#define RELPOSE_GUIDED_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_guided_abi_version() returns the value
 * the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_GUIDED_ABI_VERSION 1
int rp_guided_abi_version(void);

/* q, k, rlse, clse, Z, H, ldq, ldk, scale, swap, single: exactly as for rp_emm_matches -- image z's problem has rows i = tokens of the
 * partner image z^1 (q) and columns j = tokens of image z (k), the exponent is e = 2 S - rlse[i] - clse[j] (single != 0: S - rlse[i],
 * clse may be NULL), A = exp(e); swap = 0: the owner is row i and the other index is j, swap = 1: the owner is column j, the other i.
 *   F    [Z][9]  row-major, in token-grid units: row token i sits at r_i = (i % 24, i / 24, 1), column token j at c_j = (j % 24, j / 24, 1),
 *                and the epipolar constraint of image z's problem is c_j^T F_z r_i = 0.  Only the direction of F_z matters.
 *   band [Z]     half-width of the admitted band in token pitches, > 0 (+inf admits every pair with den > 0).  One pitch is one token on
 *                either axis: for an image with H != W the pitches differ in pixels, and the band is an ellipse-like region there.
 * Admission of the pair (i, j), the same for both values of swap, all in fp32 with fma(a, b, c) = a b + c rounded once, G = F_z 2^-k with
 * 2^(k-1) <= max|F_z| < 2^k (an exact scaling: nothing overflows, and a matrix of small integers stays exact), x = n % 24, y = n / 24:
 *   l  = G r_i:         lx = fma(G0, x, fma(G1, y, G2)),  ly = fma(G3, x, fma(G4, y, G5)),  lz = fma(G6, x, fma(G7, y, G8))
 *   m  = (G^T c_j)_xy:  mx = fma(G0, x, fma(G3, y, G6)),  my = fma(G1, x, fma(G4, y, G7))
 *   l2 = fma(lx, lx, ly ly),   m2 = fma(mx, mx, my my),   den = l2 + m2
 *   rho = fma(cx, lx, fma(cy, ly, lz))
 *   admitted  iff  not (den > 0)  or  rho rho <= (band band) den
 * -- division-free per pair, and in agreement with the Sampson distance of the solver libraries, which is 0 where den is 0: the pair is
 * admitted iff that distance is <= band^2.
 *   idx  [Z][H][576]     int: argmax of the exponent over the ADMITTED tokens of the other index, ties to the lowest index; -1 where none
 *                        is admitted (or no admitted exponent exceeds -inf)
 *   stat [Z][H][576][4]  (amax, bmass, mass, d2): amax = A at idx (0 at -1); bmass = sum of A over the admitted tokens; mass = sum of A
 *                        over all tokens of the other index; d2 = the Sampson distance of the chosen pair under G, in squared token
 *                        pitches (0 at -1).  bmass / mass is the share of the owner's attention that the pose explains.
 * A degenerate image z -- an F_z with a non-finite entry, an F_z that is all zero, or a band_z that is not > 0 (a NaN included) -- gives
 * idx = -1 and stat = 0 for all its owners; the other image of the pair is unaffected.  Nothing non-finite is written for finite inputs.
 * One wave owns 32 owner tokens and streams 32-token tiles of the other operand through LDS; the products are exact fp32
 * (v_mfma_f32_32x32x2_f32) and the two normalisers enter as a 33rd MFMA step, as in rp_emm_matches.
 * Argument checks before any launch: Z odd or <= 0, H <= 0, H*64 > ldq or ldk, a required pointer NULL -> RP_EBADSHAPE; q, k, rlse, clse,
 * idx or stat not 16-byte aligned, F or band not 4-byte aligned, or ld % 4 != 0 -> RP_EALIGN. */
int rp_emm_guided_matches(const float* q, const float* k, const float* rlse, const float* clse, const float* F, const float* band, int* idx,
                          float* stat, int Z, int H, int ldq, int ldk, float scale, int swap, int single, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_GUIDED_H */
