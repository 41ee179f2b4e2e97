/*
 * relpose_submatch.h -- C ABI of librelpose_submatch.so (gfx950 / MI355X): where, between the token centres, a match of the Essential
 * Matrix Module lies.
 *
 * rp_emm_matches (relpose_readout.h) reduces a row of the EMM's attention to its argmax token and a soft-argmax over the WHOLE row.  The
 * first is quantised to the token pitch, the second is useless for geometry where the row has more than one mode.  This sixth, small
 * library localises the peak on the score surface around the argmax: a soft-argmax over a small window and the vertex of the parabola
 * through the exponents of the argmax and its neighbours, per axis.  Neither estimator dominates the other, so both are
 * written and the host chooses.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, 576 tokens per
 * image, head dim 64, and the memory contract -- every documented output element is written by every call, nothing else is, and no
 * result depends on what an output held before (no atomics, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_SUBMATCH_H
#define RELPOSE_SUBMATCH_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_submatch_abi_version() returns the value
 * the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_SUBMATCH_ABI_VERSION 1
int rp_submatch_abi_version(void);

/* Sub-token localisation of the matches of the EMM attention, per image z of a pair (partner z^1), head h and owner token.
 * q, k, rlse, clse, Z, H, ldq, ldk, scale, swap, single exactly as for rp_emm_matches: S_z[i][j] = scale * q_{z^1}[i] . k_z[j] (rows i:
 * tokens of the partner image, columns j: tokens of image z), the exponent e[i][j] = 2 S - rlse[i] - clse[j]; single != 0:
 * e = S - rlse[i], clse unused (may be NULL).  swap = 0: the owner is row i, the other index n is j; swap = 1: the owner is column j, the
 * other index n is i.
 *   idx [Z][H][576] int   INPUT: the window centre n0 per owner, normally what rp_emm_matches wrote.  The argmax is not repeated here, so
 *                         ties and last-bit differences between the two kernels' scores cannot move the window.
 * Token n sits at grid position (n % 24, n / 24); (x0, y0) is that of n0.  The WINDOW is the set of tokens (x, y) with |x - x0| <= radius
 * and |y - y0| <= radius inside the 24 x 24 grid; radius is 1 or 2.
 * ARITHMETIC, all fp32.  dot = the 64 products q_d k_d added in the order d = 0 .. 63 by fused multiply-adds, starting from 0;
 *   e = fma(m scale, dot, -lse_owner) - lse_other, m = 2 (single: 1), a normaliser the single softmax does not apply counted as 0.
 *   e_max = the largest e of the window, u = exp2((e - e_max) log2(e)), all sums over the window in one fixed order:
 *   win [Z][H][576][4] = (wx, wy, wmass, wvar)
 *     wx = x0 + sum u (x - x0) / sum u, wy = y0 + sum u (y - y0) / sum u   in token-grid units; defined even where A underflows to 0
 *     wmass = sum exp2(e log2(e))          the share of the row the peak holds is wmass / mass of rp_emm_matches
 *     wvar = sum u ((x - wx)^2 + (y - wy)^2) / sum u
 *   quad [Z][H][576][4] = (px, py, cx, cy)
 *     along x, with a, b, c the exponents at (x0 - 1, y0), (x0, y0), (x0 + 1, y0):  cx = (b - a) + (b - c)  (= 2b - a - c);
 *     px = x0 + min(max(0.5 (c - a) / cx, -0.5), 0.5) where both neighbours are inside the grid and cx > 0, else px = x0;
 *     cx = 0 where a neighbour is outside the grid.  py, cy likewise along y.
 * An idx outside 0 .. 575 makes its owner INVALID: win = (-1, -1, 0, 0), quad = (-1, -1, 0, 0), and NOTHING IS READ THROUGH THAT INDEX.
 * Nothing non-finite is written for finite inputs.
 * One group of 32 lanes per owner (two owners per wave, eight per workgroup of 256 threads): a lane takes one window slot, loads its
 * token's 64 features as sixteen 16-byte loads and forms the dot product; the sums run through wave shuffles inside the group.  A slot
 * outside the grid, and every slot of an invalid owner, contributes exactly 0 and forms no address.
 * Argument checks before any launch: Z odd or <= 0, H <= 0, H*64 > ldq or ldk, a required pointer NULL (q, k, rlse, clse unless single,
 * idx, win, quad) -> RP_EBADSHAPE; radius outside 1 .. 2 (or more than 2^31 - 1 workgroups, 72 Z H) -> RP_EUNSUPPORTED; q, k, rlse, clse,
 * win or quad not 16-byte aligned, idx not 4-byte aligned, ld % 4 != 0 -> RP_EALIGN. */
int rp_emm_submatch(const float* q, const float* k, const float* rlse, const float* clse, const int* idx, float* win, float* quad, int Z,
                    int H, int ldq, int ldk, float scale, int swap, int single, int radius, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_SUBMATCH_H */
