/*
 * relpose_readout.h -- C ABI of librelpose_readout.so (gfx950 / MI355X): what the Essential Matrix Module matched.
 *
 * The EMM's dual-softmax attention A = softmax_rows(S) * softmax_cols(S) (vision_transformer.py:205-206) acts as soft
 * correspondences between the two images of a pair.  librelpose_hip.so only ever consumes A tile by tile (rp_emm_stats,
 * rp_emm_apply); this second, small library reads it out.  The reference has no counterpart (its epipolar visualiser works on the
 * materialised attention of the PyTorch module).
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 row-major tensors, 576 tokens per
 * image, head dim 64, and the memory contract -- every documented output element is written by every call, nothing else is, and no
 * result depends on what an output held before (no atomics, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_READOUT_H
#define RELPOSE_READOUT_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_readout_abi_version() returns the value
 * the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_READOUT_ABI_VERSION 1
int rp_readout_abi_version(void);

/* Matches of the EMM attention, per image z of a pair (partner z^1) and head h.  Inputs as for rp_emm_stats / rp_emm_apply: q / k point
 * at the first of the H*64 columns, rows (z*576 + i)*ld; S_z[i][j] = scale * q_{z^1}[i] . k_z[j] (rows i: tokens of the partner image,
 * columns j: tokens of image z); rlse / clse [Z][H][576] in natural-log units exactly as rp_emm_stats writes them.  Z must be even.
 *   A_z[i][j] = exp(2 S - rlse[i] - clse[j])        single != 0: A = exp(S - rlse[i]), clse unused (may be NULL) -- use_single_softmax
 * swap = 0: the owner is row i, reductions run over j and positions are those of token j;
 * swap = 1: the owner is column j, reductions run over i and positions are those of token i.
 *   idx [Z][H][576]     int: argmax over the other index of the EXPONENT 2 S - rlse - clse (defined even where A underflows to 0);
 *                       ties go to the lowest index
 *   stat [Z][H][576][4] (amax, mass, ex, ey): amax = A at idx; mass = sum of A over the other index; (ex, ey) = sum A * (n % 24, n / 24)
 *                       / mass over the other index's tokens n -- a soft-argmax in token-grid units (token n sits at column n % 24,
 *                       row n / 24); mass == 0: ex = ey = -1
 *   a_out (NULL = off)  the dense A, row-major [Z][H][576 i][576 j] whatever swap is (a visualisation path: 4 MB per image)
 * One wave owns 32 owner tokens and streams 32-token tiles of the other operand through LDS; the products are exact fp32
 * (v_mfma_f32_32x32x2_f32) and the two normalisers enter as a 33rd MFMA step, so the accumulators hold the exponent itself.
 * Argument checks before any launch: Z odd or <= 0, H <= 0, H*64 > ldq or ldk, a required pointer NULL -> RP_EBADSHAPE; a pointer not
 * 16-byte aligned or ld % 4 != 0 -> RP_EALIGN. */
int rp_emm_matches(const float* q, const float* k, const float* rlse, const float* clse, int* idx, float* stat, float* a_out, int Z,
                   int H, int ldq, int ldk, float scale, int swap, int single, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_READOUT_H */
