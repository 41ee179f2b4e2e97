/*
 * relpose_conv5x5.h -- C ABI of librelpose_conv5x5.so (gfx950 / MI355X): the exact-fp32 input gradient of the two valid 5x5
 * convolutions of extractor_final_conv (conv2 192 -> 192 and downsample.0 128 -> 192, 28 x 28 -> 24 x 24).
 *
 * A tenth library with one kernel: the main library's surface (include/relpose_hip.h) stays what it was.
 *
 * The conventions of relpose_hip.h hold unchanged: device pointers owned by the caller, no allocation, no global state, `stream` is
 * a hipStream_t, return value 0 / RP_E* (<0, the codes of relpose_hip.h) / hipError_t (>0), fp32 tensors, and the memory contract --
 * every documented output element is written by every call, nothing else is, and no result depends on what an output held before
 * (no atomics, no split-K, no workspace): results are bit-identical from call to call.
 */
#ifndef RELPOSE_CONV5X5_H
#define RELPOSE_CONV5X5_H

#include "relpose_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point of this header is added, removed or changes its arguments; rp_conv5x5_abi_version() returns the
 * value the library was COMPILED with, so the binding rejects a stale .so at load time */
#define RP_CONV5X5_ABI_VERSION 1
int rp_conv5x5_abi_version(void);

/* dx[n][y][x][ci] = (res ? res[n][y][x][ci] : 0) + sum over r, s in 0..4 and co in 0..191 of dy[n][y-r][x-s][co] * w[co][r][s][ci]
 * with dy taken as zero outside 0..23 in either direction:
 *   dy  [N][24][24][192]   NHWC, the gradient of the convolution's output
 *   w   [192][5][5][CI]    the memory of the channels-last forward weight [192][CI][5][5], read as it lies (no filter preparation)
 *   res [N][28][28][CI]    (NULL = off) added in the epilogue; may not alias dx
 *   dx  [N][28][28][CI]    NHWC, every element written
 * CI is 192 or 128, N any value >= 1.  One launch; a workgroup owns ONE pixel (y, x) of dx for a block of 128 images and all CI
 * channels and walks only the taps that fall inside dy for that pixel, so no product with a padding zero is ever formed; the sum
 * over (co, r, s) of one element is formed in one fixed order.
 * Argument checks before any launch: N < 1, dy / w / dx NULL -> RP_EBADSHAPE; CI not 128 or 192 -> RP_EUNSUPPORTED;
 * any pointer not 16-byte aligned -> RP_EALIGN. */
int rp_conv5x5_dgrad_f32(const float* dy, const float* w, float* dx, int N, int CI, const float* res, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_CONV5X5_H */
