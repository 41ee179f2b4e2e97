// block_sum.h -- the workgroup reduction of the six two-view geometry libraries (eight-point, refinement, consensus, five-point,
// homography, structure; the select kernels of csrc/consensus_core.h reduce through it too): sums over a workgroup of 256 threads,
// delivered to EVERY thread with the same bits, one barrier per call.
//
// Within a wave by xor shuffles (wave_sum), across the four waves through an LDS buffer the caller owns, summed by every thread in the
// same fixed order ((w0 + w1) + w2) + w3 -- so whatever a kernel derives from the sums (a rotation, a skip decision, a 5 x 5 solve) is
// uniform without a broadcast, and bit-identical from call to call.
#pragma once
#include "common.h"

constexpr int BLOCK_SUM_THREADS = 256;
constexpr int BLOCK_SUM_WAVES = BLOCK_SUM_THREADS / 64;

// sums of v[0..N-1] over the workgroup, in every thread.  red: [2][4][RED] floats of LDS, RED >= N.  One barrier per call: `phase`
// alternates between the two halves of the buffer, and whoever writes a half again (two calls later) has passed the barrier of the call
// in between, which every thread reaches only after its reads of this call.
template <int N, int RED>
RP_DEV void block_sum(float (&v)[N], float (&red)[2][BLOCK_SUM_WAVES][RED], int& phase) {
  static_assert(N <= RED, "block_sum: the reduction buffer is too narrow");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[phase][wave][i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[phase][0][i] + red[phase][1][i]) + red[phase][2][i]) + red[phase][3][i];
  phase ^= 1;
}
