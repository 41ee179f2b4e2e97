// consensus.hip -- rp_eight_point_consensus: seeded hypothesise-and-verify in front of the eight-point solver (librelpose_consensus.so).
//
// Two launches; include/relpose_consensus.h states the sampler, the hypothesis, the score and the selection.
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major, one dimension), 256 threads.
//     stage    csrc/consensus_core.h: the rows of positive weight, COMPACTED into LDS in ascending order (four barriers; from there on no
//              thread talks to another).
//     solve    one lane, one hypothesis: Floyd's eight draws (the core), eight rows gathered from LDS, Hartley normalisation, the 8 x 9
//              row matrix in registers, its null vector by eight Householder reflections of the transpose (csrc/two_view.h: every loop
//              unrolled, every index static: no scratch), F = T2^T F^ T1, svd3x3_dev, the sign rule.
//     score    the core: the lane walks the K compacted rows (LDS broadcast reads) and sums the robust Sampson cost in a fixed order.
//   select_kernel       grid n, 256 threads: the core's lowest-index argmin of hyp_cost over the valid hypotheses, the Sampson distances at
//              the winner and w_out; the sums of stat by block_sum.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_E, by the second launch after the first wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../csrc/two_view.h"
#include "../csrc/consensus_core.h"
#include "../../include/relpose_consensus.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_CONSENSUS_MAX_P;
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel

// the eight-point solve of rp_eight_point (iters = 0, unit weights) on eight rows; false: INVALID
RP_DEV bool minimal_solve(const float2 (&p1)[8], const float2 (&p2)[8], float (&e)[9]) {
  float c1x, c1y, s1, c2x, c2y, s2;
  if (!normalise(p1, c1x, c1y, s1) || !normalise(p2, c2x, c2y, s2)) return false;
  // A[k] = x2^h (x) x1^h of row k: the k-th COLUMN of the 9 x 8 transpose
  Mat8x9 m;
  float (&A)[8][9] = m.a;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float ax = (p1[k].x - c1x) * s1, ay = (p1[k].y - c1y) * s1, bx = (p2[k].x - c2x) * s2, by = (p2[k].y - c2y) * s2;
    A[k][0] = bx * ax; A[k][1] = bx * ay; A[k][2] = bx;
    A[k][3] = by * ax; A[k][4] = by * ay; A[k][5] = by;
    A[k][6] = ax;      A[k][7] = ay;      A[k][8] = 1.f;
  }
  float f[9];
  null_vector_8x9(m, f);
  // F = T2^T F^ T1, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
  float G[9], F[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[3 * i] = f[3 * i] * s1;
    G[3 * i + 1] = f[3 * i + 1] * s1;
    G[3 * i + 2] = f[3 * i + 2] - s1 * (c1x * f[3 * i] + c1y * f[3 * i + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = s2 * G[j];
    F[3 + j] = s2 * G[3 + j];
    F[6 + j] = G[6 + j] - s2 * (c2x * G[j] + c2y * G[3 + j]);
  }
  float u[3][3], sv[3], v[3][3];
  svd3x3_dev(F, u, sv, v);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) e[3 * r + c] = u[0][r] * v[0][c] + u[1][r] * v[1][c];
  const bool ok = all_finite(e);
  sign_rule(e);
  return ok;
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_E, float* hyp_cost, int* samples, int P, int M, int chunks) {
  __shared__ ConsensusRows<MAXP> sm;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + threadIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const int K = consensus_stage(sm, X1, X2, w ? w + b * P : nullptr, P);
  if (m >= M) return;                               // (behind the last barrier)
  uint32_t c[8];
  consensus_sample(sm, seed, b, m, M, K, samples, c);
  // ---- solve and score
  const float ta = tau[b], tau2 = ta * ta;
  float e[9], cost = FLT_MAX;
  bool valid = K >= 8 && ta > 0.f;
  if (valid) {
    float2 p1[8], p2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      p1[k] = sm.a[c[k]];
      p2[k] = sm.b[c[k]];
    }
    valid = minimal_solve(p1, p2, e);
  }
  if (valid) {
    cost = consensus_cost(sm, e, K, tau2, SampsonDistance());
    valid = cost < FLT_MAX;                         // (false for a NaN, too)
  }
  if (!valid) {
    cost = FLT_MAX;
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = 0.f;
  }
  float* HE = hyp_E + (b * M + m) * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) HE[i] = e[i];
  hyp_cost[b * M + m] = cost;
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ hyp_E,
                                                     const float* __restrict__ hyp_cost, float* E, int* best, float* stat, float* w_out,
                                                     int P, int M) {
  __shared__ float red[2][NW][RED];
  __shared__ float bc[NT];
  __shared__ int bi[NT];
  const long long b = blockIdx.x;
  const float* HC = hyp_cost + b * M;
  float e[9], s4[4];
  const int win = consensus_select(bc, bi, reinterpret_cast<const float2*>(x1) + b * P, reinterpret_cast<const float2*>(x2) + b * P,
                                   w ? w + b * P : nullptr, w_out ? w_out + b * P : nullptr, HC, hyp_E + b * M * 9, M, P, tau[b],
                                   SampsonDistance(), e, s4);
  int phase = 0;
  block_sum(s4, red, phase);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) E[b * 9 + i] = e[i];
    best[b] = win;
    stat[b * 4] = win >= 0 ? HC[win] : 0.f;
    stat[b * 4 + 1] = win >= 0 ? s4[1] / s4[0] : 0.f;
    stat[b * 4 + 2] = s4[3];
    stat[b * 4 + 3] = s4[2];
  }
}

}  // namespace

extern "C" int rp_consensus_abi_version(void) { return RP_CONSENSUS_ABI_VERSION; }

extern "C" int rp_eight_point_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed, float* E, int* best,
                                        float* stat, float* w_out, float* hyp_E, float* hyp_cost, int* samples, int P, int M, int n,
                                        void* stream) {
  return consensus_launch<8, RP_CONSENSUS_MAX_P, RP_CONSENSUS_MAX_M, hypothesis_kernel, select_kernel>(
      x1, x2, w, tau, seed, E, best, stat, w_out, hyp_E, hyp_cost, samples, P, M, n, stream);
}
