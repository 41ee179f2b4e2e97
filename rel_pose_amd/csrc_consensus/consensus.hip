// consensus.hip -- rp_eight_point_consensus: seeded hypothesise-and-verify in front of the eight-point solver (librelpose_consensus.so).
//
// Two launches; include/relpose_consensus.h states the sampler, the hypothesis, the score and the selection.
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major, one dimension), 256 threads.
//     stage    the flags "weight positive" of all rows go to LDS with coalesced loads; thread t then counts the flags of the CONTIGUOUS
//              rows t * per .. t * per + per - 1 (per = ceil(P / 256) <= 7), the counts go to LDS, every thread reads them back in
//              thread order (an ordered prefix sum, no atomics) and writes the numbers of its rows of positive weight: pos, ascending.
//              Points and weights are then gathered through pos, COMPACTED, with loads that are coalesced up to the gaps.  Four
//              barriers; from there on no thread talks to another.
//     solve    one lane, one hypothesis: Floyd's eight draws, eight rows gathered from LDS, Hartley normalisation, the 8 x 9 row matrix
//              in registers, eight Householder reflections of its transpose (every loop unrolled, every index static: no scratch), the
//              null vector = the reflections applied to e_9, F = T2^T F^ T1, svd3x3_dev, the sign rule.
//     score    the lane walks the K compacted rows: every lane of the workgroup reads the SAME LDS address (a broadcast, no bank
//              conflict) and adds to its own sums in the same fixed order -- no reduction, no barrier.
//   select_kernel       grid n, 256 threads: the lowest-index argmin of hyp_cost over the valid hypotheses (a tree in LDS on (cost, index)),
//              the Sampson distances at the winner, w_out, and the sums of stat by block_sum.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_E, by the second launch after the first wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../../include/relpose_consensus.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_CONSENSUS_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread stages: 7
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel
constexpr float MIN_SCALE = 1e-30f;                  // a mean distance below this counts as 0
constexpr float FINITE = 3.0e38f;                    // |v| <= FINITE: v is a number

struct Rows {
  float2 a[MAXP], b[MAXP];     // the rows of positive weight, ascending: x1, x2
  float w[MAXP];
  int pos[MAXP];               // their row numbers
  int cnt[NT];
};                             // 42 496 B

RP_DEV uint32_t mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// Sampson distance of x1 <-> x2 under e (row-major), as csrc_eightpoint/eight_point.hip; 0 where the denominator is 0
RP_DEV float sampson(const float (&e)[9], float2 a, float2 b) {
  const float l2x = e[0] * a.x + e[1] * a.y + e[2], l2y = e[3] * a.x + e[4] * a.y + e[5], l2z = e[6] * a.x + e[7] * a.y + e[8];
  const float l1x = e[0] * b.x + e[3] * b.y + e[6], l1y = e[1] * b.x + e[4] * b.y + e[7];
  const float r = b.x * l2x + b.y * l2y + l2z;
  const float den = l2x * l2x + l2y * l2y + l1x * l1x + l1y * l1y;
  return den > 0.f ? r * r / den : 0.f;
}

// Hartley transform of eight points with unit weights about the pivot p[0]: centroid (cx, cy), scale s; false on a breakdown
RP_DEV bool normalise8(const float2 (&p)[8], float& cx, float& cy, float& s) {
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sx += p[k].x - p[0].x;
    sy += p[k].y - p[0].y;
  }
  cx = p[0].x + sx / 8.f;
  cy = p[0].y + sy / 8.f;
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float dx = p[k].x - cx, dy = p[k].y - cy;
    m += sqrtf(dx * dx + dy * dy);
  }
  m = m / 8.f;
  if (!(m >= MIN_SCALE)) return false;
  s = sqrtf(2.f) / m;
  return true;
}

// the eight-point solve of rp_eight_point (iters = 0, unit weights) on eight rows; false: INVALID
RP_DEV bool minimal_solve(const float2 (&p1)[8], const float2 (&p2)[8], float (&e)[9]) {
  float c1x, c1y, s1, c2x, c2y, s2;
  if (!normalise8(p1, c1x, c1y, s1) || !normalise8(p2, c2x, c2y, s2)) return false;
  // A[k] = x2^h (x) x1^h of row k: the k-th COLUMN of the 9 x 8 transpose
  float A[8][9];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float ax = (p1[k].x - c1x) * s1, ay = (p1[k].y - c1y) * s1, bx = (p2[k].x - c2x) * s2, by = (p2[k].y - c2y) * s2;
    A[k][0] = bx * ax; A[k][1] = bx * ay; A[k][2] = bx;
    A[k][3] = by * ax; A[k][4] = by * ay; A[k][5] = by;
    A[k][6] = ax;      A[k][7] = ay;      A[k][8] = 1.f;
  }
  // Householder QR of the transpose, column by column: H_j = I - beta_j v_j v_j^T zeroes column j below its diagonal; v_j stays in
  // A[j][j ..].  A zero column gets beta = 0, v = 0: no reflection.
  float beta[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float sig = 0.f;
#pragma unroll
    for (int i = j; i < 9; ++i) sig += A[j][i] * A[j][i];
    const float nrm = sqrtf(sig);
    const float den = sig + fabsf(A[j][j]) * nrm;
    beta[j] = den > 0.f ? 1.f / den : 0.f;
    A[j][j] += copysignf(nrm, A[j][j]);
#pragma unroll
    for (int k = j + 1; k < 8; ++k) {
      float t = 0.f;
#pragma unroll
      for (int i = j; i < 9; ++i) t += A[j][i] * A[k][i];
      t *= beta[j];
#pragma unroll
      for (int i = j; i < 9; ++i) A[k][i] -= t * A[j][i];
    }
  }
  // the null vector: the last column of Q = H_0 .. H_7
  float f[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = i == 8 ? 1.f : 0.f;
#pragma unroll
  for (int j = 7; j >= 0; --j) {
    float t = 0.f;
#pragma unroll
    for (int i = j; i < 9; ++i) t += A[j][i] * f[i];
    t *= beta[j];
#pragma unroll
    for (int i = j; i < 9; ++i) f[i] -= t * A[j][i];
  }
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
  float big = fabsf(e[0]), lead = e[0];
  bool ok = fabsf(e[0]) <= FINITE;
#pragma unroll
  for (int i = 1; i < 9; ++i) {
    ok = ok && fabsf(e[i]) <= FINITE;
    if (fabsf(e[i]) > big) { big = fabsf(e[i]); lead = e[i]; }
  }
  if (lead < 0.f) {
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = -e[i];
  }
  return ok;
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_E, float* hyp_cost, int* samples, int P, int M, int chunks) {
  __shared__ Rows sm;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + tid;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  // ---- stage: the flags of the rows (coalesced), the ordered prefix over contiguous runs of them, then the rows of positive weight
  for (int r = tid; r < P; r += NT) sm.pos[r] = (W ? fmaxf(W[r], 0.f) : 1.f) > 0.f ? 1 : 0;
  __syncthreads();
  const int per = (P + NT - 1) / NT;                // thread t numbers the rows t * per .. t * per + per - 1
  int flag[ROWS], mine = 0;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid * per + i;
    flag[i] = i < per && r < P ? sm.pos[r] : 0;     // (into registers: pos is overwritten below)
    mine += flag[i];
  }
  sm.cnt[tid] = mine;
  __syncthreads();
  int at = 0, K = 0;
  for (int t = 0; t < NT; ++t) {
    const int c = sm.cnt[t];
    K += c;
    at += t < tid ? c : 0;
  }
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    if (flag[i]) sm.pos[at++] = tid * per + i;      // (every flag was read before the barrier above)
  }
  __syncthreads();
  for (int j = tid; j < K; j += NT) {               // ascending rows: close to coalesced
    const int r = sm.pos[j];
    sm.a[j] = X1[r];
    sm.b[j] = X2[r];
    sm.w[j] = W ? W[r] : 1.f;
  }
  __syncthreads();
  if (m >= M) return;                               // (behind the last barrier)
  // ---- sample
  uint32_t c[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) c[k] = 0u;
  if (K >= 8) {
    const uint32_t s = mix(mix(seed + 0x9E3779B9u * (uint32_t)(b + 1)) ^ (uint32_t)m);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint32_t r = mix(s + 0x9E3779B9u * (uint32_t)(k + 1));
      const uint32_t j = (uint32_t)(K - 8 + k);
      const uint32_t t = (uint32_t)(((uint64_t)r * (uint64_t)(j + 1u)) >> 32);
      bool seen = false;
#pragma unroll
      for (int l = 0; l < k; ++l) seen = seen || c[l] == t;
      c[k] = seen ? j : t;
    }
  }
  if (samples) {
    int* S = samples + (b * M + m) * 8;
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = K >= 8 ? sm.pos[c[k]] : 0;
  }
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
    float acc = 0.f, wsum = 0.f;
    for (int j = 0; j < K; ++j) {
      const float wt = sm.w[j];
      const float d = sampson(e, sm.a[j], sm.b[j]);
      acc += wt * (tau2 * log1pf(d / tau2));
      wsum += wt;
    }
    cost = acc / wsum;
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
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
  const float* HC = hyp_cost + b * M;
  // ---- the lowest-index minimum among the valid hypotheses, and their number
  float lo = FLT_MAX, nvalid = 0.f;
  int arg = -1;
  for (int m = tid; m < M; m += NT) {
    const float c = HC[m];
    nvalid += c < FLT_MAX ? 1.f : 0.f;
    if (c < lo) { lo = c; arg = m; }               // (ascending m: the first of equal costs stays)
  }
  bc[tid] = lo;
  bi[tid] = arg;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const float c = bc[tid + s];
      const int i = bi[tid + s];
      if (i >= 0 && (c < bc[tid] || bi[tid] < 0 || (c == bc[tid] && i < bi[tid]))) { bc[tid] = c; bi[tid] = i; }
    }
    __syncthreads();
  }
  const int win = bi[0];
  float e[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) e[i] = win >= 0 ? hyp_E[(b * M + win) * 9 + i] : 0.f;
  const float ta = tau[b], tau2 = win >= 0 ? ta * ta : 1.f;
  // ---- the weights at the winner; sum of the weights, of those within tau, count of the positive ones, count of the valid hypotheses
  float s4[4] = {0.f, 0.f, 0.f, nvalid};
  for (int r = tid; r < P; r += NT) {
    const float wt = W ? fmaxf(W[r], 0.f) : 1.f;
    const float d = sampson(e, X1[r], X2[r]);
    s4[0] += wt;
    s4[1] += d <= tau2 ? wt : 0.f;
    s4[2] += wt > 0.f ? 1.f : 0.f;
    if (WO) WO[r] = win >= 0 ? wt / (1.f + d / tau2) : wt;
  }
  int phase = 0;
  block_sum(s4, red, phase);
  if (tid == 0) {
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
  if (n <= 0 || P < 8 || M < 1 || !x1 || !x2 || !tau || !E || !best || !stat || !hyp_E || !hyp_cost) return RP_EBADSHAPE;
  if (P > RP_CONSENSUS_MAX_P || M > RP_CONSENSUS_MAX_M) return RP_EUNSUPPORTED;
  const int chunks = (M + NT - 1) / NT;
  if ((long long)n * chunks > 2147483647LL) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)E | (uintptr_t)best | (uintptr_t)stat | (uintptr_t)w_out | (uintptr_t)hyp_E |
       (uintptr_t)hyp_cost | (uintptr_t)samples) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(hypothesis_kernel, dim3(n * chunks), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, (uint32_t)seed, hyp_E, hyp_cost,
                     samples, P, M, chunks);
  RP_CHECK_LAUNCH();
  hipLaunchKernelGGL(select_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, hyp_E, hyp_cost, E, best, stat, w_out, P, M);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
