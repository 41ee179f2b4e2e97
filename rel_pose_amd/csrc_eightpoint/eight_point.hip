// eight_point.hip -- rp_eight_point: batched weighted, normalised eight-point solver with Cauchy re-weighting (librelpose_eightpoint.so).
//
// One workgroup of 256 threads per problem, the whole iteration (iters + 1 solves) in one launch.  Per solve:
//   pass A   weights (base weight, from the second solve on divided by 1 + Sampson distance / tau^2), their sum, the count of positive
//            ones and the weighted sums of x - x_0 in both images: one six-value reduction
//   pass B   the weighted mean distance from the centroid in both images: one two-value reduction
//   pass C   the rows sqrt(w) (x2^h (x) x1^h) of the normalised points, written as NINE COLUMNS into LDS, col[j][row]: thread t owns the
//            rows t, t + 256, .. (at most 7) of every column for the rest of the solve, lanes read and write stride 1 (no bank conflict)
//   Jacobi   one-sided (Hestenes) on the columns: for every pair (p, q) in the cyclic order (0,1), (0,2), .. (7,8) the three sums
//            alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q in ONE fused reduction, from which every thread derives the same (c, s)
//            -- the formulas and the relative skip threshold of svd3x3_dev -- and rotates its own rows, held in registers since the
//            sums; threads 0..8 rotate the rows of V (9 x 9, LDS).  One barrier per rotation: the reduction buffer is double buffered.
//            SWEEPS = 9 sweeps, fixed: in the float32 restatement of this arithmetic (tests/_eightpoint_ref.py) E stops changing after
//            at most 7 sweeps over P = 8 .. 1728, with and without weights; plus two.
//   finish   column norms = singular values (one nine-value reduction); the column of V that belongs to the smallest is F^;
//            F = T2^T F^ T1; svd3x3_dev; E = u0 v0^T + u1 v1^T; the sign rule.  Every thread computes this redundantly (it needs E for
//            the next round's Sampson distances), thread 0 stores.
// Reductions (csrc/block_sum.h): within a wave by xor shuffles, across the four waves through LDS, summed by every thread in the same fixed
// order -- (alpha, beta, gamma) are bit-identical in all 256 threads, so the skip decision and (c, s) are uniform and every result is
// bit-identical from call to call.  No atomics, no workspace; nothing is read from an output.
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../csrc/two_view.h"
#include "../../include/relpose_eightpoint.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_EIGHTPOINT_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows of a column one thread owns: 7
constexpr int SWEEPS = 9;
constexpr int RED = 12;                              // floats per wave in the reduction buffer (>= 9)
constexpr float MIN_SCALE = 1e-30f;                  // a weighted mean distance below this counts as 0

struct Smem {
  float col[9][MAXP];          // 62 208 B
  float red[2][NW][RED];
  float V[9][9];               // V[column][row]
};

__global__ __launch_bounds__(NT) void eight_point_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                          const float* __restrict__ w, const float* __restrict__ tau, float* E,
                                                          float* stat, float* w_out, int P, int iters) {
  __shared__ Smem sm;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
  const float tau2 = iters > 0 ? tau[b] * tau[b] : 1.f;
  const float2 o1 = X1[0], o2 = X2[0];            // the pivots of the two centroids
  float e[9], st[4];
  int phase = 0;
#pragma unroll 1
  for (int k = 0; k <= iters; ++k) {
    // ---- pass A: the weights of this solve (kept in col[8] until pass C) and their first moments
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = tid; r < P; r += NT) {
      const float2 a = X1[r], c = X2[r];
      float wt = W ? fmaxf(W[r], 0.f) : 1.f;
      if (k > 0) {
        const float d = sampson(e, a, c);
        wt = d > 0.f ? wt / (1.f + d / tau2) : wt;
      }
      sm.col[8][r] = wt;
      acc[0] += wt;
      acc[1] += wt > 0.f ? 1.f : 0.f;
      acc[2] += wt * (a.x - o1.x);
      acc[3] += wt * (a.y - o1.y);
      acc[4] += wt * (c.x - o2.x);
      acc[5] += wt * (c.y - o2.y);
    }
    block_sum(acc, sm.red, phase);
    const float wsum = acc[0];
    bool degenerate = acc[1] < 8.f;                // (uniform: every thread holds the same sums)
    float c1x = 0.f, c1y = 0.f, c2x = 0.f, c2y = 0.f, s1 = 0.f, s2 = 0.f;
    if (!degenerate) {
      c1x = o1.x + acc[2] / wsum; c1y = o1.y + acc[3] / wsum;
      c2x = o2.x + acc[4] / wsum; c2y = o2.y + acc[5] / wsum;
      // ---- pass B: the weighted mean distances
      float m[2] = {0.f, 0.f};
      for (int r = tid; r < P; r += NT) {
        const float2 a = X1[r], c = X2[r];
        const float wt = sm.col[8][r];
        const float ax = a.x - c1x, ay = a.y - c1y, bx = c.x - c2x, by = c.y - c2y;
        m[0] += wt * sqrtf(ax * ax + ay * ay);
        m[1] += wt * sqrtf(bx * bx + by * by);
      }
      block_sum(m, sm.red, phase);
      const float m1 = m[0] / wsum, m2 = m[1] / wsum;
      degenerate = !(m1 >= MIN_SCALE) || !(m2 >= MIN_SCALE);
      if (!degenerate) {
        s1 = sqrtf(2.f) / m1;
        s2 = sqrtf(2.f) / m2;
      }
    }
    if (degenerate) {
#pragma unroll
      for (int i = 0; i < 9; ++i) e[i] = 0.f;
      st[0] = st[1] = st[2] = 0.f;
      st[3] = wsum;
      if (WO)
        for (int r = tid; r < P; r += NT) WO[r] = sm.col[8][r];
      break;
    }
    // ---- pass C: the nine columns; V = I
    for (int r = tid; r < P; r += NT) {
      const float2 a = X1[r], c = X2[r];
      const float wt = sm.col[8][r];
      if (WO && k == iters) WO[r] = wt;
      const float q = sqrtf(wt);
      const float ax = (a.x - c1x) * s1, ay = (a.y - c1y) * s1, bx = (c.x - c2x) * s2, by = (c.y - c2y) * s2;
      sm.col[0][r] = q * (bx * ax); sm.col[1][r] = q * (bx * ay); sm.col[2][r] = q * bx;
      sm.col[3][r] = q * (by * ax); sm.col[4][r] = q * (by * ay); sm.col[5][r] = q * by;
      sm.col[6][r] = q * ax;        sm.col[7][r] = q * ay;        sm.col[8][r] = q;
    }
    if (tid < 81) sm.V[tid / 9][tid % 9] = tid / 9 == tid % 9 ? 1.f : 0.f;      // (visible to threads 0..8 behind the first barrier below)
    // ---- one-sided Jacobi
#pragma unroll 1
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
#pragma unroll 1
      for (int p = 0; p < 8; ++p) {
#pragma unroll 1
        for (int q = p + 1; q < 9; ++q) {
          float xr[ROWS], yr[ROWS], g[3] = {0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < ROWS; ++i) {
            const int r = tid + i * NT;
            xr[i] = r < P ? sm.col[p][r] : 0.f;
            yr[i] = r < P ? sm.col[q][r] : 0.f;
            g[0] += xr[i] * xr[i];
            g[1] += yr[i] * yr[i];
            g[2] += xr[i] * yr[i];
          }
          block_sum(g, sm.red, phase);
          const float al = g[0], be = g[1], ga = g[2];
          if (fabsf(ga) > 1e-12f * sqrtf(al * be) && ga != 0.f) {
            const float zeta = (be - al) / (2.f * ga);
            const float t = copysignf(1.f, zeta) / (fabsf(zeta) + sqrtf(1.f + zeta * zeta));
            const float c = 1.f / sqrtf(1.f + t * t), s = c * t;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
              const int r = tid + i * NT;
              if (r < P) {
                rot(xr[i], yr[i], c, s);
                sm.col[p][r] = xr[i];
                sm.col[q][r] = yr[i];
              }
            }
            if (tid < 9) rot(sm.V[p][tid], sm.V[q][tid], c, s);
          }
        }
      }
    }
    // ---- singular values; the null vector
    float sg2[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) sg2[j] = 0.f;
    for (int r = tid; r < P; r += NT) {
#pragma unroll
      for (int j = 0; j < 9; ++j) sg2[j] += sm.col[j][r] * sm.col[j][r];
    }
    block_sum(sg2, sm.red, phase);                  // (its barrier also publishes V)
    int jmin = 0;
    float smax = sg2[0];
#pragma unroll
    for (int j = 1; j < 9; ++j) {
      jmin = sg2[j] < sg2[jmin] ? j : jmin;
      smax = fmaxf(smax, sg2[j]);
    }
    float smin = 0.f, snext = 3.0e38f;             // smallest, second smallest
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      smin = j == jmin ? sg2[j] : smin;
      snext = (j != jmin && sg2[j] < snext) ? sg2[j] : snext;
    }
    float f[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = sm.V[jmin][i];
    // ---- F = T2^T F^ T1, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
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
#pragma unroll
    for (int i = 1; i < 9; ++i)
      if (fabsf(e[i]) > big) { big = fabsf(e[i]); lead = e[i]; }
    if (lead < 0.f) {
#pragma unroll
      for (int i = 0; i < 9; ++i) e[i] = -e[i];
    }
    const float inv = smax > 0.f ? 1.f / sqrtf(smax) : 0.f;
    st[0] = sqrtf(smin) * inv;
    st[1] = sqrtf(snext) * inv;
    st[2] = sv[0] > 0.f ? sv[1] / sv[0] : 0.f;
    st[3] = wsum;
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) E[b * 9 + i] = e[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) stat[b * 4 + i] = st[i];
  }
}

}  // namespace

extern "C" int rp_eightpoint_abi_version(void) { return RP_EIGHTPOINT_ABI_VERSION; }

extern "C" int rp_eight_point(const float* x1, const float* x2, const float* w, const float* tau, float* E, float* stat, float* w_out,
                              int P, int iters, int n, void* stream) {
  if (n <= 0 || P < 8 || iters < 0 || !x1 || !x2 || !E || !stat || (!tau && iters > 0)) return RP_EBADSHAPE;
  if (P > RP_EIGHTPOINT_MAX_P || iters > RP_EIGHTPOINT_MAX_ITERS) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)E | (uintptr_t)stat | (uintptr_t)w_out) & 3) return RP_EALIGN;
  hipLaunchKernelGGL(eight_point_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, x1, x2, w, tau, E, stat, w_out, P, iters);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
