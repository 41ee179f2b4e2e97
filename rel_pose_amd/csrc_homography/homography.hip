// homography.hip -- the plane-induced homography behind the matches (librelpose_homography.so): rp_homography_consensus,
// rp_homography_refine, rp_pose_from_homography.  include/relpose_homography.h states all arithmetic.
//
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major), 256 threads: the staging of csrc/consensus_core.h (flags, ordered
//              prefix, compacted rows in LDS; four barriers), then one lane per hypothesis: Floyd's four draws (the core), Hartley
//              normalisation, the 8 x 9 DLT matrix in registers, its null vector by eight Householder reflections of the transpose
//              (csrc/two_view.h: every loop unrolled, every index static: no scratch), H = T2^-1 H^ T1, Frobenius norm 1, the sign rule;
//              the lane then walks the K compacted rows (the core's cost loop, LDS broadcast reads) and sums the robust transfer cost in
//              a fixed order.
//   select_kernel       grid n, 256 threads: the core's lowest-index argmin of hyp_cost (a tree in LDS), w_out and stat at the winner.
//   refine_kernel       grid n, 256 threads: Levenberg-Marquardt over the eight generators of sl(3).  A thread's rows (at most 7) stay in
//              registers; per iteration ONE fused 44-value reduction (36 of the normal matrix, 8 of the gradient), the 8 x 8 Cholesky
//              (csrc/two_view.h) and the retraction redundantly in every thread, one one-value reduction for the trial cost: two barriers.
//   decompose_kernel    grid n, 256 threads: every thread decomposes H redundantly (svd3x3_dev, closed form); one reduction fixes the sign
//              of H, one fused eight-value reduction gives visibility and Sampson cost of the four candidates.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_H, by select_kernel after hypothesis_kernel wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../csrc/two_view.h"
#include "../csrc/consensus_core.h"
#include "../../include/relpose_homography.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_HOMOGRAPHY_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread stages / owns: 7
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel
constexpr int NPAR = 8;                              // degrees of freedom of H
constexpr int LMRED = NPAR * (NPAR + 1) / 2 + NPAR;  // 44: the upper triangle of the normal matrix and the gradient
constexpr int DRED = 8;                              // decompose_kernel: (visibility, Sampson cost) of four candidates
constexpr float DEN_MIN = 1e-30f, D_MAX = 1e30f;     // the clamps of the transfer distance
constexpr float LAMBDA0 = 1e-3f, LAMBDA_MIN = 1e-7f, LAMBDA_MAX = 1e7f;
constexpr float ROTATION_GAP = 1e-4f;                // sigma_1 - sigma_3 below this: pure rotation
constexpr float RANK_MIN = 1e-6f;                    // s_2 <= RANK_MIN s_1: H has no middle singular value to scale by

// squared one-sided transfer distance |pi(H x1h) - x2|^2, the denominator clamped below and the value above: independent of the sign of h
RP_DEV float transfer(const float (&h)[9], float2 a, float2 b) {
  const float m0 = h[0] * a.x + h[1] * a.y + h[2], m1 = h[3] * a.x + h[4] * a.y + h[5], m2 = h[6] * a.x + h[7] * a.y + h[8];
  const float ex = m0 - b.x * m2, ey = m1 - b.y * m2;
  return fminf((ex * ex + ey * ey) / fmaxf(m2 * m2, DEN_MIN), D_MAX);
}

// the distance of this library
struct TransferDistance {
  RP_DEV float operator()(const float (&h)[9], float2 a, float2 b) const { return transfer(h, a, b); }
};

// h / |h|_F; false if the norm is below RP_MIN_SCALE or not a number (h is then left as it is)
RP_DEV bool frob_unit(float (&h)[9]) {
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) ss += h[i] * h[i];
  const float nrm = sqrtf(ss);
  if (!(nrm >= RP_MIN_SCALE) || !(nrm <= RP_FINITE)) return false;
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = h[i] / nrm;
  return true;
}

// the four-point DLT on four rows; false: INVALID
RP_DEV bool minimal_solve(const float2 (&p1)[4], const float2 (&p2)[4], float (&h)[9]) {
  float c1x, c1y, s1, c2x, c2y, s2;
  if (!normalise(p1, c1x, c1y, s1) || !normalise(p2, c2x, c2y, s2)) return false;
  // A[j] = row j of the 8 x 9 matrix: the j-th COLUMN of the 9 x 8 transpose
  Mat8x9 m;
  float (&A)[8][9] = m.a;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ax = (p1[k].x - c1x) * s1, ay = (p1[k].y - c1y) * s1, bx = (p2[k].x - c2x) * s2, by = (p2[k].y - c2y) * s2;
    A[2 * k][0] = ax;  A[2 * k][1] = ay;  A[2 * k][2] = 1.f;
    A[2 * k][3] = 0.f; A[2 * k][4] = 0.f; A[2 * k][5] = 0.f;
    A[2 * k][6] = -bx * ax; A[2 * k][7] = -bx * ay; A[2 * k][8] = -bx;
    A[2 * k + 1][0] = 0.f; A[2 * k + 1][1] = 0.f; A[2 * k + 1][2] = 0.f;
    A[2 * k + 1][3] = ax;  A[2 * k + 1][4] = ay;  A[2 * k + 1][5] = 1.f;
    A[2 * k + 1][6] = -by * ax; A[2 * k + 1][7] = -by * ay; A[2 * k + 1][8] = -by;
  }
  float f[9];
  null_vector_8x9(m, f);
  // H = T2^-1 H^ T1, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], T^-1 = [[1/s, 0, cx], [0, 1/s, cy], [0, 0, 1]]
  float G[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    G[3 * i] = f[3 * i] * s1;
    G[3 * i + 1] = f[3 * i + 1] * s1;
    G[3 * i + 2] = f[3 * i + 2] - s1 * (c1x * f[3 * i] + c1y * f[3 * i + 1]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    h[j] = G[j] / s2 + c2x * G[6 + j];
    h[3 + j] = G[3 + j] / s2 + c2y * G[6 + j];
    h[6 + j] = G[6 + j];
  }
  if (!all_finite(h) || !frob_unit(h)) return false;
  sign_rule(h);
  return true;
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_H, float* hyp_cost, int* samples, int P, int M, int chunks) {
  __shared__ ConsensusRows<MAXP> sm;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + threadIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const int K = consensus_stage(sm, X1, X2, w ? w + b * P : nullptr, P);
  if (m >= M) return;                               // (behind the last barrier)
  uint32_t c[4];
  consensus_sample(sm, seed, b, m, M, K, samples, c);
  // ---- solve and score
  const float ta = tau[b], tau2 = ta * ta;
  float h[9], cost = FLT_MAX;
  bool valid = K >= 4 && ta > 0.f;
  if (valid) {
    float2 p1[4], p2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p1[k] = sm.a[c[k]];
      p2[k] = sm.b[c[k]];
    }
    valid = minimal_solve(p1, p2, h);
  }
  if (valid) {
    cost = consensus_cost(sm, h, K, tau2, TransferDistance());
    valid = cost < FLT_MAX;                         // (false for a NaN, too)
  }
  if (!valid) {
    cost = FLT_MAX;
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = 0.f;
  }
  float* HH = hyp_H + (b * M + m) * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) HH[i] = h[i];
  hyp_cost[b * M + m] = cost;
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ hyp_H,
                                                     const float* __restrict__ hyp_cost, float* H, int* best, float* stat, float* w_out,
                                                     int P, int M) {
  __shared__ float red[2][NW][RED];
  __shared__ float bc[NT];
  __shared__ int bi[NT];
  const long long b = blockIdx.x;
  const float* HC = hyp_cost + b * M;
  float h[9], s4[4];
  const int win = consensus_select(bc, bi, reinterpret_cast<const float2*>(x1) + b * P, reinterpret_cast<const float2*>(x2) + b * P,
                                   w ? w + b * P : nullptr, w_out ? w_out + b * P : nullptr, HC, hyp_H + b * M * 9, M, P, tau[b],
                                   TransferDistance(), h, s4);
  int phase = 0;
  block_sum(s4, red, phase);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[b * 9 + i] = h[i];
    best[b] = win;
    stat[b * 4] = win >= 0 ? HC[win] : 0.f;
    stat[b * 4 + 1] = win >= 0 ? s4[1] / s4[0] : 0.f;
    stat[b * 4 + 2] = s4[3];
    stat[b * 4 + 3] = s4[2];
  }
}

// the robust transfer cost term of one row
RP_DEV float cost_term(const float (&h)[9], float ax, float ay, float bx, float by, float wt, float tau2) {
  const float d = transfer(h, make_float2(ax, ay), make_float2(bx, by));
  return wt * (tau2 * log1pf(d / tau2));
}

__global__ __launch_bounds__(NT) void refine_kernel(const float* H0, const float* __restrict__ x1, const float* __restrict__ x2,
                                                     const float* __restrict__ w, const float* __restrict__ tau, int iters, float* H,
                                                     float* stat, float* w_out, int P) {
  __shared__ float red[2][NW][LMRED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  float* WO = w_out ? w_out + b * P : nullptr;
  // ---- the thread's rows, once
  float ax[ROWS], ay[ROWS], bx[ROWS], by[ROWS], wt[ROWS];
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    ax[i] = ay[i] = bx[i] = by[i] = wt[i] = 0.f;
    if (r < P) {
      const float2 a = X1[r], c = X2[r];
      ax[i] = a.x; ay[i] = a.y; bx[i] = c.x; by[i] = c.y;
      wt[i] = W ? fmaxf(W[r], 0.f) : 1.f;
    }
  }
  const int nrows = (P + NT - 1) / NT;             // row slots in use (uniform)
  float h0[9], h[9];
  bool degenerate = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    h0[i] = H0[b * 9 + i];
    h[i] = h0[i];
    degenerate = degenerate || !(fabsf(h0[i]) <= RP_FINITE);
  }
  const float ta = tau[b], tau2 = ta * ta;
  degenerate = degenerate || !frob_unit(h) || !(ta > 0.f);
  if (degenerate) {                                // (uniform) arithmetic below stays finite; its results are not used
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = i % 4 == 0 ? 1.f : 0.f;
  }
  int phase = 0;
  // ---- start: sum of the weights, count of the positive ones, cost
  float s3[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int i = 0; i < nrows; ++i) {
    s3[0] += wt[i];
    s3[1] += wt[i] > 0.f ? 1.f : 0.f;
    s3[2] += cost_term(h, ax[i], ay[i], bx[i], by[i], wt[i], degenerate ? 1.f : tau2);
  }
  block_sum(s3, red, phase);
  const float wsum = s3[0];
  degenerate = degenerate || s3[1] < 4.f;
  if (degenerate) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (WO && r < P) WO[r] = wt[i];
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) H[b * 9 + i] = h0[i];
      stat[b * 4] = 0.f; stat[b * 4 + 1] = 0.f; stat[b * 4 + 2] = 0.f; stat[b * 4 + 3] = s3[1];
    }
    return;
  }
  float c = s3[2] / wsum, lam = LAMBDA0, accepted = 0.f;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // ---- pass 1: the normal matrix and the gradient
    float a[LMRED];
#pragma unroll
    for (int i = 0; i < LMRED; ++i) a[i] = 0.f;
#pragma unroll 1
    for (int i = 0; i < nrows; ++i) {
      const float x = ax[i], y = ay[i];
      const float m0 = h[0] * x + h[1] * y + h[2], m1 = h[3] * x + h[4] * y + h[5], m2 = h[6] * x + h[7] * y + h[8];
      const float ex = m0 - bx[i] * m2, ey = m1 - by[i] * m2, den = m2 * m2;
      const bool in = den >= DEN_MIN;               // a row mapped to infinity has no derivative
      const float inv = in ? 1.f / m2 : 0.f;
      const float d = fminf((ex * ex + ey * ey) / fmaxf(den, DEN_MIN), D_MAX);
      const float om = in ? wt[i] / (1.f + d / tau2) : 0.f;
      const float rx = ex * inv, ry = ey * inv, px = m0 * inv, py = m1 * inv;
      const float c0 = (h[0] - px * h[6]) * inv, c1 = (h[1] - px * h[7]) * inv, c2 = (h[2] - px * h[8]) * inv;
      const float e0 = (h[3] - py * h[6]) * inv, e1 = (h[4] - py * h[7]) * inv, e2 = (h[5] - py * h[8]) * inv;
      const float Jx[NPAR] = {y * c0, c0, x * c1, c1, x * c2, y * c2, x * c0 - y * c1, y * c1 - c2};
      const float Jy[NPAR] = {y * e0, e0, x * e1, e1, x * e2, y * e2, x * e0 - y * e1, y * e1 - e2};
      int m = 0;
#pragma unroll
      for (int u = 0; u < NPAR; ++u)
#pragma unroll
        for (int v = u; v < NPAR; ++v) a[m++] += om * (Jx[u] * Jx[v] + Jy[u] * Jy[v]);
#pragma unroll
      for (int u = 0; u < NPAR; ++u) a[36 + u] += om * (Jx[u] * rx + Jy[u] * ry);
    }
    block_sum(a, red, phase);
    // ---- the step and the trial H (uniform): H (I + D), D = sum delta_k G_k
    float delta[NPAR], h1[9];
    bool solved = lm_cholesky_solve(a, lam, delta);
    if (!solved) {
#pragma unroll
      for (int i = 0; i < NPAR; ++i) delta[i] = 0.f;
    }
    const float D[9] = {delta[6], delta[0], delta[1], delta[2], delta[7] - delta[6], delta[3], delta[4], delta[5], -delta[7]};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        h1[3 * r + k] = h[3 * r + k] + ((h[3 * r] * D[k] + h[3 * r + 1] * D[3 + k]) + h[3 * r + 2] * D[6 + k]);
    if (!frob_unit(h1)) {
      solved = false;
#pragma unroll
      for (int i = 0; i < 9; ++i) h1[i] = h[i];
    }
    // ---- pass 2: the trial cost
    float c1[1] = {0.f};
#pragma unroll 1
    for (int i = 0; i < nrows; ++i) c1[0] += cost_term(h1, ax[i], ay[i], bx[i], by[i], wt[i], tau2);
    block_sum(c1, red, phase);
    const float ct = c1[0] / wsum;
    if (solved && ct < c) {
#pragma unroll
      for (int i = 0; i < 9; ++i) h[i] = h1[i];
      c = ct;
      lam = fmaxf(lam / 10.f, LAMBDA_MIN);
      accepted += 1.f;
    } else {
      lam = fminf(lam * 10.f, LAMBDA_MAX);
    }
  }
  // ---- finish: the sign rule, the weights and the inlier share at the output
  sign_rule(h);
  float inl[1] = {0.f};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    if (r < P) {
      const float d = transfer(h, make_float2(ax[i], ay[i]), make_float2(bx[i], by[i]));
      inl[0] += d <= tau2 ? wt[i] : 0.f;
      if (WO) WO[r] = wt[i] / (1.f + d / tau2);
    }
  }
  block_sum(inl, red, phase);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[b * 9 + i] = h[i];
    stat[b * 4] = c; stat[b * 4 + 1] = inl[0] / wsum; stat[b * 4 + 2] = accepted; stat[b * 4 + 3] = s3[1];
  }
}

RP_DEV void matvec(const float (&m)[9], const float (&v)[3], float (&o)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o[r] = (m[3 * r] * v[0] + m[3 * r + 1] * v[1]) + m[3 * r + 2] * v[2];
}

__global__ __launch_bounds__(NT) void decompose_kernel(const float* __restrict__ H, const float* __restrict__ x1,
                                                        const float* __restrict__ x2, const float* __restrict__ w,
                                                        const float* __restrict__ tau, float vis_min, float* pose, float* normal,
                                                        float* cstat, int* pick, int P) {
  __shared__ float red[2][NW][DRED];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const float* W = w ? w + b * P : nullptr;
  // ---- H, its singular values, the scale
  float h[9];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    h[i] = H[b * 9 + i];
    bad = bad || !(fabsf(h[i]) <= RP_FINITE);
  }
  const float ta = tau[b], tau2 = ta > 0.f ? ta * ta : 1.f;
  bad = bad || !(ta > 0.f);
  if (bad) {
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = i % 4 == 0 ? 1.f : 0.f;
  }
  float u[3][3], sg[3], v[3][3];
  svd3x3_dev(h, u, sg, v);
  if (!(sg[1] > 0.f) || !(sg[1] >= RANK_MIN * sg[0]) || !(sg[0] <= RP_FINITE)) {
    bad = true;                                    // (uniform) the identity and its factors: arithmetic below stays finite
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = i % 4 == 0 ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sg[c] = 1.f;
#pragma unroll
      for (int r = 0; r < 3; ++r) u[c][r] = v[c][r] = r == c ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = h[i] / sg[1];
  // ---- the thread's rows with their Cauchy weights at H; the sign of H
  float ax[ROWS], ay[ROWS], bx[ROWS], by[ROWS], wt[ROWS], wc[ROWS];
  float s4[4] = {0.f, 0.f, 0.f, 0.f};              // sum w_c sign, sum w_c, sum w, unused
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    ax[i] = ay[i] = bx[i] = by[i] = wt[i] = wc[i] = 0.f;
    if (r < P) {
      const float2 a = X1[r], c = X2[r];
      ax[i] = a.x; ay[i] = a.y; bx[i] = c.x; by[i] = c.y;
      wt[i] = W ? fmaxf(W[r], 0.f) : 1.f;
      wc[i] = wt[i] / (1.f + transfer(h, a, c) / tau2);
      const float m0 = h[0] * a.x + h[1] * a.y + h[2], m1 = h[3] * a.x + h[4] * a.y + h[5], m2 = h[6] * a.x + h[7] * a.y + h[8];
      const float side = (c.x * m0 + c.y * m1) + m2;
      s4[0] += side > 0.f ? wc[i] : side < 0.f ? -wc[i] : 0.f;
      s4[1] += wc[i];
      s4[2] += wt[i];
    }
  }
  int phase = 0;
  block_sum(s4, red, phase);
  const float wcsum = s4[1], wsum = s4[2];
  bad = bad || !(wcsum > 0.f);
  if (s4[0] < 0.f) {
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = -h[i];
  }
  // ---- the candidates (uniform): sigma_i = (s_i / s_2)^2
  const float r1 = sg[0] / sg[1], r3 = sg[2] / sg[1];
  const float sig1 = r1 * r1, sig3 = r3 * r3, gap = sig1 - sig3;
  const bool rotation = !(gap >= ROTATION_GAP);
  float ct[4][3], cq[4][4], cn[4][3], cE[4][9], scale[4];
  bool cvalid[4];
  if (rotation) {
    // the rotation nearest to H: U diag(1, 1, det) V^T
    float R[9];
    float uc[3], vc[3];
    const float u0[3] = {u[0][0], u[0][1], u[0][2]}, u1[3] = {u[1][0], u[1][1], u[1][2]};
    const float v0[3] = {v[0][0], v[0][1], v[0][2]}, v1[3] = {v[1][0], v[1][1], v[1][2]};
    cross(u0, u1, uc);
    cross(v0, v1, vc);
    const float sgn = s4[0] < 0.f ? -1.f : 1.f;    // u of -H is -u: the first two columns change sign, their cross product does not
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * r + c] = sgn * (u0[r] * v0[c] + u1[r] * v1[c]) + uc[r] * vc[c];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cvalid[k] = k == 0;
      scale[k] = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i) ct[k][i] = cn[k][i] = 0.f;
#pragma unroll
      for (int i = 0; i < 9; ++i) cE[k][i] = 0.f;
      rot_to_quat(R, cq[k]);
    }
  } else {
    const float ca = sqrtf(fmaxf(1.f - sig3, 0.f) / gap), cb = sqrtf(fmaxf(sig1 - 1.f, 0.f) / gap);
    const float v2[3] = {v[1][0], v[1][1], v[1][2]};
    float hv2[3];
    matvec(h, v2, hv2);
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
      const float sb = pair == 0 ? cb : -cb;
      float uu[3], nn[3], hu[3], w3[3], R[9], q[4], td[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) uu[i] = ca * v[0][i] + sb * v[2][i];
      cross(v2, uu, nn);
      matvec(h, uu, hu);
      cross(hv2, hu, w3);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (hv2[r] * v2[c] + hu[r] * uu[c]) + w3[r] * nn[c];
      float hn[3], rn[3];
      matvec(h, nn, hn);
      matvec(R, nn, rn);
#pragma unroll
      for (int i = 0; i < 3; ++i) td[i] = hn[i] - rn[i];
      rot_to_quat(R, q);
      quat_to_rot(q, R);
      const float tn = sqrtf((td[0] * td[0] + td[1] * td[1]) + td[2] * td[2]);
      float tu[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) tu[i] = tn > 0.f ? td[i] / tn : 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k = 2 * pair + s;
        const float sg_ = s == 0 ? 1.f : -1.f;
        cvalid[k] = tn > 0.f && tn <= RP_FINITE;
        scale[k] = tn;
#pragma unroll
        for (int i = 0; i < 3; ++i) { ct[k][i] = sg_ * tu[i]; cn[k][i] = sg_ * nn[i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i) cq[k][i] = q[i];
        cross_times(ct[k], R, cE[k]);
      }
    }
  }
  // ---- visibility and Sampson cost of the four candidates: one fused reduction
  float s8[DRED];
#pragma unroll
  for (int i = 0; i < DRED; ++i) s8[i] = 0.f;
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {                  // (rows past P carry weight 0; static indices: nothing goes to scratch)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float front = (cn[k][0] * ax[i] + cn[k][1] * ay[i]) + cn[k][2];
      s8[2 * k] += front > 0.f ? wc[i] : 0.f;
      const float d = sampson(cE[k], make_float2(ax[i], ay[i]), make_float2(bx[i], by[i]));
      s8[2 * k + 1] += wt[i] * (tau2 * log1pf(d / tau2));
    }
  }
  block_sum(s8, red, phase);
  if (tid != 0) return;
  float vis[4], cost[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cvalid[k] = cvalid[k] && !bad;
    vis[k] = rotation ? 1.f : s8[2 * k] / wcsum;
    cost[k] = rotation ? 0.f : s8[2 * k + 1] / wsum;
    cvalid[k] = cvalid[k] && cost[k] <= RP_FINITE;    // (false for a NaN, too)
    float* PO = pose + (b * 4 + k) * 7;
    float* NO = normal + (b * 4 + k) * 3;
    float* CS = cstat + (b * 4 + k) * 4;
#pragma unroll
    for (int i = 0; i < 3; ++i) { PO[i] = cvalid[k] ? ct[k][i] : 0.f; NO[i] = cvalid[k] ? cn[k][i] : 0.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) PO[3 + i] = cvalid[k] ? cq[k][i] : 0.f;
    CS[0] = cvalid[k] ? vis[k] : 0.f;
    CS[1] = cvalid[k] ? cost[k] : 0.f;
    CS[2] = cvalid[k] ? scale[k] : 0.f;
    CS[3] = cvalid[k] ? 1.f : 0.f;
  }
  // ---- the two best: valid first, then visibility >= vis_min first, then ascending Sampson cost, then index
  int first = -1, second = -1;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    int arg = -1, argc = 2;
    float argv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cls = vis[k] >= vis_min ? 0 : 1;
      const bool open = cvalid[k] && !(round == 1 && k == first);
      if (open && (arg < 0 || cls < argc || (cls == argc && cost[k] < argv))) { arg = k; argc = cls; argv = cost[k]; }
    }
    if (round == 0) first = arg; else second = arg;
  }
  pick[b * 2] = first;
  pick[b * 2 + 1] = second;
}

}  // namespace

extern "C" int rp_homography_abi_version(void) { return RP_HOMOGRAPHY_ABI_VERSION; }

extern "C" int rp_homography_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed, float* H, int* best,
                                       float* stat, float* w_out, float* hyp_H, float* hyp_cost, int* samples, int P, int M, int n,
                                       void* stream) {
  return consensus_launch<4, RP_HOMOGRAPHY_MAX_P, RP_HOMOGRAPHY_MAX_M, hypothesis_kernel, select_kernel>(
      x1, x2, w, tau, seed, H, best, stat, w_out, hyp_H, hyp_cost, samples, P, M, n, stream);
}

extern "C" int rp_homography_refine(const float* x1, const float* x2, const float* w, const float* tau, const float* H0, int iters,
                                    float* H, float* stat, float* w_out, int P, int n, void* stream) {
  if (n <= 0 || P < 4 || iters < 0 || !x1 || !x2 || !tau || !H0 || !H || !stat) return RP_EBADSHAPE;
  if (P > RP_HOMOGRAPHY_MAX_P || iters > RP_HOMOGRAPHY_MAX_ITERS) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)H0 | (uintptr_t)H | (uintptr_t)stat | (uintptr_t)w_out) & 3) return RP_EALIGN;
  hipLaunchKernelGGL(refine_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, H0, x1, x2, w, tau, iters, H, stat, w_out, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}

extern "C" int rp_pose_from_homography(const float* H, const float* x1, const float* x2, const float* w, const float* tau, float vis_min,
                                       float* pose, float* normal, float* cstat, int* pick, int P, int n, void* stream) {
  if (n <= 0 || P < 1 || !H || !x1 || !x2 || !tau || !pose || !normal || !cstat || !pick) return RP_EBADSHAPE;
  if (P > RP_HOMOGRAPHY_MAX_P) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)H | (uintptr_t)w | (uintptr_t)tau | (uintptr_t)pose | (uintptr_t)normal | (uintptr_t)cstat | (uintptr_t)pick) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(decompose_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, H, x1, x2, w, tau, vis_min, pose, normal, cstat, pick, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
