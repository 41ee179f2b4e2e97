// rotation.hip -- the pure-rotation model behind the matches (librelpose_rotation.so): rp_rotation_consensus, rp_rotation_refine.
// include/relpose_rotation.h states all arithmetic.
//
//   hypothesis_kernel   grid n * ceil(M / 256) (problem-major), 256 threads: the staging of csrc/consensus_core.h (flags, ordered
//              prefix, compacted rows in LDS; four barriers), then one lane per hypothesis: Floyd's two draws (the core), the bearings of
//              the two rows, one orthonormal frame per image, R = sum f_i e_i^T -- a few dozen fmas, no trigonometry, every index static;
//              the lane then walks the K compacted rows (the core's cost loop, LDS broadcast reads) and sums the robust cost in a fixed
//              order.
//   select_kernel       grid n, 256 threads: the core's lowest-index argmin of hyp_cost (a tree in LDS), w_out and stat at the winner.
//   refine_kernel       grid n, 256 threads: Levenberg-Marquardt over the three parameters of a left rotation increment; the state is a
//              unit quaternion.  A thread's rows (at most 7) stay in registers; per iteration ONE fused 9-value reduction (6 of the normal
//              matrix, 3 of the gradient), the 3 x 3 Cholesky (csrc/two_view.h) and the retraction redundantly in every thread, one
//              one-value reduction for the trial cost: two barriers.
// No atomics, no workspace; the only output that is read is hyp_cost / hyp_R, by select_kernel after hypothesis_kernel wrote all of it.
#include <float.h>
#include "../csrc/common.h"
#include "../csrc/block_sum.h"
#include "../csrc/svd3x3.h"
#include "../csrc/two_view.h"
#include "../csrc/consensus_core.h"
#include "../../include/relpose_rotation.h"

namespace {

constexpr int NT = BLOCK_SUM_THREADS;                // threads per workgroup
constexpr int NW = BLOCK_SUM_WAVES;
constexpr int MAXP = RP_ROTATION_MAX_P;
constexpr int ROWS = (MAXP + NT - 1) / NT;           // rows one thread stages / owns: 7
constexpr int RED = 4;                               // floats per wave in the reduction buffer of select_kernel
constexpr int NPAR = 3;                              // degrees of freedom of R
constexpr int LMRED = NPAR * (NPAR + 1) / 2 + NPAR;  // 9: the upper triangle of the normal matrix and the gradient
constexpr float DEN_MIN = 1e-30f, D_MAX = 1e30f;     // the clamps of the distance
constexpr float LAMBDA0 = 1e-3f, LAMBDA_MIN = 1e-7f, LAMBDA_MAX = 1e7f;
constexpr float SPAN_MIN = 1e-6f;                    // |a_0 x a_1| below this: the two bearings span no plane
constexpr float SQRT3 = 1.7320508075688772f;

// the transfer distance of the homography library at H = R, and the maximum for a row that R sends behind the second camera
RP_DEV float rot_distance(const float (&h)[9], float2 a, float2 b) {
  const float m0 = h[0] * a.x + h[1] * a.y + h[2], m1 = h[3] * a.x + h[4] * a.y + h[5], m2 = h[6] * a.x + h[7] * a.y + h[8];
  const float ex = m0 - b.x * m2, ey = m1 - b.y * m2;
  const float d = fminf((ex * ex + ey * ey) / fmaxf(m2 * m2, DEN_MIN), D_MAX);
  return m2 > 0.f ? d : D_MAX;
}

// the distance of this library
struct RotationDistance {
  RP_DEV float operator()(const float (&h)[9], float2 a, float2 b) const { return rot_distance(h, a, b); }
};

// the orthonormal frame of two bearings: e[0] along their sum, e[2] along their cross product, e[1] = e[2] x e[0].  The cross product of
// two close bearings is orthogonal to their sum only to eps32 / |p0 x p1|, so e[1] is normalised and e[2] taken again as e[0] x e[1]:
// the frame is orthonormal to rounding whatever the span.  false: the bearings span no plane
RP_DEV bool frame(const float (&p0)[3], const float (&p1)[3], float (&e)[3][3]) {
  const float s[3] = {p0[0] + p1[0], p0[1] + p1[1], p0[2] + p1[2]};
  unit(s, e[0]);
  float c[3], n[3], t[3];
  cross(p0, p1, c);
  const float span = unit(c, n);
  cross(n, e[0], t);
  unit(t, e[1]);
  cross(e[0], e[1], e[2]);
  return span >= SPAN_MIN;                           // (false for a NaN, too)
}

// the two-point rotation on two rows; false: INVALID
RP_DEV bool minimal_solve(const float2 (&p1)[2], const float2 (&p2)[2], float (&h)[9]) {
  float a[2][3], b[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float va[3] = {p1[k].x, p1[k].y, 1.f}, vb[3] = {p2[k].x, p2[k].y, 1.f};
    unit(va, a[k]);
    unit(vb, b[k]);
  }
  float e[3][3], f[3][3];
  const bool oka = frame(a[0], a[1], e), okb = frame(b[0], b[1], f);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) h[3 * r + c] = (f[0][r] * e[0][c] + f[1][r] * e[1][c]) + f[2][r] * e[2][c];
  return oka && okb && all_finite(h);
}

__global__ __launch_bounds__(NT) void hypothesis_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                         const float* __restrict__ w, const float* __restrict__ tau, uint32_t seed,
                                                         float* hyp_R, float* hyp_cost, int* samples, int P, int M, int chunks) {
  __shared__ ConsensusRows<MAXP> sm;
  const long long b = blockIdx.x / chunks;
  const int m = (blockIdx.x % chunks) * NT + threadIdx.x;
  const float2* X1 = reinterpret_cast<const float2*>(x1) + b * P;
  const float2* X2 = reinterpret_cast<const float2*>(x2) + b * P;
  const int K = consensus_stage(sm, X1, X2, w ? w + b * P : nullptr, P);
  if (m >= M) return;                               // (behind the last barrier)
  uint32_t c[2];
  consensus_sample(sm, seed, b, m, M, K, samples, c);
  // ---- solve and score
  const float ta = tau[b], tau2 = ta * ta;
  float h[9], cost = FLT_MAX;
  bool valid = K >= 2 && ta > 0.f;
  if (valid) {
    float2 p1[2], p2[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      p1[k] = sm.a[c[k]];
      p2[k] = sm.b[c[k]];
    }
    valid = minimal_solve(p1, p2, h);
  }
  if (valid) {
    cost = consensus_cost(sm, h, K, tau2, RotationDistance());
    valid = cost < FLT_MAX;                         // (false for a NaN, too)
  }
  if (!valid) {
    cost = FLT_MAX;
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = 0.f;
  }
  float* HH = hyp_R + (b * M + m) * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) HH[i] = h[i];
  hyp_cost[b * M + m] = cost;
}

__global__ __launch_bounds__(NT) void select_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ w,
                                                     const float* __restrict__ tau, const float* __restrict__ hyp_R,
                                                     const float* __restrict__ hyp_cost, float* R, int* best, float* stat, float* w_out,
                                                     int P, int M) {
  __shared__ float red[2][NW][RED];
  __shared__ float bc[NT];
  __shared__ int bi[NT];
  const long long b = blockIdx.x;
  const float* HC = hyp_cost + b * M;
  float h[9], s4[4];
  const int win = consensus_select(bc, bi, reinterpret_cast<const float2*>(x1) + b * P, reinterpret_cast<const float2*>(x2) + b * P,
                                   w ? w + b * P : nullptr, w_out ? w_out + b * P : nullptr, HC, hyp_R + b * M * 9, M, P, tau[b],
                                   RotationDistance(), h, s4);
  int phase = 0;
  block_sum(s4, red, phase);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[b * 9 + i] = h[i];
    best[b] = win;
    stat[b * 4] = win >= 0 ? HC[win] : 0.f;
    stat[b * 4 + 1] = win >= 0 ? s4[1] / s4[0] : 0.f;
    stat[b * 4 + 2] = s4[3];
    stat[b * 4 + 3] = s4[2];
  }
}

// the robust cost term of one row
RP_DEV float cost_term(const float (&h)[9], float ax, float ay, float bx, float by, float wt, float tau2) {
  const float d = rot_distance(h, make_float2(ax, ay), make_float2(bx, by));
  return wt * (tau2 * log1pf(d / tau2));
}

__global__ __launch_bounds__(NT) void refine_kernel(const float* R0, const float* __restrict__ x1, const float* __restrict__ x2,
                                                     const float* __restrict__ w, const float* __restrict__ tau, int iters, float* R,
                                                     float* pose, float* stat, float* w_out, int P) {
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
  // ---- the start: R0 at Frobenius norm sqrt 3, its quaternion, the matrix of that
  float h0[9], h[9], q[4];
  bool degenerate = false;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    h0[i] = R0[b * 9 + i];
    degenerate = degenerate || !(fabsf(h0[i]) <= RP_FINITE);
    ss += h0[i] * h0[i];
  }
  const float nrm = sqrtf(ss);
  const float ta = tau[b], tau2 = ta * ta;
  degenerate = degenerate || !(nrm >= RP_MIN_SCALE) || !(nrm <= RP_FINITE) || !(ta > 0.f);
#pragma unroll
  for (int i = 0; i < 9; ++i) h[i] = degenerate ? (i % 4 == 0 ? 1.f : 0.f) : (h0[i] / nrm) * SQRT3;   // (uniform; the identity keeps the arithmetic below finite)
  rot_to_quat(h, q);
  quat_to_rot(q, h);
  const int nrows = (P + NT - 1) / NT;             // row slots in use (uniform)
  int phase = 0;
  // ---- sum of the weights, count of the positive ones, cost
  float s3[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {                  // (unrolled under a uniform guard: static indices, nothing goes to scratch)
    if (i >= nrows) break;
    s3[0] += wt[i];
    s3[1] += wt[i] > 0.f ? 1.f : 0.f;
    s3[2] += cost_term(h, ax[i], ay[i], bx[i], by[i], wt[i], degenerate ? 1.f : tau2);
  }
  block_sum(s3, red, phase);
  const float wsum = s3[0];
  degenerate = degenerate || s3[1] < 2.f;
  if (degenerate) {
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      const int r = tid + i * NT;
      if (WO && r < P) WO[r] = wt[i];
    }
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < 9; ++i) R[b * 9 + i] = h0[i];
#pragma unroll
      for (int i = 0; i < 7; ++i) pose[b * 7 + i] = 0.f;
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
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      if (i >= nrows) break;
      const float x = ax[i], y = ay[i];
      const float m0 = h[0] * x + h[1] * y + h[2], m1 = h[3] * x + h[4] * y + h[5], m2 = h[6] * x + h[7] * y + h[8];
      const float ex = m0 - bx[i] * m2, ey = m1 - by[i] * m2, den = m2 * m2;
      const bool in = m2 > 0.f && den >= DEN_MIN;   // a row behind the camera or on its horizon has no derivative
      const float inv = in ? 1.f / m2 : 0.f;
      const float dd = fminf((ex * ex + ey * ey) / fmaxf(den, DEN_MIN), D_MAX);
      const float d = m2 > 0.f ? dd : D_MAX;
      const float om = in ? wt[i] / (1.f + d / tau2) : 0.f;
      const float rx = ex * inv, ry = ey * inv, px = m0 * inv, py = m1 * inv;
      const float Jx[NPAR] = {-(px * py), 1.f + px * px, -py};
      const float Jy[NPAR] = {-(1.f + py * py), px * py, px};
      int m = 0;
#pragma unroll
      for (int u = 0; u < NPAR; ++u)
#pragma unroll
        for (int v = u; v < NPAR; ++v) a[m++] += om * (Jx[u] * Jx[v] + Jy[u] * Jy[v]);
#pragma unroll
      for (int u = 0; u < NPAR; ++u) a[6 + u] += om * (Jx[u] * rx + Jy[u] * ry);
    }
    block_sum(a, red, phase);
    // ---- the step and the trial q (uniform): unit((delta / 2, 1) (x) q)
    float delta[NPAR], q1[4], h1[9];
    bool solved = lm_cholesky_solve(a, lam, delta);
    if (!solved) {
#pragma unroll
      for (int i = 0; i < NPAR; ++i) delta[i] = 0.f;
    }
    const float px = delta[0] / 2.f, py = delta[1] / 2.f, pz = delta[2] / 2.f;
    const float v[4] = {((q[0] + px * q[3]) + py * q[2]) - pz * q[1], ((q[1] - px * q[2]) + py * q[3]) + pz * q[0],
                        ((q[2] + px * q[1]) - py * q[0]) + pz * q[3], ((q[3] - px * q[0]) - py * q[1]) - pz * q[2]};
    const float nq = unit(v, q1);
    if (!(nq > 0.f) || !(nq <= RP_FINITE)) {
      solved = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) q1[i] = q[i];
    }
    if (q1[3] < 0.f) {
#pragma unroll
      for (int i = 0; i < 4; ++i) q1[i] = -q1[i];
    }
    quat_to_rot(q1, h1);
    // ---- pass 2: the trial cost
    float c1[1] = {0.f};
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
      if (i >= nrows) break;
      c1[0] += cost_term(h1, ax[i], ay[i], bx[i], by[i], wt[i], tau2);
    }
    block_sum(c1, red, phase);
    const float ct = c1[0] / wsum;
    if (solved && ct < c) {
#pragma unroll
      for (int i = 0; i < 9; ++i) h[i] = h1[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = q1[i];
      c = ct;
      lam = fmaxf(lam / 10.f, LAMBDA_MIN);
      accepted += 1.f;
    } else {
      lam = fminf(lam * 10.f, LAMBDA_MAX);
    }
  }
  // ---- finish: the weights and the inlier share at the output
  float inl[1] = {0.f};
#pragma unroll
  for (int i = 0; i < ROWS; ++i) {
    const int r = tid + i * NT;
    if (r < P) {
      const float d = rot_distance(h, make_float2(ax[i], ay[i]), make_float2(bx[i], by[i]));
      inl[0] += d <= tau2 ? wt[i] : 0.f;
      if (WO) WO[r] = wt[i] / (1.f + d / tau2);
    }
  }
  block_sum(inl, red, phase);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) R[b * 9 + i] = h[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[b * 7 + i] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) pose[b * 7 + 3 + i] = q[i];
    stat[b * 4] = c; stat[b * 4 + 1] = inl[0] / wsum; stat[b * 4 + 2] = accepted; stat[b * 4 + 3] = s3[1];
  }
}

}  // namespace

extern "C" int rp_rotation_abi_version(void) { return RP_ROTATION_ABI_VERSION; }

extern "C" int rp_rotation_consensus(const float* x1, const float* x2, const float* w, const float* tau, int seed, float* R, int* best,
                                     float* stat, float* w_out, float* hyp_R, float* hyp_cost, int* samples, int P, int M, int n,
                                     void* stream) {
  return consensus_launch<2, RP_ROTATION_MAX_P, RP_ROTATION_MAX_M, hypothesis_kernel, select_kernel>(
      x1, x2, w, tau, seed, R, best, stat, w_out, hyp_R, hyp_cost, samples, P, M, n, stream);
}

extern "C" int rp_rotation_refine(const float* x1, const float* x2, const float* w, const float* tau, const float* R0, int iters,
                                  float* R, float* pose, float* stat, float* w_out, int P, int n, void* stream) {
  if (n <= 0 || P < 2 || iters < 0 || !x1 || !x2 || !tau || !R0 || !R || !pose || !stat) return RP_EBADSHAPE;
  if (P > RP_ROTATION_MAX_P || iters > RP_ROTATION_MAX_ITERS) return RP_EUNSUPPORTED;
  if (((uintptr_t)x1 | (uintptr_t)x2) & 7) return RP_EALIGN;
  if (((uintptr_t)w | (uintptr_t)tau | (uintptr_t)R0 | (uintptr_t)R | (uintptr_t)pose | (uintptr_t)stat | (uintptr_t)w_out) & 3)
    return RP_EALIGN;
  hipLaunchKernelGGL(refine_kernel, dim3(n), dim3(NT), 0, (hipStream_t)stream, R0, x1, x2, w, tau, iters, R, pose, stat, w_out, P);
  RP_CHECK_LAUNCH();
  return RP_OK;
}
